"""The C-ABI library: loads, exports every symbol include/*.h declares,
reports a clean error without a GPU, and its host-side Philox matches the KATs.
No compute runs here (CPU-only container)."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import pytest

from helpers import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", h) for h in sorted(os.listdir(os.path.join(ROOT, "include")))
           if h.endswith(".h")]


def declared_functions():
    src = "".join(open(h).read() for h in HEADERS)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(raft_[a-z0-9_]+)\s*\(", src)
    return sorted(set(n for n in names if n != "raft_group_words"))   # static inline helper


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        importlib.import_module("raft-kotlin_amd.build").build()
    return abi.load_library()


def test_library_exports_every_declared_symbol(lib):
    decl = declared_functions()
    assert set(decl) == set(abi.EXPORTED_SYMBOLS), set(decl) ^ set(abi.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (raft_\w+)", out))
    missing = [n for n in decl if n not in exported]
    assert not missing, missing


C_TYPES = {"int16_t": C.c_int16, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64}
# records of the header that abi has as a numpy dtype only
DTYPE_ONLY = {"raft_outbox_entry": "OUTBOX_ENTRY_DTYPE", "raft_outbox_done": "OUTBOX_DONE_DTYPE"}


def header_structs() -> dict:
    """name -> [(field, ctype)] of every `typedef struct NAME { ... } NAME;` of
    include/raft_engine.h (`int64_t a, b[3];` declares two fields)."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_engine.h")).read(), flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", src, re.S):
        decls = re.findall(r"(\w+)\s+([^;]+);", body)
        assert len(decls) == body.count(";") and all(t in C_TYPES for t, _ in decls), (name, decls)
        out[name] = []
        for ctype, names in decls:
            for k in names.split(","):
                k, _, count = k.strip().partition("[")
                out[name].append((k, C_TYPES[ctype] * int(count[:-1]) if count else C_TYPES[ctype]))
    return out


def abi_structs() -> dict:
    return {k: v for k, v in vars(abi).items()
            if not k.startswith("_") and isinstance(v, type) and issubclass(v, C.Structure)}


def test_every_record_is_in_the_header_and_in_abi():
    assert set(header_structs()) == set(abi_structs()) | set(DTYPE_ONLY)
    assert len(abi_structs()) >= 40


@pytest.mark.parametrize("name", sorted(header_structs()))
def test_record_layout_equals_the_header(name):
    """Every record of the C-ABI: the ctypes.Structure has the header's fields,
    in its order and of its types; its numpy dtype has the struct's size and
    offsets; the scalar fields are all but the reserved ones and the arrays."""
    import numpy as np
    want = header_structs()[name]
    names = [k for k, _ in want]
    if name in DTYPE_ONLY:
        dtype = getattr(abi, DTYPE_ONLY[name])
        struct = type(name, (C.Structure,), {"_fields_": want})          # the header's own layout
    else:
        struct = abi_structs()[name]
        dtype = struct.dtype
        assert [(k, t._type_, getattr(t, "_length_", None)) for k, t in struct._fields_] == \
               [(k, t._type_, getattr(t, "_length_", None)) for k, t in want]
        assert struct.scalars == tuple(k for k, t in want if not hasattr(t, "_length_") and not k.startswith("reserved"))
        assert list(dtype.names) == names
        if not any(v is dtype for v in vars(abi).values()):
            return                                   # never handed out as an array (raft_params has tail padding)
    assert list(dtype.names) == names
    assert C.sizeof(struct) == dtype.itemsize
    assert [dtype.fields[k][1] for k in names] == [getattr(struct, k).offset for k in names]
    assert [dtype.fields[k][0].itemsize for k in names] == [getattr(struct, k).size for k in names]


def test_every_public_dtype_and_field_tuple_comes_from_a_record():
    """No dtype or *_FIELDS tuple of abi is stated a second time: each is a
    record's own (or one of the two outbox records checked above)."""
    import numpy as np
    structs = abi_structs().values()
    for k, v in vars(abi).items():
        if isinstance(v, np.dtype):
            assert k in DTYPE_ONLY.values() or any(v is s.dtype for s in structs), k
        elif k.endswith("_FIELDS") and isinstance(v, tuple):
            assert any(v is s.scalars for s in structs), k


def test_signature_table_is_what_the_library_binds(lib):
    """EXPORTED_SYMBOLS is the signature table, and every entry is bound."""
    assert abi.EXPORTED_SYMBOLS == list(abi.SIGNATURES)
    for name, (res, args) in abi.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes) == list(args), name


def test_library_is_gfx950(lib):
    data = open(abi.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data          # the embedded code-object bundle id


def test_abi_version_and_defaults(lib):
    assert lib.raft_abi_version() == 2
    p = abi.raft_params()
    lib.raft_params_default(C.byref(p))
    for k, v in abi.DEFAULTS.items():
        assert getattr(p, k) == v, k


def test_engine_philox_matches_kats(lib):
    eng = importlib.import_module("raft-kotlin_amd.engine")
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "philox_kat.json")))
    for v in kat["vectors"]:
        ctr = [int(x, 16) for x in v["ctr"]]
        key = [int(x, 16) for x in v["key"]]
        assert eng.philox4x32_10(ctr, key) == [int(x, 16) for x in v["out"]]


def test_create_rejects_bad_params_before_touching_a_device(lib):
    p = abi.make_params(R=9)
    h = C.c_void_p()
    assert lib.raft_engine_create(C.byref(p), 0, C.byref(h)) == abi.RAFT_EINVAL
    assert b"R must be" in lib.raft_last_error()


def test_create_without_gpu_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    eng = importlib.import_module("raft-kotlin_amd.engine")
    with pytest.raises(eng.RaftError):
        eng.RaftEngine(abi.make_params(G=4))


def test_comm_rejects_bad_arguments_before_loading_rccl(lib):
    """raft_comm_create checks its arguments before RCCL is loaded or a device
    touched (include/raft_engine.h raft_comm_*): a rank outside 0..nranks-1,
    null pointers, and (in the wrapper) an id of the wrong length."""
    eng = importlib.import_module("raft-kotlin_amd.engine")
    uid = bytes(abi.COMM_ID_BYTES)
    for nranks, rank in ((2, 2), (2, -1), (0, 0)):
        with pytest.raises(eng.RaftError, match="rank outside"):
            eng.RaftComm(uid, nranks, rank, 0)
    with pytest.raises(ValueError):
        eng.RaftComm(uid[:-1], 1, 0, 0)
    h = C.c_void_p()
    assert lib.raft_comm_create(None, 1, 0, 0, C.byref(h)) == abi.RAFT_EINVAL
    assert lib.raft_comm_get_unique_id(None) == abi.RAFT_EINVAL
    assert lib.raft_comm_destroy(None) == abi.RAFT_OK


def _unbound_engine(R=5, cap=8):
    """A RaftEngine shell without a device handle: the argument checks of the
    batch wrappers run before any library call."""
    eng = importlib.import_module("raft-kotlin_amd.engine")
    e = object.__new__(eng.RaftEngine)
    e.R, e.cap, e.G, e._h = R, cap, 4, None
    return e


@pytest.mark.parametrize("call", ["vote", "append", "command"])
def test_batch_wrappers_reject_mismatched_lengths(call):
    """group / replica / request arrays of different lengths would make the C
    side read past the shorter host buffer: the wrapper refuses."""
    e = _unbound_engine()
    g3, d2, d3 = [0, 1, 2], [0, 1], [0, 1, 2]
    with pytest.raises(ValueError):
        if call == "vote":
            e.vote_batch(g3, d2, [[1, 1, 0, 0]] * 3)
        elif call == "append":
            e.append_batch(g3, d3, [[1, 1, -1, -1, 0, 0, 0, 0]] * 2)
        else:
            e.append_command_batch(g3, d3, [7, 8])
    with pytest.raises(ValueError):
        e.vote_batch([[0, 1, 2]], d3, [[1, 1, 0, 0]] * 3)          # 2-D group index


def test_write_log_rejects_wrong_shapes():
    import numpy as np
    e = _unbound_engine(R=3, cap=8)
    with pytest.raises(ValueError):
        e.write_log(np.zeros((2, 3, 8), np.int32), np.zeros((2, 3, 4), np.uint32))
    with pytest.raises(ValueError):
        e.write_log(np.zeros((2, 2, 8), np.int32), np.zeros((2, 2, 8), np.uint32))


def test_missing_entry_points_bind_stubs(monkeypatch):
    """An experimental library (RAFT_ENGINE_LIB) without some entry point gets a
    warning per missing symbol and a stub that raises a clear error when called
    (here: the oracle's library, which exports none of the engine's symbols)."""
    other = os.path.join(ROOT, "oracle", "lib", "liboracle.so")
    if not os.path.exists(other):
        pytest.skip("oracle library not built")
    monkeypatch.setenv("RAFT_ENGINE_LIB", other)
    with pytest.warns(UserWarning, match="raft_engine_subranges"):
        lib = abi.load_library(other)
    with pytest.raises(RuntimeError, match="not in this engine build"):
        lib.raft_engine_subranges(None)


def test_host_alloc_arguments(lib):
    """raft_host_alloc refuses a non-positive size with a message; freeing NULL
    is a no-op (the page-locked allocation itself needs the HIP runtime: GPU test)."""
    assert lib.raft_host_alloc(0) is None
    assert b"positive" in lib.raft_last_error()
    assert lib.raft_host_free(None) == abi.RAFT_OK


def test_library_is_built_from_these_sources(lib):
    """The loaded engine carries the id of the sources and flags it was built
    from (build.py library_source_id), equal to the working tree's, and the
    step kernel's id bench.py keys its rocprofv3 rows on."""
    B = importlib.import_module("raft-kotlin_amd.build")
    ids = abi.build_ids()
    assert ids["library_source_id"] == B.library_source_id() == B.built_source_id()
    assert ids["kernel_source_id"] == B.kernel_source_id()
    assert not B.needs_build()


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """abi.load_library refuses a library whose compiled-in source id is not
    the working tree's (a binary that describes other code)."""
    B = importlib.import_module("raft-kotlin_amd.build")
    monkeypatch.setattr(B, "library_source_id", lambda: "0" * 12)
    with pytest.raises(RuntimeError, match="rebuild"):
        abi.check_build(abi.load_library(), abi.LIB_PATH)
