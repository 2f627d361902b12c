"""The extension header include/ext/raft_replay.h against its Python side
raft-kotlin_amd/replay.py and the library, as tests/test_abi.py holds
include/raft_engine.h to abi.py: every function the header declares is in the
module's signature table and exported by the library, every record has the
header's fields, order, types and offsets, the flag has the header's value.
The module's public surface is pinned in tests/golden/python_api_replay.json,
as tests/test_python_api_cpu.py pins abi's and engine's; a pull request that
means to change it regenerates the file:

    python tests/test_replay_abi_cpu.py --write
"""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "ext", "raft_replay.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "python_api_replay.json")
C_TYPES = {"int16_t": C.c_int16, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64}


def _mods():
    return importlib.import_module("raft-kotlin_amd.abi"), importlib.import_module("raft-kotlin_amd.replay")


def header_source() -> str:
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared_functions() -> list:
    return sorted(set(re.findall(r"\b(raft_[a-z0-9_]+)\s*\(", header_source())))


def header_structs() -> dict:
    """name -> [(field, ctype)] of every `typedef struct NAME { ... } NAME;` of the header."""
    out = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", header_source(), re.S):
        decls = re.findall(r"(\w+)\s+([^;]+);", body)
        assert len(decls) == body.count(";") and all(t in C_TYPES for t, _ in decls), (name, decls)
        out[name] = []
        for ctype, names in decls:
            for k in names.split(","):
                k, _, count = k.strip().partition("[")
                out[name].append((k, C_TYPES[ctype] * int(count[:-1]) if count else C_TYPES[ctype]))
    return out


def module_structs(rpl) -> dict:
    return {k: v for k, v in vars(rpl).items()
            if not k.startswith("_") and isinstance(v, type) and issubclass(v, C.Structure)}


def test_header_functions_are_the_modules_and_the_librarys():
    abi, rpl = _mods()
    decl = declared_functions()
    assert decl and set(decl) == set(rpl.EXPORTED_SYMBOLS) and rpl.EXPORTED_SYMBOLS == list(rpl.SIGNATURES)
    assert not set(decl) & set(abi.EXPORTED_SYMBOLS)                  # an extension: nothing declared twice
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_engine.h")).read(), flags=re.S)
    assert not any(re.search(rf"\b{n}\s*\(", main) for n in decl)
    if not os.path.exists(abi.LIB_PATH):
        importlib.import_module("raft-kotlin_amd.build").build()
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (raft_\w+)", out))
    assert not [n for n in decl if n not in exported]
    lib = rpl.bind(abi.load_library())
    for name, (res, args) in rpl.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes) == list(args), name


def test_header_records_are_the_modules():
    """Fields, order, types, sizes and offsets; the numpy dtype of the record
    agrees with the struct; scalars are all but the reserved and the arrays."""
    _, rpl = _mods()
    want, have = header_structs(), module_structs(rpl)
    assert set(want) == set(have) == {"raft_replay_info"}
    for name, fields in want.items():
        struct = have[name]
        assert [(k, t._type_, getattr(t, "_length_", None)) for k, t in struct._fields_] == \
               [(k, t._type_, getattr(t, "_length_", None)) for k, t in fields]
        ref = type(name + "_h", (C.Structure,), {"_fields_": fields})  # the header's own layout
        names = [k for k, _ in fields]
        assert C.sizeof(struct) == C.sizeof(ref) == struct.dtype.itemsize == 64
        assert [getattr(struct, k).offset for k in names] == [getattr(ref, k).offset for k in names] == \
            [struct.dtype.fields[k][1] for k in names]
        assert struct.scalars == tuple(k for k, t in fields if not hasattr(t, "_length_") and not k.startswith("reserved"))
    assert rpl.REPLAY_INFO_FIELDS is rpl.raft_replay_info.scalars


def test_header_constants_are_the_modules():
    _, rpl = _mods()
    defines = dict(re.findall(r"#define\s+(RAFT_REPLAY_\w+)\s+(\d+)", header_source()))
    assert defines == {"RAFT_REPLAY_KEEP_VOLATILE": str(rpl.REPLAY_KEEP_VOLATILE)}


def surface() -> dict:
    """The public surface of raft-kotlin_amd/replay.py as JSON would hand it back."""
    _, rpl = _mods()
    values, structs, functions = {}, {}, {}
    for name, v in sorted(vars(rpl).items()):
        if name.startswith("_") or inspect.ismodule(v):
            continue
        if isinstance(v, type) and issubclass(v, C.Structure):
            structs[name] = {"sizeof": C.sizeof(v), "fields": [[k, t.__name__, getattr(v, k).offset, getattr(v, k).size]
                                                               for k, t in v._fields_]}
        elif inspect.isfunction(v) and v.__module__ == rpl.__name__:
            functions[name] = str(inspect.signature(v))
        elif isinstance(v, (int, str, tuple, list)) and not isinstance(v, type):
            values[name] = repr(v)
    signatures = {n: {"restype": res.__name__, "argtypes": [t.__name__ for t in args]}
                  for n, (res, args) in rpl.SIGNATURES.items()}
    return json.loads(json.dumps({"values": values, "structs": structs, "functions": functions, "signatures": signatures}))


def test_module_surface_equals_the_golden_file():
    want, have = json.load(open(GOLDEN)), surface()
    assert have == want, (have, want)
    assert set(want["functions"]) >= {"bind", "replay", "replay_dev", "image_records"} and len(want["signatures"]) == 2


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
