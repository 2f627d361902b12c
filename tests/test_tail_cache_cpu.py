"""The reference of the log-tail cache tests, without a GPU.

1. tail_cache_model.derive / defined against a naive per-replica loop.
2. The conditions on every input tests/test_gpu_tail_cache.py uses, on the
   oracle's state after every recorded call: no cache word below the window on a
   flat log, at most 1 % on a ring; and the facts that keep a case from going
   vacuous (ghost tails, overwrites, truncations, LOG_FULL, re-proposals, ...).
3. The extension header include/ext/raft_debug.h against its Python side
   raft-kotlin_amd/debug.py and the library, as tests/test_replay_abi_cpu.py
   does for the replay extension; the module's surface is pinned in
   tests/golden/python_api_debug.json:

    python tests/test_tail_cache_cpu.py --write
"""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tail_cache_model as TC                                       # noqa: E402
from helpers import abi, fld, handler_messages, random_ring_states, random_states   # noqa: E402

HEADER = os.path.join(ROOT, "include", "ext", "raft_debug.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "python_api_debug.json")


# ---- 1. derive and defined
def naive(state, terms, cmds, R, W):
    n = state.shape[0]
    want = np.zeros((n, R, 3), np.int32)
    ok = np.ones((n, R, 3), bool)
    for g in range(n):
        for r in range(R):
            last, phys = int(fld(state[g], R, r, "last")), int(fld(state[g], R, r, "phys"))
            lo = max(0, phys - W) if W else 0
            if last >= 1:
                want[g, r, 0] = terms[g, r, last - 1]
                want[g, r, 2] = np.uint32(cmds[g, r, last - 1]).astype(np.int32)
                ok[g, r, 0] = ok[g, r, 2] = last - 1 >= lo
            if last >= 2:
                want[g, r, 1] = terms[g, r, last - 2]
                ok[g, r, 1] = last - 2 >= lo
    return want, ok


@pytest.mark.parametrize("R", [1, 3, 5, 8])
@pytest.mark.parametrize("W", [0, 64])
def test_derive_equals_the_naive_loop(R, W):
    rng = np.random.default_rng(100 * R + W)
    cap = 160 if W else 8
    w, lt, lc = random_ring_states(rng, 300, R, cap, W) if W else random_states(rng, 300, R, cap)
    want, ok = naive(w, lt, lc, R, W)
    assert np.array_equal(TC.derive(w, lt, lc, R, W), want)
    assert np.array_equal(TC.defined(w, R, W), ok)
    last = np.stack([fld(w, R, r, "last") for r in range(R)], 1)
    assert (last == 0).any() and (last == 1).any() and (last >= 2).any()      # every rule of derive ran
    assert TC.first_mismatch(want, w, lt, lc, R, W) is None
    wrong = want.copy()
    g, r = np.argwhere(ok[:, :, 1])[0]
    wrong[g, r, 1] ^= 1
    assert f"group {g} replica {r} word t2" in TC.first_mismatch(wrong, w, lt, lc, R, W)
    if W:
        assert ok.all()                                            # random_ring_states: lastIndex within W / 2 of physLen
    else:
        assert TC.excluded_share(w, R, 0) == 0.0


def test_defined_excludes_words_below_the_window():
    """A crafted ring state: lastIndex far under physLen, at the window's edge and inside it."""
    from helpers import blank_groups, set_fld
    R, W = 3, 16
    w = blank_groups(1, R)
    for r, (last, phys) in enumerate(((10, 40), (25, 40), (26, 40))):       # the window is [24, 40)
        set_fld(w, R, r, "last", last)
        set_fld(w, R, r, "phys", phys)
    assert TC.defined(w, R, W)[0].tolist() == [[False, False, False], [True, False, True], [True, True, True]]
    assert TC.defined(w, R, 0).all()
    assert TC.excluded_share(w, R, W) == pytest.approx(4 / 9)
    with pytest.raises(AssertionError):
        TC.assert_condition(w, R, W)


@pytest.mark.parametrize("R", [3, 5, 7])
def test_ring_handler_inputs_stay_inside_the_window(R):
    """random_ring_states / handler_messages keep physLen - lastIndex under 3 W / 4."""
    W, cap, G = 64, 160, 2000
    rng = np.random.default_rng(647 + R)
    w, _, _ = random_ring_states(rng, G, R, cap, W)
    handler_messages(rng, 10_000, G, R, cap, w, W)
    gap = np.stack([fld(w, R, r, "phys") - fld(w, R, r, "last") for r in range(R)], 1)
    assert gap.max() < 3 * W // 4


# ---- 2. the conditions on the GPU file's inputs
def facts_hold(name, f):
    """What keeps scenario `name` from going vacuous."""
    rows = f.get("rows")
    if name.startswith("handlers-"):
        assert ("ring" in name) == f["wrapped"]
        assert f["ghost"] > 0 or "-tb-" in name
    elif name.startswith("consumer-"):
        assert f["accepted"] > 100 and f["refused"] > 50 and ("ring" in name) == f["wrapped"]
        assert TC._sum(rows, "leaders_elected") > 0 and TC._sum(rows, "commits") > 0
        assert TC._sum(rows, "log_window_miss") == 0
    elif name.startswith("step-"):
        assert TC._sum(rows, "log_window_miss") == 0
        assert (TC._sum(rows, "log_overflow") > 0) == ("overflow" in name)
        assert TC._sum(rows, "commands") > 0 and TC._sum(rows, "entry_writes") > 0 or name.endswith("R1")
        if re.match(r"step-ref-R[2-8]|step-general|step-balanced|step-epochs|step-catchup", name):
            assert f["ghost"] > 0 and f["shrunk"] > 0, f     # ghost tails (phys != last) and overwrites (last fell)
        if name.startswith("step-tb-"):
            assert f["shrunk"] > 0, f                           # truncations
        if "ring" in name or "epochs" in name:
            assert f["wrapped"]
        if "catchup" in name:
            assert f["lag"] >= 3
    elif name.startswith("client-propose"):
        assert f["ACCEPTED"] > 0 and f["NO_LEADER"] > 0
        if name.endswith("crafted"):
            assert f["LOG_FULL"] == 2 and f["ghost_before"] > 0 and (f["GHOSTED"] == 2) == ("-ref-" in name)
    elif name.startswith("client-noops"):
        assert f["appended"] > 0
        if name.endswith("crafted"):
            assert f["log_full"] == 1 and f["ghosted"] == ("-ref-" in name)
    elif name.startswith("outbox-"):
        assert f["retried"] > 0 and f["accepted"] > 0 and (f["ghosted"] > 0) == ("-ref-" in name)
    elif name.startswith("restart-"):
        assert f["restarted"] > 0 and f["random"] > 0 and f["spared"] > 0 and f["kept"]
        assert (f["emptied"] > 0) == name.endswith("amnesia")
    elif name.startswith("install-"):
        assert f["installed"] > 0 and f["shorter"] > 0
        assert (f["ring_full"] > 0) == ("ring" in name)           # the leader's floor is above 0
    elif name.startswith("replay-"):
        assert f["malformed"] == 0 and f["hardstates"] > 0 and f["truncates"] > 0 and f["entries"] > 2000
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("name", list(TC.SCENARIOS))
def test_inputs_meet_the_conditions(name):
    run = TC.host_run(name)
    W = run["W"]
    assert any(c["name"] in TC.WRITERS for c in run["trace"])
    for k, c in enumerate(run["trace"]):
        assert c["share"] == 0.0 if not W else c["share"] <= TC.EXCLUDED_MAX, (name, k, c["name"], c["share"])
    TC.assert_condition(run["state"], run["R"], W, name)
    facts_hold(name, run["facts"])


def test_every_writer_has_a_scenario():
    called = {c["name"] for name in TC.SCENARIOS for c in TC.host_run(name)["trace"]}
    assert TC.WRITERS - {"transfer"} <= called


# ---- 3. the header against the binding and the library
def _mods():
    return importlib.import_module("raft-kotlin_amd.abi"), importlib.import_module("raft-kotlin_amd.debug")


def header_source() -> str:
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared() -> dict:
    """name -> (return type, [argument types]) of every function the header declares."""
    out = {}
    for ret, name, args in re.findall(r"\b(\w+)\s+(raft_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_source()):
        out[name] = (ret, [re.sub(r"\s*\w+\s*$", "", a.strip()).replace(" ", "") for a in args.split(",")])
    return out


C_ARG = {"raft_engine*": C.c_void_p, "int64_t": C.c_int64, "int32_t*": C.POINTER(C.c_int32), "int": C.c_int}


def test_header_function_is_the_modules_and_the_librarys():
    abi_, dbg = _mods()
    decl = declared()
    assert list(decl) == ["raft_debug_read_tail_cache"] == dbg.EXPORTED_SYMBOLS == list(dbg.SIGNATURES)
    assert not set(decl) & set(abi_.EXPORTED_SYMBOLS)              # an extension: nothing declared twice
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_engine.h")).read(), flags=re.S)
    assert not any(re.search(rf"\b{n}\s*\(", main) for n in decl)
    for name, (ret, args) in decl.items():                          # the header's types are the binding's
        res, argtypes = dbg.SIGNATURES[name]
        assert C_ARG[ret] is res and [C_ARG[a] for a in args] == list(argtypes), (name, ret, args)
    if not os.path.exists(abi_.LIB_PATH):
        importlib.import_module("raft-kotlin_amd.build").build()
    out = subprocess.run(["nm", "-D", "--defined-only", abi_.LIB_PATH], capture_output=True, text=True).stdout
    assert set(decl) <= set(re.findall(r" T (raft_\w+)", out))
    lib = dbg.bind(abi_.load_library())
    for name, (res, args) in dbg.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes) == list(args), name
    assert not re.findall(r"typedef struct|#define\s+RAFT_DEBUG", header_source())   # one function, nothing else
    assert dbg.TAIL_CACHE_WORDS == TC.WORDS


def surface() -> dict:
    """The public surface of raft-kotlin_amd/debug.py as JSON would hand it back."""
    _, dbg = _mods()
    values, functions = {}, {}
    for name, v in sorted(vars(dbg).items()):
        if name.startswith("_") or inspect.ismodule(v):
            continue
        if inspect.isfunction(v) and v.__module__ == dbg.__name__:
            functions[name] = str(inspect.signature(v))
        elif isinstance(v, (int, str, tuple, list)) and not isinstance(v, type):
            values[name] = repr(v)
    signatures = {n: {"restype": res.__name__, "argtypes": [t.__name__ for t in args]}
                  for n, (res, args) in dbg.SIGNATURES.items()}
    return json.loads(json.dumps({"values": values, "functions": functions, "signatures": signatures}))


def test_module_surface_equals_the_golden_file():
    want, have = json.load(open(GOLDEN)), surface()
    assert have == want, (have, want)
    assert set(want["functions"]) == {"bind", "read_tail_cache"} and len(want["signatures"]) == 1


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
