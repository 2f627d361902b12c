"""The Python binding's public surface, pinned: what `abi` and `engine` offer
equals tests/golden/python_api.json -- the constants, the records' layouts,
the signature bound to every entry point of the library, and the signature of
every public method.  A refactor of the binding keeps the file untouched; a
pull request that means to change the surface regenerates it:

    python tests/test_python_api_cpu.py --write
"""
import ctypes as C
import importlib
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "python_api.json")

# where the package lies on this machine: not part of the surface
PATHS = ("PKG_DIR", "LIB_PATH")
ENGINE_NAMES = ("RaftError", "RaftComm", "RaftAudit", "RaftMonitor", "RaftWal", "WalImage", "RaftEngine",
                "philox4x32_10")


def _plain(v) -> bool:
    """An int, a str, None, or a tuple, list or dict of those."""
    if v is None or isinstance(v, (int, str)):
        return True
    if isinstance(v, (tuple, list)):
        return all(_plain(x) for x in v)
    if isinstance(v, dict):
        return all(_plain(k) and _plain(x) for k, x in v.items())
    return False


def _tname(t) -> str:
    return "None" if t is None else t.__name__


def _abi_surface(abi) -> dict:
    values, dtypes, structs = {}, {}, {}
    for name, v in sorted(vars(abi).items()):
        if name.startswith("_") or name in PATHS:
            continue
        if isinstance(v, np.dtype):
            dtypes[name] = {"descr": v.descr, "itemsize": v.itemsize,
                            "offsets": {k: v.fields[k][1] for k in v.names}}
        elif isinstance(v, type) and issubclass(v, C.Structure):
            structs[name] = {"sizeof": C.sizeof(v),
                             "fields": [[k, t.__name__, getattr(v, k).offset, getattr(v, k).size]
                                        for k, t in v._fields_]}
        elif _plain(v):
            values[name] = repr(v)                   # a tuple stays a tuple, an int key an int
    lib = abi.load_library()
    signatures = {}
    for name in abi.EXPORTED_SYMBOLS:
        f = getattr(lib, name)
        signatures[name] = {"restype": _tname(f.restype), "argtypes": [_tname(t) for t in f.argtypes]}
    return {"values": values, "dtypes": dtypes, "structs": structs, "signatures": signatures}


def _member(cls, name) -> dict:
    raw = inspect.getattr_static(cls, name)
    if isinstance(raw, property):
        return {"kind": "property", "signature": str(inspect.signature(raw.fget)), "setter": raw.fset is not None}
    kind = "staticmethod" if isinstance(raw, staticmethod) else "classmethod" if isinstance(raw, classmethod) else "method"
    return {"kind": kind, "signature": str(inspect.signature(getattr(cls, name)))}


def _engine_surface(eng) -> dict:
    out = {}
    for name in ENGINE_NAMES:
        obj = getattr(eng, name)
        if not isinstance(obj, type):
            out[name] = {"kind": "function", "signature": str(inspect.signature(obj))}
            continue
        members = {}
        for m in dir(obj):
            if m.startswith("_") and m != "__init__":
                continue
            raw = inspect.getattr_static(obj, m)
            if isinstance(raw, (property, staticmethod, classmethod)) or inspect.isfunction(raw):
                members[m] = _member(obj, m)
        out[name] = {"kind": "class", "bases": [b.__name__ for b in obj.__bases__], "members": members}
    return out


def surface() -> dict:
    """The surface of the modules as they are now, as JSON would hand it back."""
    abi = importlib.import_module("raft-kotlin_amd.abi")
    eng = importlib.import_module("raft-kotlin_amd.engine")
    return json.loads(json.dumps({"abi": _abi_surface(abi), "engine": _engine_surface(eng)}))


def _diff(have, want, path="") -> list:
    """The paths at which two JSON values differ (for a readable failure)."""
    if isinstance(have, dict) and isinstance(want, dict):
        out = []
        for k in sorted(set(have) | set(want)):
            if k not in have or k not in want:
                out.append(f"{path}/{k}: {'missing' if k not in have else 'not in the golden file'}")
            else:
                out += _diff(have[k], want[k], f"{path}/{k}")
        return out
    return [] if have == want else [f"{path}: {have!r} != {want!r}"]


def test_python_surface_equals_the_golden_file():
    want = json.load(open(GOLDEN))
    have = surface()
    assert have == want, "\n".join(_diff(have, want)[:40])


def test_golden_file_covers_what_it_claims():
    """The pin is not vacuous: every kind of thing is in it, and in numbers."""
    want = json.load(open(GOLDEN))
    a = want["abi"]
    assert len(a["values"]) >= 150 and len(a["dtypes"]) >= 22 and len(a["structs"]) >= 40 and len(a["signatures"]) >= 134
    assert a["structs"]["raft_outbox_info"]["fields"][-1][:2] == ["age_hist", "c_long_Array_32"]
    assert set(want["engine"]) == set(ENGINE_NAMES)
    assert len(want["engine"]["RaftEngine"]["members"]) >= 90
    assert not any(p in a["values"] for p in PATHS)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
