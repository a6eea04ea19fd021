#!/usr/bin/env python3
"""Record every call the host operator layer makes into libcambrian_amd.so, and compare two recordings.

    abi_call_trace.py record  OUT.gz [--root TREE] [TEST_FILE ...]
    abi_call_trace.py compare OLD.gz NEW.gz [--no-ptr-low]
    abi_call_trace.py same    A.gz B.gz          (two recordings of ONE tree: which fields are stable run to run)

The counterpart of ``kernel_asm_diff.py`` for the Python side: a refactor of ``cambrian_amd/ops.py`` and its neighbours must
make the same library calls, in the same order, with the same arguments.  ``record`` imports ``cambrian_amd`` from TREE
(default: the tree this file lies in), puts a recording proxy in the place of the loaded library object behind ``lib.load()``
— so it needs nothing of the tree but ``lib.load`` and ``lib.SIGNATURES`` and works on any revision — and runs the test
files in process through ``pytest.main``.  One line per call, grouped by test: the symbol, every argument rendered by its
``SIGNATURES`` type (integers and floats verbatim, pointers as ``null`` or ``set`` plus their low 9 bits, by-reference
structs field by field under the same rule) and the value returned.  ``compare`` matches the tests of both recordings by
their ids and their calls one by one; a test only one side has is listed and left out.  It only compares: it looks for no
particular call.  Exit status 1 if anything differs (``record``: the status of pytest).
"""
import argparse
import ctypes as C
import gzip
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_TESTS = [
    "test_model_gpu.py", "test_kernels_gpu.py", "test_commuted_proj_gpu.py", "test_towers_train_gpu.py", "test_hook_link_gpu.py",
    "test_residual_link_gpu.py", "test_optim_gpu.py", "test_dynamic_gpu.py", "test_decode_attn_gpu.py",
    # the symbols the nine files above do not reach
    "test_fp8_gpu.py", "test_ln_fold_gpu.py", "test_towers_gpu.py", "test_gemm_pair_gpu.py", "test_sva_gpu.py",
    "test_sva_absorbed_gpu.py", "test_resample_bwd_gpu.py", "test_weight_prep_gpu.py", "test_ln_fwd_multi_gpu.py",
]
PTR_LOW = 0x1FF


def _ptr(v) -> str:
    v = getattr(v, "value", v)
    if not v:
        return "null"
    return f"set+{int(v) & PTR_LOW:#x}"


def _value(ctype, v) -> str:
    """One value of declared type ``ctype`` as text."""
    if ctype is C.c_void_p or ctype is C.c_char_p:
        return _ptr(v)
    if isinstance(ctype, type) and issubclass(ctype, C.Structure):
        return "{" + ",".join(f"{name}={_value(ft, getattr(v, name))}" for name, ft in ctype._fields_) + "}"
    if isinstance(ctype, type) and issubclass(ctype, C.Array):
        return "[" + ",".join(_value(ctype._type_, v[i]) for i in range(ctype._length_)) + "]"
    if isinstance(ctype, type) and issubclass(ctype, C._Pointer):       # POINTER(T): byref(obj) / a pointer / None
        if v is None:
            return "null"
        obj = getattr(v, "_obj", None)
        if obj is None:
            obj = v.contents if v else None
        if obj is None:
            return "null"
        target = ctype._type_
        # a by-reference scalar is an output slot: its content before the call is not an argument
        return _value(target, obj) if issubclass(target, (C.Structure, C.Array)) else "out"
    v = getattr(v, "value", v)
    return repr(v)


class Recorder:
    """Stands in for the CDLL: ``proxy.cmb_x`` is a function that records and forwards."""

    def __init__(self, real, signatures, sink):
        self.__dict__.update(_real=real, _sigs=signatures, _sink=sink, _fns={})

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._real, name)
            sig = self._sigs.get(name)
            if sig is None:
                return real
            argtypes, sink = sig[1], self._sink

            def fn(*args, _real=real, _name=name):
                text = ",".join(_value(t, a) for t, a in zip(argtypes, args))
                rc = _real(*args)
                sink(f"{_name}({text})->{rc!r}")
                return rc
            self._fns[name] = fn
        return fn

    def __setattr__(self, name, value):
        setattr(self._real, name, value)


class _Sections:
    """pytest plugin: one ``# <test id>`` line in front of the calls of each test."""

    def __init__(self, sink):
        self.sink = sink

    def pytest_runtest_logstart(self, nodeid, location):
        self.sink("# " + nodeid)


def record(out_path, root, tests):
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    os.chdir(root)
    import pytest
    import cambrian_amd.lib as L
    assert os.path.abspath(L.__file__).startswith(root + os.sep), f"cambrian_amd came from {L.__file__}, not from {root}"
    lines = []
    real_load = L.load

    def load():
        lib = real_load()
        if not isinstance(lib, Recorder):       # (a test may have reset the handle: __graft_entry__.build())
            L._lib = lib = Recorder(lib, L.SIGNATURES, lines.append)
        return lib
    L.load = load
    rc = pytest.main(["-q", "-p", "no:cacheprovider"] + [os.path.join("tests", t) for t in tests], plugins=[_Sections(lines.append)])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
    with gzip.open(out_path, "wt") as f:
        f.write("\n".join(lines) + "\n")
    counts = {}
    for ln in lines:
        if not ln.startswith("#"):
            sym = ln.split("(", 1)[0]
            counts[sym] = counts.get(sym, 0) + 1
    used = set()
    for path in ("cambrian_amd/ops.py", "cambrian_amd/model/multimodal_encoder/vit_ops.py"):
        used |= set(re.findall(r"\bcmb_\w+", open(os.path.join(root, path)).read())) & set(L.SIGNATURES)
    summary = {"pytest_exit": int(rc), "tests": sum(ln.startswith("#") for ln in lines), "calls": sum(counts.values()),
               "symbols": dict(sorted(counts.items())), "called_by_ops_but_not_traced": sorted(used - set(counts))}
    with open(re.sub(r"\.gz$", "", out_path) + ".summary.json", "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps({k: summary[k] for k in ("pytest_exit", "tests", "calls", "called_by_ops_but_not_traced")}))
    return int(rc)


def sections(path):
    out = {"<before the first test>": []}
    cur = out["<before the first test>"]
    with gzip.open(path, "rt") as f:
        for ln in f:
            ln = ln.rstrip("\n")
            if ln.startswith("# "):
                cur = out.setdefault(ln[2:], [])
            elif ln:
                cur.append(ln)
    return out


_LOW = re.compile(r"set\+0x[0-9a-f]+")


def _fields(line):
    """A call line as a flat list of values (structs and arrays flattened in order)."""
    return [t for t in re.split(r"[(),{}\[\]]|->", line) if t]


def compare(old_path, new_path, drop_low):
    old, new = sections(old_path), sections(new_path)
    norm = (lambda s: _LOW.sub("set", s)) if drop_low else (lambda s: s)
    bad = n_calls = n_tests = 0
    for name in old:
        if name not in new:
            print(f"only in OLD  {name} ({len(old[name])} calls)")
    for name in new:
        if name not in old:
            print(f"only in NEW  {name} ({len(new[name])} calls)")
            continue
        a, b = [norm(x) for x in old[name]], [norm(x) for x in new[name]]
        n_tests += 1
        n_calls += len(b)
        if a != b:
            bad += 1
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"DIFFERS ({len(a)} vs {len(b)} calls, first at call {i})  {name}")
            print("    old: " + (a[i] if i < len(a) else "<end>"))
            print("    new: " + (b[i] if i < len(b) else "<end>"))
    print(f"{n_tests} tests on both sides, {n_calls} calls compared, pointer low bits {'dropped' if drop_low else 'compared'}, "
          f"{bad} tests differ")
    return 1 if bad else 0


def same(a_path, b_path):
    """Two recordings of one tree: name what is not stable run to run, by kind of field."""
    a, b = sections(a_path), sections(b_path)
    kinds = {"call sequence": 0, "pointer low bits": 0, "null / set": 0, "other value": 0}
    examples = {}
    calls = 0
    for name in a:
        x, y = a[name], b.get(name)
        if y is None or len(x) != len(y) or any(p.split("(", 1)[0] != q.split("(", 1)[0] for p, q in zip(x, y)):
            kinds["call sequence"] += 1
            examples.setdefault("call sequence", name)
            continue
        for p, q in zip(x, y):
            calls += 1
            if p == q:
                continue
            for u, v in zip(_fields(p), _fields(q)):
                if u == v:
                    continue
                u3, v3 = u.split("=")[-1][:3], v.split("=")[-1][:3]
                k = "pointer low bits" if u3 == v3 == "set" else "null / set" if {u3, v3} == {"nul", "set"} else "other value"
                kinds[k] += 1
                examples.setdefault(k, f"{name}: {p.split('(', 1)[0]}: {u} vs {v}")
    print(json.dumps({"tests": len(a), "calls": calls, "unstable": kinds, "examples": examples}, indent=1))
    return 1 if any(kinds.values()) else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("out")
    r.add_argument("--root", default=os.path.dirname(HERE))
    r.add_argument("tests", nargs="*")
    c = sub.add_parser("compare")
    c.add_argument("old")
    c.add_argument("new")
    c.add_argument("--no-ptr-low", action="store_true")
    s = sub.add_parser("same")
    s.add_argument("a")
    s.add_argument("b")
    a = ap.parse_args()
    if a.cmd == "record":
        return record(a.out, a.root, a.tests or DEFAULT_TESTS)
    if a.cmd == "compare":
        return compare(a.old, a.new, a.no_ptr_low)
    return same(a.a, a.b)


if __name__ == "__main__":
    sys.exit(main())
