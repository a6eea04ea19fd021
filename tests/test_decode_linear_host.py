"""CPU: host side of the decode-step linear (``cmb_decode_linear``, decode_linear.hip) — symbols and ABI revision, the shape
predicate, the argument checks that run before anything is launched, the row-slab plan and the absence of a CPU path or a
backward.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_decode_linear", "cmb_decode_linear_supported", "cmb_decode_linear_plan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_symbols_are_declared_exported_and_bound_under_revision_13(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    lib = built.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in built.SIGNATURES
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    assert int(re.search(r"#define\s+CMB_ABI_VERSION\s+(\d+)", text).group(1)) == 13
    assert "cmb_decode_linear" in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert "decode_linear.hip" in open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()


def test_supported_grid(built):
    lib = built.load()
    for M in range(-1, 20):
        for N in (0, 1, 2, 3, 30, 4096, 128256):
            for K in (0, 4, 8, 12, 64, 72, 4096, 14336):
                for act in (-1, 0, 1, 2):
                    want = 1 <= M <= 16 and N >= 1 and K >= 8 and K % 8 == 0 and act in (0, 1) and not (act == 1 and N % 2)
                    assert lib.cmb_decode_linear_supported(M, N, K, act) == int(want), (M, N, K, act)
    assert lib.cmb_decode_linear_supported(1, (1 << 31) + 2, 8, 0) == 0
    assert lib.cmb_decode_linear_supported(1, 8, (1 << 31) + 8, 0) == 0


def _aligned(nbytes=256):
    raw = (C.c_char * (nbytes + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


def test_bad_arguments_are_rejected_before_any_launch(built):
    """Every case returns CMB_ERR_BAD_ARG from the host-side checks; the pointers are never dereferenced (this box may have
    no device at all, and the buffers behind them are a few bytes)."""
    lib = built.load()
    bad = -1
    keep, p = _aligned()

    def call(x=p, x_ld=64, M=3, norm=p, eps=1e-5, W=p, w_ld=64, N=32, K=64, act=0, res=p, r_ld=32, out=p, o_ld=32, f32=0):
        return lib.cmb_decode_linear(x, x_ld, M, norm, eps, W, w_ld, N, K, act, res, r_ld, out, o_ld, f32, None)

    for name in ("x", "W", "out"):
        assert call(**{name: None}) == bad, f"NULL {name}"
    assert call(M=0) == bad and call(M=17) == bad and call(M=-1) == bad
    assert call(K=60, x_ld=64, w_ld=64) == bad and call(K=0) == bad and call(K=4) == bad
    assert call(N=0) == bad
    assert call(x_ld=56) == bad and call(w_ld=56) == bad                    # shorter than K
    assert call(o_ld=24) == bad and call(r_ld=24) == bad                    # shorter than N'
    assert call(x_ld=68) == bad and call(w_ld=68) == bad and call(o_ld=36) == bad and call(r_ld=36) == bad   # not a multiple of 8
    for name in ("x", "W", "out", "norm", "res"):
        assert call(**{name: p + 2}) == bad and call(**{name: p + 8}) == bad, f"misaligned {name}"
    assert call(act=1, res=None, N=31) == bad                               # odd N with SwiGLU
    assert call(act=1, N=32) == bad                                         # SwiGLU together with a residual
    assert call(act=1, res=None, N=32, o_ld=8) == bad                       # N' = 16 > o_ld
    assert call(act=2, res=None) == bad and call(act=-1) == bad
    assert call(f32=2) == bad
    assert call(eps=-1.0) == bad and call(eps=float("nan")) == bad
    del keep


def test_plan_is_deterministic_covers_n_and_fills_the_chip(built):
    from cambrian_amd import ops
    for cus in (256, 304, 64):
        for act in (None, "swiglu"):
            for N in [2, 4, 30, 62, 64, 66, 1024, 4096, 6144, 9216, 16384, 28672, 40960, 128256]:
                for M in (1, 16):
                    rows, wgs = ops.decode_linear_plan(M, N, 4096, act, cus)
                    assert (rows, wgs) == ops.decode_linear_plan(M, N, 4096, act, cus)
                    assert (rows, wgs) == ops.decode_linear_plan(M, N, 14336, act, cus)    # today K does not enter
                    assert rows >= ops.decode_linear_plan(1, N, 4096, act, cus)[0]         # more rows of x: never a smaller slab
                    assert rows in (8, 16, 32) and not (act and rows == 8)
                    per = rows // 2 if act else rows                   # output columns a workgroup owns
                    cols = N // 2 if act else N
                    assert (wgs - 1) * per < cols <= wgs * per         # covers N' exactly: no empty workgroup, none missing
                    bigger = 2 * rows
                    if bigger <= 32:                                   # a larger slab was refused only to keep the chip filled
                        assert -(-cols // (bigger // 2 if act else bigger)) < (3 * cus // 2 if M > 4 else 2 * cus)
        for M in (1, 16):
            rows, wgs = ops.decode_linear_plan(M, 4096, 4096, None, cus)
            if cus <= 256:
                assert wgs >= 2 * cus, f"N = 4096 on {cus} CUs: {wgs} workgroups"
    assert ops.decode_linear_plan(16, 4096, 14336, None, 256) == (8, 512)          # o_proj / down_proj on an MI355X
    assert ops.decode_linear_plan(1, 128256, 4096, None, 256) == (32, 4008)        # lm_head
    assert ops.decode_linear_plan(1, 28672, 4096, "swiglu", 256) == (32, 1792 // 2)
    assert ops.decode_linear_plan(4, 7168, 20480, None, 256) == (8, 896)           # two workgroups per CU up to M = 4 ...
    assert ops.decode_linear_plan(5, 7168, 20480, None, 256) == (16, 448)          # ... one and a half above
    assert ops.decode_linear_plan(1, 4096, 4096)[0] in (8, 16, 32)                 # cus = 0: this machine's device, or 256
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_plan(17, 4096, 4096)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_plan(1, 31, 64, "swiglu")


def test_no_cpu_path_and_no_backward(built):
    from cambrian_amd import ops
    x, w = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16)
    assert not ops.decode_linear_supported(x, w, None)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear(x, w)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear(x, w, norm_weight=torch.ones(64, dtype=torch.bfloat16), eps=1e-5, act="swiglu")
    for bad in ("x", "w"):
        xx = x.clone().requires_grad_(bad == "x")
        ww = w.clone().requires_grad_(bad == "w")
        with pytest.raises(built.CambrianAmdError, match="no backward"):
            ops.decode_linear(xx, ww)
        with torch.no_grad(), pytest.raises(built.CambrianAmdError, match="CPU"):
            ops.decode_linear(xx, ww)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_plan(1, 64, 64, "gelu")


def test_switch_and_default(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "0")
    assert not ops.decode_linear_enabled(1) and not ops.decode_linear_enabled(16)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "1")
    assert ops.decode_linear_enabled(1) and ops.decode_linear_enabled(16)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_LINEAR")
    assert 0 <= ops.DECODE_LINEAR_DEFAULT_MAX_ROWS <= ops.DECODE_LINEAR_MAX_ROWS == 16
    for rows in (1, 4, 16):
        assert ops.decode_linear_enabled(rows) == (rows <= ops.DECODE_LINEAR_DEFAULT_MAX_ROWS)
