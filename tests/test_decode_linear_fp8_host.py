"""CPU: host side of the decode-step linear on e4m3 weights (``cmb_decode_linear_fp8``, decode_linear_fp8.hip) — symbols and
ABI revision, the shape predicate, the argument checks that run before anything is launched, the row-slab plan, the absence
of a CPU path or a backward, and the opt-in switch.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_decode_linear_fp8", "cmb_decode_linear_fp8_supported", "cmb_decode_linear_fp8_plan")


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
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]       # resolves: the symbol left the library
    assert len(built.SIGNATURES["cmb_decode_linear_fp8"][1]) == len(built.SIGNATURES["cmb_decode_linear"][1]) + 1
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    assert int(re.search(r"#define\s+CMB_ABI_VERSION\s+(\d+)", text).group(1)) == 13
    assert "cmb_decode_linear_fp8" in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert "decode_linear_fp8.hip" in open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()


def test_supported_grid(built):
    lib = built.load()
    sizes = (0, 8, 16, 24, 112, 128, 144, 4096, 14336, 20480)
    for M in range(-1, 20):
        for N in sizes + (1, 2, 3, 30):
            for K in sizes:
                for act in (-1, 0, 1, 2):
                    want = 1 <= M <= 16 and N >= 1 and K >= 16 and K % 16 == 0 and act in (0, 1) and not (act == 1 and N % 2)
                    assert lib.cmb_decode_linear_fp8_supported(M, N, K, act) == int(want), (M, N, K, act)
    assert lib.cmb_decode_linear_fp8_supported(1, (1 << 31) + 2, 16, 0) == 0
    assert lib.cmb_decode_linear_fp8_supported(1, 8, (1 << 31) + 16, 0) == 0
    assert lib.cmb_decode_linear_fp8_supported(1, 1 << 31, 1 << 31, 0) == 1


def _aligned(nbytes=256):
    raw = (C.c_char * (nbytes + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


def test_bad_arguments_are_rejected_before_any_launch(built):
    """Every case returns CMB_ERR_BAD_ARG from the host-side checks; the pointers are never dereferenced (this box may have
    no device at all, and the buffers behind them are a few bytes)."""
    lib = built.load()
    bad = -1
    keep, p = _aligned()

    def call(x=p, x_ld=64, M=3, norm=p, eps=1e-5, W=p, w_ld=64, inv=p, N=32, K=64, act=0, res=p, r_ld=32, out=p, o_ld=32, f32=0):
        return lib.cmb_decode_linear_fp8(x, x_ld, M, norm, eps, W, w_ld, inv, N, K, act, res, r_ld, out, o_ld, f32, None)

    for name in ("x", "W", "inv", "out"):
        assert call(**{name: None}) == bad, f"NULL {name}"
    assert call(M=0) == bad and call(M=17) == bad and call(M=-1) == bad
    assert call(K=60) == bad and call(K=0) == bad and call(K=8) == bad
    assert call(K=24, x_ld=24, w_ld=32) == bad and call(K=56) == bad        # multiples of 8 that are no multiple of 16
    assert call(N=0) == bad
    assert call(x_ld=56) == bad and call(w_ld=48) == bad                    # shorter than K
    assert call(o_ld=24) == bad and call(r_ld=24) == bad                    # shorter than N'
    assert call(x_ld=68) == bad and call(o_ld=36) == bad and call(r_ld=36) == bad        # not a multiple of 8
    assert call(w_ld=72) == bad and call(w_ld=68) == bad                    # the byte stride: not a multiple of 16
    for name in ("x", "W", "out", "norm", "res"):
        assert call(**{name: p + 2}) == bad and call(**{name: p + 8}) == bad, f"misaligned {name}"
    assert call(inv=p + 1) == bad and call(inv=p + 2) == bad and call(inv=p + 7) == bad      # fp32: 4-byte aligned
    assert call(act=1, res=None, N=31) == bad                               # odd N with SwiGLU
    assert call(act=1, N=32) == bad                                         # SwiGLU together with a residual
    assert call(act=1, res=None, N=32, o_ld=8) == bad                       # N' = 16 > o_ld
    assert call(act=2, res=None) == bad and call(act=-1) == bad
    assert call(f32=2) == bad
    assert call(eps=-1.0) == bad and call(eps=float("nan")) == bad
    del keep


def test_plan_is_pure_covers_n_and_fills_the_chip(built):
    from cambrian_amd import ops
    for cus in (256, 304, 64):
        for act in (None, "swiglu"):
            for N in [2, 4, 30, 62, 64, 66, 1024, 4096, 6144, 9216, 16384, 28672, 40960, 128256]:
                for M in (1, 4, 5, 16):
                    rows, wgs = ops.decode_linear_fp8_plan(M, N, 4096, act, cus)
                    assert (rows, wgs) == ops.decode_linear_fp8_plan(M, N, 4096, act, cus)     # a pure function of its arguments
                    assert (rows, wgs) == ops.decode_linear_fp8_plan(M, N, 14336, act, cus)    # K does not enter
                    assert rows >= ops.decode_linear_fp8_plan(1, N, 4096, act, cus)[0]         # more rows of x: never a smaller slab
                    assert rows in (8, 16, 32) and not (act and rows == 8)
                    per = rows // 2 if act else rows                   # output columns a workgroup owns
                    cols = N // 2 if act else N
                    assert (wgs - 1) * per < cols <= wgs * per         # covers N' exactly: no empty workgroup, none missing
                    if rows < 32:                                      # a larger slab was refused only to keep the chip filled
                        assert -(-cols // (rows if act else 2 * rows)) < cus
                    if rows > (16 if act else 8):
                        assert wgs >= cus
    for M in (1, 4, 16):
        rows, wgs = ops.decode_linear_fp8_plan(M, 4096, 14336, None, 256)
        assert wgs >= 256 and rows * wgs == 4096, f"N = 4096 on 256 CUs at M = {M}: {wgs} workgroups of {rows} rows"
    assert ops.decode_linear_fp8_plan(1, 128256, 4096, None, 256) == (32, 4008)        # lm_head
    assert ops.decode_linear_fp8_plan(1, 28672, 4096, "swiglu", 256) == (32, 896)
    assert ops.decode_linear_fp8_plan(1, 4096, 4096)[0] in (8, 16, 32)                 # cus = 0: this machine's device, or 256
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp8_plan(17, 4096, 4096)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp8_plan(1, 4096, 24)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp8_plan(1, 31, 64, "swiglu")


def test_no_cpu_path_and_no_backward(built):
    from cambrian_amd import ops
    x, w = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16)
    q, inv = torch.zeros(32, 64, dtype=torch.uint8), torch.ones(32)
    assert not ops.decode_linear_fp8_supported(x, q, inv, None)
    assert not ops.decode_linear_fp8_weight_supported(2, w)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear_fp8(x, q, inv)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear_fp8(x, q, inv, norm_weight=torch.ones(64, dtype=torch.bfloat16), eps=1e-5, act="swiglu")
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_fp8_weight(w)
    xx = x.clone().requires_grad_(True)
    with pytest.raises(built.CambrianAmdError, match="no backward"):
        ops.decode_linear_fp8(xx, q, inv)
    with pytest.raises(built.CambrianAmdError, match="no backward"):
        ops.decode_linear_fp8(x, q, inv.clone().requires_grad_(True))
    with torch.no_grad(), pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear_fp8(xx, q, inv)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp8_plan(1, 64, 64, "gelu")


def test_switch_env_over_config_default_off(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8", raising=False)
    assert ops.decode_fp8_enabled() is False                       # default off
    assert ops.decode_fp8_enabled(False) is False and ops.decode_fp8_enabled(True) is True
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    assert ops.decode_fp8_enabled() and ops.decode_fp8_enabled(False) and ops.decode_fp8_enabled(True)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP8", "0")
    assert not ops.decode_fp8_enabled() and not ops.decode_fp8_enabled(True)        # the environment overrides the config
    # the bf16 path's own switch is untouched by this one
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_LINEAR", raising=False)
    assert ops.decode_linear_enabled(1) == (1 <= ops.DECODE_LINEAR_DEFAULT_MAX_ROWS)
    # the model reads config.decode_fp8_weights, absent = off
    from cambrian_amd.model.language_model import cambrian_llama
    import inspect
    assert "fp8" in inspect.signature(cambrian_llama.LlamaDecoderLayer.decode).parameters
    assert inspect.signature(cambrian_llama.LlamaDecoderLayer.decode).parameters["fp8"].default is False
