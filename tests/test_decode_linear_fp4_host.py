"""CPU: host side of the MXFP4 decode-step linear (``cmb_decode_linear_fp4``, ``cmb_quantize_mxfp4_rows``) — symbols, the shape
predicate, the status of every bad argument before anything is launched (``cmb_decode_step`` with ``fp8`` = 2 / 3 included),
the row-slab plan, the switch, and the properties of the CPU restatement of the format (tests/mxfp4_ref.py) that the GPU
tests quantise with.  No kernel is launched here.

Quantiser bound, per element, with e the block's exponent and u = 2^e: a value that is not clamped (|w| <= 6 u) lands on a
neighbouring grid point, so |w - deq| <= half the local grid spacing times u (spacing 0.5 below 2, 1 from 2 to 4, 2 from 4 to
6); a clamped one (6 u < |w| < 8 u, amax < 8 u by the choice of e) is off by less than 2 u.  Both follow from the rule, not
from the kernel.  The relative L2 error on N(0, 0.02^2) weights is printed and only asserted below 0.15 (a numpy experiment
gave 0.114; the margin covers other seeds)."""
import ctypes as C
import os
import re

import pytest
import torch

import mxfp4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_decode_linear_fp4", "cmb_decode_linear_fp4_supported", "cmb_decode_linear_fp4_plan", "cmb_quantize_mxfp4_rows")
BAD_ARG, ALIGNMENT, SHAPE, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_symbols_are_declared_exported_and_bound(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    lib = built.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in built.SIGNATURES
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]       # resolves: the symbol left the library
        assert name in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    # the e4m3 form's arguments with the row factors replaced by (scale bytes, their row stride)
    assert len(built.SIGNATURES["cmb_decode_linear_fp4"][1]) == len(built.SIGNATURES["cmb_decode_linear_fp8"][1]) + 1
    assert built.ABI_VERSION == lib.cmb_abi_version()
    mk = open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()
    assert "decode_linear_fp4.hip" in mk and "mxfp4.hip" in mk


def test_supported_grid(built):
    lib = built.load()
    sizes = (0, 8, 16, 32, 48, 64, 224, 256, 288, 4096, 14336, 20480)
    for M in range(-1, 20):
        for N in sizes + (1, 2, 3, 30):
            for K in sizes:
                for act in (-1, 0, 1, 2):
                    want = 1 <= M <= 16 and N >= 1 and K >= 32 and K % 32 == 0 and act in (0, 1) and not (act == 1 and N % 2)
                    assert lib.cmb_decode_linear_fp4_supported(M, N, K, act) == int(want), (M, N, K, act)
    assert lib.cmb_decode_linear_fp4_supported(1, 8, 48, 0) == 0 and lib.cmb_decode_linear_fp8_supported(1, 8, 48, 0) == 1
    assert lib.cmb_decode_linear_fp4_supported(1, (1 << 31) + 2, 32, 0) == 0
    assert lib.cmb_decode_linear_fp4_supported(1, 8, (1 << 31) + 32, 0) == 0
    assert lib.cmb_decode_linear_fp4_supported(1, 1 << 31, 1 << 31, 0) == 1


def _aligned(nbytes=256):
    raw = (C.c_char * (nbytes + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


def test_linear_bad_arguments_are_rejected_before_any_launch(built):
    """Every case returns CMB_ERR_BAD_ARG from the host-side checks; the pointers are never dereferenced (this box may have
    no device at all, and the buffers behind them are a few bytes)."""
    lib = built.load()
    bad = BAD_ARG
    keep, p = _aligned()

    def call(x=p, x_ld=64, M=3, norm=p, eps=1e-5, W=p, w_ld=32, S=p, s_ld=2, N=32, K=64, act=0, res=p, r_ld=32, out=p, o_ld=32,
             f32=0):
        return lib.cmb_decode_linear_fp4(x, x_ld, M, norm, eps, W, w_ld, S, s_ld, N, K, act, res, r_ld, out, o_ld, f32, None)

    for name in ("x", "W", "S", "out"):
        assert call(**{name: None}) == bad, f"NULL {name}"
    assert call(M=0) == bad and call(M=17) == bad and call(M=-1) == bad
    assert call(K=60) == bad and call(K=0) == bad and call(K=8) == bad and call(K=16) == bad
    assert call(K=48, x_ld=48, w_ld=32, s_ld=2) == bad                      # a multiple of 16 (the e4m3 kernel takes it), not of 32
    assert call(K=-32) == bad
    assert call(N=0) == bad
    assert call(x_ld=56) == bad and call(w_ld=16) == bad and call(s_ld=1) == bad         # shorter than K, K / 2, K / 32
    assert call(o_ld=24) == bad and call(r_ld=24) == bad                    # shorter than N'
    assert call(x_ld=68) == bad and call(o_ld=36) == bad and call(r_ld=36) == bad        # not a multiple of 8
    assert call(w_ld=40) == bad and call(w_ld=36) == bad                    # the byte stride: not a multiple of 16
    for name in ("x", "W", "out", "norm", "res"):
        assert call(**{name: p + 2}) == bad and call(**{name: p + 8}) == bad, f"misaligned {name}"
    assert call(act=1, res=None, N=31) == bad                               # odd N with SwiGLU
    assert call(act=1, N=32) == bad                                         # SwiGLU together with a residual
    assert call(act=1, res=None, N=32, o_ld=8) == bad                       # N' = 16 > o_ld
    assert call(act=2, res=None) == bad and call(act=-1) == bad
    assert call(f32=2) == bad
    assert call(eps=-1.0) == bad and call(eps=float("nan")) == bad
    # the plan query's own refusals
    rows, wgs = C.c_int32(0), C.c_int64(0)
    for M, N, K, act, cus in ((0, 32, 64, 0, 256), (17, 32, 64, 0, 256), (1, 0, 64, 0, 256), (1, 32, 48, 0, 256), (1, 31, 64, 1, 256),
                              (1, 32, 64, 2, 256), (1, 32, 64, 0, -1)):
        assert lib.cmb_decode_linear_fp4_plan(M, N, K, act, cus, C.byref(rows), C.byref(wgs)) == bad, (M, N, K, act, cus)
    assert lib.cmb_decode_linear_fp4_plan(1, 32, 64, 0, 256, None, None) == 0
    del keep


def test_quantiser_bad_arguments_are_rejected_before_any_launch(built):
    lib = built.load()
    keep, p = _aligned()

    def call(dtype=0, x=p, ldx=64, rows=4, K=64, q=p, ldq=32, s=p, lds=2):
        return lib.cmb_quantize_mxfp4_rows(dtype, x, ldx, rows, K, q, ldq, s, lds, None)

    assert call(rows=0) == 0                                                # nothing to do, as cmb_quantize_fp8_rows
    for name in ("x", "q", "s"):
        assert call(**{name: None}) == BAD_ARG, f"NULL {name}"
    assert call(rows=-1) == BAD_ARG and call(K=0) == BAD_ARG and call(K=-32) == BAD_ARG
    assert call(dtype=2) == BAD_ARG and call(dtype=3) == BAD_ARG and call(dtype=-1) == BAD_ARG
    assert call(K=48, ldx=48) == SHAPE and call(K=16, ldx=16) == SHAPE
    assert call(ldx=56) == SHAPE and call(ldq=16) == SHAPE and call(ldq=40) == SHAPE and call(lds=1) == SHAPE
    assert call(x=p + 2) == ALIGNMENT and call(q=p + 8) == ALIGNMENT
    assert call(ldx=68) == ALIGNMENT                                        # bf16 rows 136 bytes apart
    assert call(dtype=1, ldx=66) == ALIGNMENT                               # fp32 rows 264 bytes apart
    del keep


GEO = dict(B=3, H=256, I=512, nh=4, nkv=2, hd=64)


def _step_case(built, fp8, layers=2):
    keep, p = _aligned()
    table = (built.DecodeLayer * layers)()
    for row in table:
        for name, ld in (("qkv", 128), ("o", 128), ("gate_up", 128), ("down", 256)):        # bytes of two e2m1 each: K / 2
            setattr(row, "w_" + name, p)
            setattr(row, "ld_" + name, ld)
            setattr(row, "w_" + name + "_scale", p)
        row.norm1 = row.norm2 = row.kcache = row.vcache = p
    desc = built.DecodeStepDesc(layers=layers, fp8=fp8, V=64, eps=1e-5, scale=0.125, c_sb=2 * 64 * 64, c_sh=64 * 64, c_st=64,
                                final_norm=p, head=p, ld_head=128, head_scale=p, **GEO)
    return keep, p, desc, table


def test_step_takes_format_2_and_refuses_every_other_value(built):
    """fp8 = 2 passes every check up to the workspace (one float short: nothing is launched); 3, -1 and 255 are
    CMB_ERR_BAD_ARG; with fp8 = 2 the MXFP4 rules hold: K % 32, byte strides of K / 2, scale pointers present and free of any
    alignment rule."""
    lib = built.load()
    t = 36
    need = lib.cmb_decode_step_ws(*GEO.values(), t)
    assert need > 0

    def call(desc, table, p, ws_floats=need - 1):
        return lib.cmb_decode_step(C.byref(desc), table, p + (1 << 20), 256, p, p, t, p, 64, p, ws_floats, p, 64, None)

    keep, p, desc, table = _step_case(built, 2)
    assert call(desc, table, p) == WORKSPACE
    for value in (3, -1, 4, 255):
        k2, p2, d2, t2 = _step_case(built, value)
        assert call(d2, t2, p2) == BAD_ARG, f"fp8 = {value}"
    k2, p2, d2, t2 = _step_case(built, 2)
    t2[1].w_o_scale = None
    assert call(d2, t2, p2) == BAD_ARG
    t2[1].w_o_scale = p2 + 1                                                # bytes: any address
    assert call(d2, t2, p2) == WORKSPACE
    t2[0].ld_down = 240                                                     # < I / 2 = 256
    assert call(d2, t2, p2) == BAD_ARG
    t2[0].ld_down = 264                                                     # not a multiple of 16
    assert call(d2, t2, p2) == BAD_ARG
    k3, p3, d3, t3 = _step_case(built, 2)
    d3.head_scale = None
    assert call(d3, t3, p3) == BAD_ARG
    k3, p3, d3, t3 = _step_case(built, 2)
    d3.H = 272                                                              # K % 16 == 0 (fine for e4m3), K % 32 != 0
    d3.hd = 68
    assert call(d3, t3, p3) == BAD_ARG
    k3, p3, d3, t3 = _step_case(built, 2)
    t3[1].w_down = p3 + 8
    assert call(d3, t3, p3) == ALIGNMENT
    del keep, k2, k3


def test_plan_is_pure_covers_n_and_fills_the_chip(built):
    from cambrian_amd import ops
    for cus in (256, 304, 64):
        for act in (None, "swiglu"):
            prev = 0
            for N in [2, 4, 30, 62, 64, 66, 1024, 4096, 6144, 9216, 16384, 28672, 40960, 128256]:
                for M in (1, 4, 5, 16):
                    rows, wgs = ops.decode_linear_fp4_plan(M, N, 4096, act, cus)
                    assert (rows, wgs) == ops.decode_linear_fp4_plan(M, N, 4096, act, cus)     # a pure function of its arguments
                    assert (rows, wgs) == ops.decode_linear_fp4_plan(M, N, 20480, act, cus)    # K does not enter
                    assert rows in (8, 16, 32) and not (act and rows == 8)
                    per = rows // 2 if act else rows                   # output columns a workgroup owns
                    cols = N // 2 if act else N
                    assert (wgs - 1) * per < cols <= wgs * per         # covers N' exactly: no empty workgroup, none missing
                    if rows > (16 if act else 8):
                        assert wgs >= cus
                assert rows >= prev                                    # monotone in N
                prev = rows
    assert ops.decode_linear_fp4_plan(1, 128256, 4096, None, 256) == (32, 4008)        # lm_head
    assert ops.decode_linear_fp4_plan(1, 28672, 4096, "swiglu", 256) == (32, 896)
    assert ops.decode_linear_fp4_plan(16, 7168, 20480, None, 256)[0] in (8, 16)        # Yi-34B down_proj: taken
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp4_plan(17, 4096, 4096)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp4_plan(1, 4096, 48)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_fp4_plan(1, 31, 64, "swiglu")


def test_no_cpu_path_and_no_backward(built):
    from cambrian_amd import ops
    x, w = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16)
    q, s = torch.zeros(32, 32, dtype=torch.uint8), torch.full((32, 2), 127, dtype=torch.uint8)
    assert not ops.decode_linear_fp4_supported(x, q, s, None)
    assert not ops.decode_linear_fp4_weight_supported(2, w)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear_fp4(x, q, s)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_fp4_weight(w)
    with pytest.raises(built.CambrianAmdError, match="no backward"):
        ops.decode_linear_fp4(x.clone().requires_grad_(True), q, s)


def test_switch_env_over_config_default_off_and_both_raise(built, monkeypatch):
    from types import SimpleNamespace
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP4", raising=False)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8", raising=False)
    assert ops.decode_fp4_enabled() is False                       # unset: off
    assert ops.decode_fp4_enabled(False) is False and ops.decode_fp4_enabled(True) is True
    assert ops.decode_weight_format(SimpleNamespace()) is None
    assert ops.decode_weight_format(SimpleNamespace(decode_fp4_weights=True)) == "fp4"
    assert ops.decode_weight_format(SimpleNamespace(decode_fp8_weights=True)) == "fp8"
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "1")
    assert ops.decode_fp4_enabled() and ops.decode_fp4_enabled(False) and ops.decode_fp4_enabled(True)
    assert ops.decode_weight_format(SimpleNamespace()) == "fp4"
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "0")
    assert not ops.decode_fp4_enabled() and not ops.decode_fp4_enabled(True)        # the environment overrides the config
    assert ops.decode_weight_format(SimpleNamespace(decode_fp4_weights=True)) is None
    # both modes on, from whichever source: an error that names both switches
    for env8, env4, cfg in (("1", "1", SimpleNamespace()), (None, "1", SimpleNamespace(decode_fp8_weights=True)),
                            ("1", None, SimpleNamespace(decode_fp4_weights=True)),
                            (None, None, SimpleNamespace(decode_fp8_weights=True, decode_fp4_weights=True))):
        for name, v in (("CAMBRIAN_AMD_DECODE_FP8", env8), ("CAMBRIAN_AMD_DECODE_FP4", env4)):
            monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, v)
        with pytest.raises(built.CambrianAmdError) as err:
            ops.decode_weight_format(cfg)
        for word in ("decode_fp8_weights", "CAMBRIAN_AMD_DECODE_FP8", "decode_fp4_weights", "CAMBRIAN_AMD_DECODE_FP4"):
            assert word in str(err.value)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "0")
    assert ops.decode_weight_format(SimpleNamespace(decode_fp4_weights=True)) == "fp8"          # the environment switched one off
    # the model's entry points carry the format beside fp8, default off; fp8's stay what they were
    import inspect
    from cambrian_amd.model.language_model import cambrian_llama, cambrian_phi3
    for fn in (cambrian_llama.LlamaDecoderLayer.decode, cambrian_llama.LlamaDecoderLayer.decode_operands,
               cambrian_phi3.Phi3DecoderLayer.decode, cambrian_phi3.Phi3DecoderLayer.decode_operands,
               cambrian_llama._decode_logits, cambrian_llama.DecodeStepPlan.build):
        par = inspect.signature(fn).parameters
        assert par["fp4"].default is False and "fp8" in par, fn
    assert inspect.signature(cambrian_llama.decode_layer_fused).parameters["fp4"].default is None


# ---- the CPU restatement of the format ----
def _bound(w, e):
    """Per element: half the local grid spacing times 2^e where the value is not clamped, 2 x 2^e where it is."""
    u = torch.ldexp(torch.ones((), dtype=torch.float64), e.to(torch.int32)).repeat_interleave(R.BLOCK, dim=1)
    a = w.double().abs() / u
    half = torch.where(a <= 2, 0.25, torch.where(a <= 4, 0.5, 1.0))
    return torch.where(a <= 6, half, torch.full_like(a, 2.0)) * u, a > 6


def test_reference_quantiser_on_gaussian_weights():
    g = torch.Generator().manual_seed(7)
    for dt in (torch.float32, torch.bfloat16):
        w = (torch.randn(256, 4096, generator=g) * 0.02).to(dt)
        q, s = R.quantize(w)
        assert q.shape == (256, 2048) and s.shape == (256, 128) and q.dtype == s.dtype == torch.uint8
        assert int(s.min()) >= 1 and int(s.max()) <= 254
        e = s.to(torch.int32) - 127
        assert torch.equal(e, R.block_exponent(w))
        deq = R.dequantize(q, s)
        err = (deq - w.double()).abs()
        bound, clamped = _bound(w, e)
        assert bool((err[~clamped] <= bound[~clamped]).all()), "an unclamped value is further than half a grid step away"
        assert bool((err[clamped] < bound[clamped]).all()), "a clamped value is 2 x 2^e away or more"
        assert bool(clamped.any()), "the Gaussian case is meant to contain clamped values (amax in (6, 8) 2^e)"
        # every block's amax lies in [4, 8) 2^e
        amax = w.double().abs().reshape(256, 128, 32).amax(-1) / torch.ldexp(torch.ones((), dtype=torch.float64), e)
        assert bool(((amax >= 4) & (amax < 8)).all())
        rel = float((deq - w.double()).norm() / w.double().norm())
        print(f"MXFP4 on N(0, 0.02^2) [256, 4096] {dt}: relative L2 error {rel:.4f}, clamped {float(clamped.double().mean()):.4f}")
        assert rel < 0.15
        # every dequantised value is exactly a bf16
        assert torch.equal(deq.to(torch.bfloat16).double(), deq)


def test_reference_quantiser_on_hand_made_blocks():
    K = 64
    w = torch.zeros(8, K)
    w[1, 5] = 3.0                        # a single non-zero: floor(log2 3) = 1, e = -1, 3 / 2^-1 = 6
    w[2, 40] = -4.0                      # floor(log2 4) = 2, e = 0: magnitude 4
    w[3, 0] = 2.0 ** -130                # subnormal amax: e clamps at -126
    w[4, :32] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] * 4) * 2.0 ** -3      # ties, amax 6 -> e = 0 - 3
    w[5, :32] = torch.tensor([7.0] + [-0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0] + [0.0] * 24) * 4.0   # amax 7 x 2^e: clamps
    w[6, :32] = torch.tensor([3.9990234375] + [1.0] * 31)                   # just below 4: e = -1, 7.998 -> clamps to 6
    w[7, 33] = -0.0
    q, s = R.quantize(w)
    codes, e = R.unpack(q), s.to(torch.int32) - 127
    assert int(s[0, 0]) == 127 and int(s[0, 1]) == 127 and not q[0].any()            # a zero block: code 127, zero nibbles
    assert int(s[7, 1]) == 127 and not q[7].any()                                     # -0 is a zero block too, written +0
    assert int(e[1, 0]) == -1 and int(codes[1, 5]) == 7 and int(codes[1].count_nonzero()) == 1     # 6 x 2^-1
    assert int(e[2, 1]) == 0 and int(codes[2, 40]) == (8 | 6) and int(codes[2].count_nonzero()) == 1      # -4 x 2^0
    assert int(s[3, 0]) == 1 and int(codes[3, 0]) == 0                                # 2^-130 / 2^-126 = 1/16: rounds to 0
    # ties go to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4; 6 stays
    # (amax = 6 x 2^-3 = 0.75: floor(log2 0.75) = -1, e = -3)
    assert int(e[4, 0]) == -3
    assert codes[4, :8].tolist() == [0, 2, 2, 4, 4, 6, 6, 7]
    assert R.dequantize(q, s)[4, :8].tolist() == [v * 2.0 ** -3 for v in (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0)]
    # amax 28 = 7 x 2^2: floor(log2 28) = 4, e = 2; 7 clamps to 6; negative ties mirror the positive ones, -0.25 becomes +0
    assert int(e[5, 0]) == 2 and codes[5, :8].tolist() == [7, 0, 8 | 2, 8 | 2, 8 | 4, 8 | 4, 8 | 6, 8 | 6]
    assert int(e[6, 0]) == -1 and int(codes[6, 0]) == 7 and codes[6, 1:32].tolist() == [4] * 31
    assert int(s.min()) >= 1 and int(s.max()) <= 254
