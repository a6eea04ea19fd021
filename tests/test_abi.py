"""CPU: the C-ABI library builds, loads, and exports exactly the symbols include/cambrian_amd.h declares;
host-side guards (no CPU fallback) hold.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cmb_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_every_declared_symbol_is_exported_and_bound(built):
    syms = _header_symbols()
    assert len(syms) >= 25
    lib = built.load()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in cambrian_amd.h but not exported"
        assert s in built.SIGNATURES, f"{s} has no ctypes signature in cambrian_amd/lib.py"
    extra = set(built.SIGNATURES) - set(syms)
    assert not extra, f"bound but undeclared symbols: {extra}"
    assert lib.cmb_version().decode().endswith("gfx950")


def test_library_contains_gfx950_code_object(built):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", built.LIB_PATH],
                         capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_no_cpu_fallback(built):
    from cambrian_amd import ops
    with pytest.raises(built.CambrianAmdError):
        ops.k_gemm(torch.zeros(4, 64), torch.zeros(8, 64))
    from cambrian_amd.model.vision_sampler import VisionTokenSampler
    m = VisionTokenSampler(1024, 1024, [1024], [1], 1024, 1)
    q = torch.zeros(2, 1, 1024)
    with pytest.raises(built.CambrianAmdError):
        m(q, q, q, torch.ones(2, 1, dtype=torch.bool))


def test_missing_library_fails_loudly(built, monkeypatch):
    monkeypatch.setattr(built, "_lib", None)
    monkeypatch.setattr(built, "LIB_PATH", "/nonexistent/libcambrian_amd.so")
    with pytest.raises(built.CambrianAmdError, match="no PyTorch fallback"):
        built.load()


def test_state_dict_keys_match_reference_contract():
    """SURVEY.md §8b key list (vision_sampler.py:170-175,254-267)."""
    from cambrian_amd.model.vision_sampler import VisionTokenSampler
    m = VisionTokenSampler(4096, 1024, [1024] * 4, [1, 1, 1, 4], 1024, 1)
    keys = set(m.state_dict().keys())
    want = {"layers.0.proj_context.weight", "layers.0.proj_in.weight", "layers.0.proj_out.linear_1.weight",
            "layers.0.proj_out.linear_2.weight", "layers.0.norm.weight", "layers.0.norm.bias",
            "layers.0.cross_attn.q_proj.0.weight", "layers.0.cross_attn.q_proj.0.bias",
            "layers.0.cross_attn.q_proj.1.weight", "layers.0.cross_attn.o_proj.weight", "layers.0.pos_embed_3"}
    for i in range(4):
        for kv in "kv":
            want |= {f"layers.0.cross_attn.{kv}_proj_{i}.0.weight", f"layers.0.cross_attn.{kv}_proj_{i}.0.bias",
                     f"layers.0.cross_attn.{kv}_proj_{i}.1.weight"}
    assert keys == want
    sd = m.state_dict()
    assert sd["layers.0.proj_in.weight"].shape == (1024, 4096 + 1024)
    assert sd["layers.0.proj_out.linear_2.weight"].shape == (4096, 1024)
    assert sd["layers.0.pos_embed_3"].shape == (16, 1024)


def test_abi_revision_is_checked(built, monkeypatch):
    """a library of another ABI revision resolves every symbol and then receives shifted argument lists; the
    binding compares cmb_abi_version() with the header revision it was written against."""
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    rev = int(re.search(r"#define\s+CMB_ABI_VERSION\s+(\d+)", text).group(1))
    assert built.ABI_VERSION == rev == built.load().cmb_abi_version()
    monkeypatch.setattr(built, "_lib", None)
    monkeypatch.setattr(built, "ABI_VERSION", rev + 1)
    with pytest.raises(built.CambrianAmdError, match="ABI revision"):
        built.load()


def test_only_the_c_abi_leaves_the_library(built):
    """`nm -D`: every defined dynamic symbol is a ``cmb_*`` entry point of the header — no mangled C++ launcher, no per-TU
    marker (csrc/exports.map)."""
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert names, "no dynamic symbols?"
    foreign = [n for n in names if not n.startswith("cmb_")]
    assert not foreign, f"symbols outside the C-ABI are exported: {foreign[:5]}"
    assert sorted(set(names)) == _header_symbols()


def test_knob_values_are_validated(built):
    """cmb_knob_set rejects values outside each knob's closed set: a typo in an A/B run must not launch a bogus
    grid or silently select another variant."""
    lib = built.load()
    ok, bad = 0, -1
    saved = [lib.cmb_knob_get(k) for k in range(8)]
    try:
        assert lib.cmb_knob_set(built.KNOB_DWCONV, -3) == bad
        assert lib.cmb_knob_set(built.KNOB_LN_FWD, -1) == bad
        assert lib.cmb_knob_set(built.KNOB_VIT_ATTN, 4) == bad
        assert lib.cmb_knob_set(built.KNOB_SVA_ABS, 7) == bad
        assert lib.cmb_knob_set(built.KNOB_LN_MULTI_CHUNK, 3) == bad and lib.cmb_knob_set(built.KNOB_LN_MULTI_CHUNK, 8) == bad
        assert lib.cmb_knob_set(99, 0) == bad
        assert lib.cmb_knob_set(built.KNOB_COLSUM_WGS, -1) == bad
        assert lib.cmb_knob_set(built.KNOB_LN_BWD_ROWS, 0) == bad and lib.cmb_knob_set(built.KNOB_LN_BWD_ROWS, 257) == bad
        assert [lib.cmb_knob_get(k) for k in range(8)] == saved          # a rejected value changes nothing
        assert lib.cmb_knob_set(built.KNOB_COLSUM_WGS, 0) == ok and lib.cmb_knob_set(built.KNOB_LN_BWD_ROWS, 64) == ok
        assert lib.cmb_knob_set(built.KNOB_LN_MULTI_CHUNK, 7) == ok and lib.cmb_knob_get(built.KNOB_LN_MULTI_CHUNK) == 7
        assert lib.cmb_knob_set(built.KNOB_DWCONV, 32) == ok
    finally:
        for k, v in enumerate(saved):
            assert lib.cmb_knob_set(k, v) == ok


def test_flash_attn_arguments_are_checked_before_any_launch(built):
    """cmb_flash_attn_fwd / _bwd share one host-side argument check (flash_common.h): the status per kind of mistake and the
    order of the checks.  Every case returns before anything is launched; the pointers are never dereferenced."""
    import ctypes as C
    lib = built.load()
    ok, bad_arg, alignment, shape = 0, -1, -2, -3
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def fwd(q=p, k=p, v=p, B=2, S=256, H=4, HKV=2, hd=128, q_ss=512, kv_sh=128, causal=1, kv_len=256, out=p, lse=p):
        return lib.cmb_flash_attn_fwd(q, k, v, B, S, H, HKV, hd, S * H * 128, q_ss, 128, S * HKV * 128, HKV * 128, kv_sh, 0.088,
                                      causal, kv_len, None, out, lse, None)

    def bwd(q=p, k=p, v=p, o=p, dout=p, lse=p, B=2, S=256, H=4, HKV=2, hd=128, q_ss=512, kv_sh=128, causal=1, kv_len=256,
            dvec=p, dq=p, dk=p, dv=p):
        return lib.cmb_flash_attn_bwd(q, k, v, o, dout, lse, B, S, H, HKV, hd, S * H * 128, q_ss, 128, S * HKV * 128, HKV * 128,
                                      kv_sh, 0.088, causal, kv_len, None, dvec, dq, dk, dv, None)

    for f, ptrs in ((fwd, ("q", "k", "v", "out", "lse")), (bwd, ("q", "k", "v", "o", "dout", "lse", "dvec", "dq", "dk", "dv"))):
        for name in ptrs:
            assert f(**{name: None}) == bad_arg, f"{f.__name__}: NULL {name}"
            assert f(**{name: None}, hd=64, B=0) == bad_arg             # the null test comes first
        assert f(hd=64) == shape
        assert f(S=100) == shape and f(S=0) == shape
        assert f(H=3, HKV=2) == shape
        assert f(H=0) == shape and f(HKV=0) == shape and f(B=-1) == shape
        assert f(causal=0, kv_len=0) == shape and f(causal=0, kv_len=257) == shape
        assert f(q_ss=4) == alignment and f(kv_sh=4) == alignment and f(q_ss=516) == alignment
        assert f(B=0) == ok
        assert f(B=0, causal=1, kv_len=0) == ok                          # kv_len matters only to the bidirectional kernels
        assert f(B=0, q_ss=4) == ok                                      # an empty batch returns before the stride test ...
        assert f(B=0, hd=64) == shape and f(B=0, causal=0, kv_len=0) == shape   # ... and after the shape tests


def test_streaming_entry_points_check_arguments_before_any_launch(built):
    """The norm / RMSNorm / RoPE / cross-entropy / SwiGLU / QKV-RoPE / depthwise-conv entry points dispatch dtype, row width and
    their bool variants through the macros of csrc/launch.h: the status per kind of mistake and the order of the checks.  Every
    case returns before anything is launched; the pointers are never dereferenced."""
    import ctypes as C
    lib = built.load()
    ok, bad_arg, shape = 0, -1, -3
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def entry(name, **args):          # args: the C argument list in order, without the trailing stream
        def call(**over):
            assert not set(over) - set(args), over
            return getattr(lib, name)(*[over.get(k, v) for k, v in args.items()], None)
        call.__name__ = name
        return call

    ln_fwd = entry("cmb_layernorm_fwd", dtype=0, x=p, rows=4, D=1024, ldx=1024, add=None, side=0, grid_r=0, gamma=None, beta=None,
                   eps=1e-5, y=p, ldy=1024, mean=p, rstd=p)
    ln_bwd = entry("cmb_layernorm_bwd", dtype=0, dy=p, lddy=1024, x=p, ldx=1024, rows=4, D=1024, add=None, side=0, grid_r=0,
                   gamma=None, mean=p, rstd=p, dx=p, lddx=1024, dx_accumulate=0, dgamma=None, dbeta=None, dadd=None,
                   workspace=None, workspace_floats=0)
    stats = entry("cmb_row_stats", dtype=0, x=p, rows=4, D=1024, ldx=1024, eps=1e-5, mean=p, rstd=p)
    rms_fwd = entry("cmb_rmsnorm_fwd", dtype=0, x=p, rows=4, D=1024, w=p, eps=1e-5, y=p, rstd=p)
    rms_bwd = entry("cmb_rmsnorm_bwd", dtype=0, dy=p, x=p, rows=4, D=1024, w=p, rstd=p, dx=p, dw=None)
    add_rms = entry("cmb_add_rmsnorm_fwd", dtype=0, x=p, res=p, rows=4, D=1024, w=p, eps=1e-5, sum=p, y=p, rstd=p)
    rms_bwd_add = entry("cmb_rmsnorm_bwd_add", dtype=0, dy=p, x=p, dadd=None, rows=4, D=1024, w=p, rstd=p, dx=p)
    rope_table = entry("cmb_rope_table", pos=p, rows=4, D=128, base=1e4, cos=p, sin=p)
    rope = entry("cmb_rope_apply", dtype=0, x=p, cos=p, sin=p, rows=4, H=2, D=128, row_stride=256, inverse=0)
    ce_fwd = entry("cmb_cross_entropy_fwd", dtype=0, logits=p, rows=4, D=1024, ld=1024, labels=p, ignore_index=-100, lse=p, loss=p)
    ce_bwd = entry("cmb_cross_entropy_bwd", dtype=0, logits=p, rows=4, D=1024, ld=1024, labels=p, ignore_index=-100, lse=p,
                   scale=p, dlogits=p, ldd=1024)
    swiglu = entry("cmb_swiglu_bwd", dtype=0, dh=p, lddh=1024, g=p, ldg=1024, u=p, ldu=1024, rows=4, D=1024, dg=p, lddg=1024,
                   du=p, lddu=1024)
    qkv = entry("cmb_qkv_rope", dtype=0, merge=0, packed=p, cos=p, sin=p, rows=1, S=4, nh=2, nkv=1, D=128, q=p, k=p, v=p)
    dwconv = entry("cmb_dwconv7x7_nhwc", dtype=0, x=p, rows=2, H=8, W=8, D=64, w=p, bias=p, y=p)
    wgrad = entry("cmb_dwconv7x7_wgrad", dtype=0, x=p, dy=p, rows=2, H=8, W=8, D=64, partial=p, slots=4)

    # entry point -> its required pointers; `rows` is the count that may be zero, `D` the width
    required = {ln_fwd: ("x", "y"), ln_bwd: ("dy", "x", "dx", "mean", "rstd"), stats: ("x", "mean", "rstd"),
                rms_fwd: ("x", "y", "w"), rms_bwd: ("dy", "x", "w", "rstd", "dx"),
                add_rms: ("x", "res", "w", "sum", "y", "rstd"), rms_bwd_add: ("dy", "x", "w", "rstd", "dx"),
                rope_table: ("pos", "cos", "sin"), rope: ("x", "cos", "sin"),
                ce_fwd: ("logits", "labels", "lse", "loss"), ce_bwd: ("logits", "labels", "lse", "scale", "dlogits"),
                swiglu: ("dh", "g", "u", "dg", "du"), qkv: ("packed", "cos", "sin", "q", "k", "v"),
                dwconv: ("x", "w", "bias", "y"), wgrad: ("x", "dy", "partial")}
    for f, ptrs in required.items():
        for name in ptrs:
            assert f(**{name: None}) == bad_arg, f"{f.__name__}: NULL {name}"
            assert f(**{name: None}, rows=0) == bad_arg, f"{f.__name__}: NULL {name}, no rows"   # the null test comes first
        assert f(rows=0) == ok, f.__name__
        assert f(rows=-1) == bad_arg, f.__name__
        if f is not rope_table:
            assert f(dtype=7) == bad_arg and f(dtype=-1) == bad_arg, f.__name__

    # a width that is no whole number of 16-byte vectors (RoPE: of vector pairs); the cross-entropy takes any vocabulary
    for f in (ln_fwd, ln_bwd, stats, rms_fwd, rms_bwd, add_rms, rms_bwd_add, swiglu, dwconv):
        assert f(D=1020) == bad_arg and f(D=0) == bad_arg and f(D=1020, rows=0) == bad_arg, f.__name__
    for f in (rope, qkv):
        assert f(D=120) == bad_arg and f(D=0) == bad_arg, f.__name__
    assert rope_table(D=127) == bad_arg and ce_fwd(D=0) == bad_arg and ce_bwd(D=0) == bad_arg
    assert wgrad(D=72) == shape and wgrad(D=72, rows=0) == shape          # 64-channel slices; tested before the empty batch

    # rows wider than the widest instantiation: 16 vec8 chunks per lane = 8192 elements, 8 = 4096 for the LayerNorm backward
    for f in (ln_fwd, rms_fwd, rms_bwd, add_rms, rms_bwd_add):
        assert f(D=8192 + 8) == shape, f.__name__
        assert f(D=8192 + 8, rows=0) == ok, f.__name__                      # an empty input returns before the width test
    assert ln_fwd(D=8192 + 8, gamma=p, beta=p) == shape                     # (the LDS variant of the affine LayerNorms)
    assert ln_bwd(D=4096 + 8) == shape and ln_bwd(D=4096 + 8, dx_accumulate=1, dtype=1) == shape
    assert stats(D=4096 + 8) == bad_arg
    # an unknown dtype and an unsupported width together: the fused RMSNorm pair tests the width first, the others the dtype
    assert add_rms(D=8192 + 8, dtype=7) == shape and rms_bwd_add(D=8192 + 8, dtype=7) == shape
    assert rms_fwd(D=8192 + 8, dtype=7) == bad_arg and rms_bwd(D=8192 + 8, dtype=7) == bad_arg
    assert ln_fwd(D=8192 + 8, dtype=7) == bad_arg and ln_bwd(D=4096 + 8, dtype=7) == bad_arg
    # where the dtype is tested relative to the empty input
    for f in (ce_fwd, ce_bwd):
        assert f(dtype=7, rows=0) == bad_arg, f.__name__
    for f in (ln_fwd, ln_bwd, stats, rms_fwd, rms_bwd, add_rms, rms_bwd_add, rope, swiglu, qkv, dwconv, wgrad):
        assert f(dtype=7, rows=0) == ok, f.__name__
    # the other argument rules of these entry points
    assert ln_fwd(gamma=p) == bad_arg and ln_fwd(beta=p) == bad_arg         # affine parameters come as a pair
    assert ln_fwd(add=p, side=4, grid_r=3) == bad_arg and ln_bwd(add=p, side=0, grid_r=1) == bad_arg
    assert ln_bwd(add=p, side=4, grid_r=2, rows=24) == shape               # whole images only
    assert ln_bwd(gamma=p, dgamma=p) == -4 and ln_bwd(add=p, side=2, grid_r=2, dadd=p) == -4   # CMB_ERR_WORKSPACE

    # the multi-layer LayerNorm pair: descriptors; one instantiation (rows of up to 1024 elements)
    def multi(fn, desc_t, fields, **over):
        d = desc_t()
        for k, v in {**fields, **over}.items():
            if isinstance(v, list):
                for i, e in enumerate(v):
                    getattr(d, k)[i] = e
            else:
                setattr(d, k, v)
        return fn(C.byref(d), None)

    fwd_fields = dict(dtype=0, layers=2, x=p, ldx=1024, rows=4, D=1024, side=0, grid_r=0, eps=1e-5, y=[p, p], mean=[p, p],
                      rstd=[p, p])
    bwd_fields = dict(dtype=0, layers=2, x=p, ldx=1024, rows=4, D=1024, side=0, grid_r=0, dy=[p, p], mean=[p, p], rstd=[p, p],
                      dx=p, lddx=1024)
    for fn, desc_t, fields, wide in ((lib.cmb_layernorm_fwd_multi, built.LnFwdMultiDesc, fwd_fields, bad_arg),
                                     (lib.cmb_layernorm_bwd_multi, built.LnMultiDesc, bwd_fields, shape)):
        assert fn(None, None) == bad_arg
        assert multi(fn, desc_t, fields, x=None) == bad_arg and multi(fn, desc_t, fields, mean=[p, None]) == bad_arg
        assert multi(fn, desc_t, fields, dtype=7) == bad_arg and multi(fn, desc_t, fields, dtype=7, rows=0) == bad_arg
        assert multi(fn, desc_t, fields, D=1020) == bad_arg
        assert multi(fn, desc_t, fields, layers=0) == bad_arg and multi(fn, desc_t, fields, layers=built.LN_MULTI_MAX + 1) == bad_arg
        assert multi(fn, desc_t, fields, D=1032) == wide
        assert multi(fn, desc_t, fields, rows=0) == ok and multi(fn, desc_t, fields, rows=0, D=1032) == (bad_arg if wide == bad_arg else ok)
