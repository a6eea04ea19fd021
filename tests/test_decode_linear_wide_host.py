"""CPU: host side of the wide decode-step linear (``cmb_decode_linear_wide``, decode_linear_wide.hip) — the switch, the shape
predicate and the plan through the library, the symbols, and which function the decoder layers hand a decode step of 16 / 32
rows to, with the ops replaced by recorders.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_decode_linear_wide", "cmb_decode_linear_wide_supported", "cmb_decode_linear_wide_plan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


@pytest.fixture()
def env(monkeypatch):
    for name in ("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_FP8",
                 "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_ATTN"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_switch_env_over_config_default_off(built, env):
    from cambrian_amd import ops
    assert ops.DECODE_LINEAR_WIDE_MAX_ROWS == 64 and ops.DECODE_LINEAR_MAX_ROWS == 16
    assert ops.decode_linear_wide_enabled() is False                      # unset, no config flag: off
    assert ops.decode_linear_wide_enabled(True) is True and ops.decode_linear_wide_enabled(False) is False
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "1")
    assert ops.decode_linear_wide_enabled(False) is True
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "0")
    assert ops.decode_linear_wide_enabled(True) is False
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "")
    assert ops.decode_linear_wide_enabled(True) is True
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "yes")
    with pytest.raises(ValueError, match="CAMBRIAN_AMD_DECODE_LINEAR_WIDE"):
        ops.decode_linear_wide_enabled()
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "1")
    assert [ops.decode_linear_wide_rows(r) for r in (1, 16, 17, 64, 65)] == [False, False, True, True, False]
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "0")                          # the stock sequence everywhere wins
    assert not ops.decode_linear_wide_rows(32)
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "1")
    assert ops.decode_linear_wide_rows(32)


def test_symbols_are_declared_exported_and_bound_under_revision_13(built):
    import fnmatch
    import subprocess
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    lib = built.load()
    vs = open(os.path.join(ROOT, "cambrian_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:(.*?)local:", re.sub(r"/\*.*?\*/", "", vs, flags=re.S), flags=re.S).group(1)
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert any(fnmatch.fnmatchcase(name, g.strip()) for g in globs.split(";") if g.strip())
        assert name in exported
        assert name in built.SIGNATURES
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]
    assert built.SIGNATURES["cmb_decode_linear_wide"] == built.SIGNATURES["cmb_decode_linear"]       # the narrow contract
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    assert "cmb_decode_linear_wide" in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert "decode_linear_wide.hip" in open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()


def test_supported_and_plan_through_the_library(built):
    from cambrian_amd import ops
    lib = built.load()
    for M in (-1, 0, 1, 16, 17, 63, 64, 65, 128):
        for N in (0, 1, 2, 3, 30, 4096, 128256):
            for K in (0, 4, 8, 12, 64, 72, 4096, 14336):
                for act in (-1, 0, 1, 2):
                    want = 1 <= M <= 64 and N >= 1 and K >= 8 and K % 8 == 0 and act in (0, 1) and not (act == 1 and N % 2)
                    assert lib.cmb_decode_linear_wide_supported(M, N, K, act) == int(want), (M, N, K, act)
    assert lib.cmb_decode_linear_wide_supported(64, 4096, 4096, 0) == 1
    assert lib.cmb_decode_linear_wide_supported(0, 4096, 4096, 0) == 0 == lib.cmb_decode_linear_wide_supported(65, 4096, 4096, 0)
    assert lib.cmb_decode_linear_wide_supported(32, 31, 64, 1) == 0                 # odd N with SwiGLU
    assert lib.cmb_decode_linear_wide_supported(32, 32, 60, 0) == 0                 # K % 8
    assert lib.cmb_decode_linear_wide_supported(1, (1 << 31) + 2, 8, 0) == 0
    for M in (0, 65):
        with pytest.raises(built.CambrianAmdError):
            ops.decode_linear_wide_plan(M, 4096, 4096)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_wide_plan(32, 31, 64, "swiglu")
    with pytest.raises(built.CambrianAmdError):
        ops.decode_linear_wide_plan(32, 32, 60)
    for cus in (256, 304, 64):
        for act in (None, "swiglu"):
            for N in [2, 4, 30, 62, 64, 66, 1024, 4096, 6144, 8192, 9216, 16384, 28672, 128256]:
                plans = {ops.decode_linear_wide_plan(M, N, K, act, cus) for M in (1, 17, 64) for K in (4096, 14336)}
                assert len(plans) == 1                                 # a pure function of (N, act, CU count)
                rows, wgs = plans.pop()
                assert (rows, wgs) == ops.decode_linear_wide_plan(64, N, 4096, act, cus)
                assert rows in (16, 32)
                per = rows // 2 if act else rows                       # output columns a workgroup owns
                cols = N // 2 if act else N
                assert (wgs - 1) * per < cols <= wgs * per             # covers N' exactly
                if rows == 16:                                         # the larger slab was refused only to keep a workgroup per CU
                    assert -(-cols // (2 * per)) < cus
                else:
                    assert wgs >= cus
    assert ops.decode_linear_wide_plan(64, 4096, 14336, None, 256) == (16, 256)        # o_proj / down_proj on an MI355X
    assert ops.decode_linear_wide_plan(64, 28672, 4096, "swiglu", 256) == (32, 896)
    assert ops.decode_linear_wide_plan(64, 128256, 4096, None, 256) == (32, 4008)
    assert ops.decode_linear_wide_plan(64, 4096, 4096)[0] in (16, 32)                  # cus = 0: this machine's device, or 256


def test_bad_arguments_are_rejected_before_any_launch(built):
    lib = built.load()
    bad = -1
    raw = (C.c_char * 272)()
    p = (C.addressof(raw) + 15) & ~15

    def call(x=p, x_ld=64, M=33, norm=p, eps=1e-5, W=p, w_ld=64, N=32, K=64, act=0, res=p, r_ld=32, out=p, o_ld=32, f32=0):
        return lib.cmb_decode_linear_wide(x, x_ld, M, norm, eps, W, w_ld, N, K, act, res, r_ld, out, o_ld, f32, None)

    for name in ("x", "W", "out"):
        assert call(**{name: None}) == bad, f"NULL {name}"
    assert call(M=0) == bad and call(M=65) == bad and call(M=-1) == bad
    assert call(K=60) == bad and call(K=0) == bad and call(N=0) == bad
    assert call(x_ld=56) == bad and call(w_ld=56) == bad and call(o_ld=24) == bad and call(r_ld=24) == bad
    assert call(x_ld=68) == bad and call(w_ld=68) == bad and call(o_ld=36) == bad and call(r_ld=36) == bad
    for name in ("x", "W", "out", "norm", "res"):
        assert call(**{name: p + 2}) == bad and call(**{name: p + 8}) == bad, f"misaligned {name}"
    assert call(act=1, res=None, N=31) == bad and call(act=1, N=32) == bad and call(act=2, res=None) == bad
    assert call(f32=2) == bad and call(eps=-1.0) == bad and call(eps=float("nan")) == bad
    del raw


def test_no_cpu_path_and_no_backward(built):
    from cambrian_amd import ops
    x, w = torch.zeros(40, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16)
    assert not ops.decode_linear_wide_supported(x, w, None)
    with pytest.raises(built.CambrianAmdError, match="CPU"):
        ops.decode_linear_wide(x, w)
    with pytest.raises(built.CambrianAmdError, match="no backward"):
        ops.decode_linear_wide(x, w.clone().requires_grad_())


# ---- dispatch: which linear a decode step is handed to ----
class _Rec:
    """Stand-ins for the ops a five-launch step calls: they count, check the row limit of the function they replace and
    return zeros of the right shape."""

    def __init__(self, monkeypatch):
        from cambrian_amd import ops
        from cambrian_amd.model.language_model import cambrian_llama as CL, cambrian_phi3 as CP
        self.n = {"narrow": 0, "wide": 0, "attn": 0, "quant": 0}
        rec = self

        def shape_ok(limit):
            def supported(x, w, act=None):
                return x.dim() == 2 and w.dim() == 2 and 1 <= x.shape[0] <= limit and x.shape[1] == w.shape[1]

            def weight_supported(M, w, act=None):
                return w.dim() == 2 and 1 <= M <= limit
            return supported, weight_supported

        def linear(key, limit):
            def fn(x, w, *, norm_weight=None, eps=0.0, act=None, residual=None, out_dtype=None, out=None):
                assert 1 <= x.shape[0] <= limit, f"{key} linear handed {x.shape[0]} rows"
                rec.n[key] += 1
                cols = w.shape[0] // 2 if act else w.shape[0]
                return torch.zeros(x.shape[0], cols, dtype=out_dtype or torch.bfloat16)
            return fn

        def attn(q, k, v, *a, **kw):
            rec.n["attn"] += 1
            return torch.zeros(q.shape[0], q.shape[1], dtype=q.dtype)

        def quant(w, *a, **kw):
            rec.n["quant"] += 1
            return (torch.zeros(w.shape, dtype=torch.uint8), torch.ones(w.shape[0]))

        for name, limit in (("decode_linear", 16), ("decode_linear_wide", 64)):
            sup, wsup = shape_ok(limit)
            monkeypatch.setattr(ops, name + "_supported", sup)
            monkeypatch.setattr(ops, name + "_weight_supported", wsup)
            monkeypatch.setattr(ops, name, linear("narrow" if limit == 16 else "wide", limit))
        monkeypatch.setattr(ops, "decode_linear_fp8_weight_supported", lambda M, w, act=None: M <= 16)
        monkeypatch.setattr(ops, "decode_fp8_weight", quant)
        narrow = linear("narrow", 16)
        monkeypatch.setattr(ops, "decode_linear_fp8", lambda x, q, inv_scale, **kw: narrow(x, q, **kw))
        monkeypatch.setattr(ops, "decode_attention_any", attn)
        for mod in (CL, CP):
            monkeypatch.setattr(mod, "use_decode_kernel", lambda x, nh, nkv, hd: True)


def _layer(lm, **cfg_kw):
    from cambrian_amd.model.language_model import cambrian_llama as CL, cambrian_phi3 as CP
    mod = CP if lm == "phi3" else CL
    cfg = mod.CambrianConfig(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                             num_key_value_heads=2, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=64, **cfg_kw)
    layer = (CP.Phi3DecoderLayer if lm == "phi3" else CL.LlamaDecoderLayer)(cfg, "cpu", torch.bfloat16)
    # the stock sequence is GPU kernels too: stand-ins on this instance, so that a step that takes it can run here
    layer.input_layernorm.forward = layer.post_attention_layernorm.forward = lambda x: x
    layer.self_attn.decode = lambda x, *a, **kw: torch.zeros_like(x)
    layer.mlp.forward = lambda h, residual=None: torch.zeros_like(h)
    return layer.requires_grad_(False), cfg


def _decode(layer, rows, **kw):
    x = torch.zeros(rows, 1, 64, dtype=torch.bfloat16)
    kc = torch.zeros(rows, 2, 8, 32, dtype=torch.bfloat16)
    cos = sin = torch.zeros(rows, 1, 32)
    mask = torch.ones(rows, 8, dtype=torch.bool)
    with torch.no_grad():
        return layer.decode(x, cos, sin, kc, kc.clone(), 4, mask, **kw)


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_dispatch_of_a_decode_step(built, env, lm):
    rec = _Rec(env)
    layer, cfg = _layer(lm)
    # switch off (the default): 32 rows are the stock sequence, not one wide call
    y = _decode(layer, 32)
    assert y.shape == (32, 1, 64) and rec.n == {"narrow": 0, "wide": 0, "attn": 0, "quant": 0}
    assert layer.decode_operands(torch.zeros(32, 1, 64, dtype=torch.bfloat16)) is None
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "0")
    cfg.decode_linear_wide = True                                          # the environment overrides the config
    _decode(layer, 32)
    assert rec.n["wide"] == 0 and rec.n["attn"] == 0
    # switch on through the config: five launches, four of them the wide linear
    env.delenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE")
    y = _decode(layer, 32)
    assert y.shape == (32, 1, 64) and rec.n == {"narrow": 0, "wide": 4, "attn": 1, "quant": 0}
    found = layer.decode_operands(torch.zeros(32, 1, 64, dtype=torch.bfloat16))
    assert found is not None and len(found[0]) == 4 and found[1] is None
    for rows in (17, 64):
        _decode(layer, rows)
    assert rec.n == {"narrow": 0, "wide": 12, "attn": 3, "quant": 0}
    # 16 rows still go to the narrow function, 65 to neither
    _decode(layer, 16)
    assert rec.n == {"narrow": 4, "wide": 12, "attn": 4, "quant": 0}
    _decode(layer, 65)
    assert rec.n == {"narrow": 4, "wide": 12, "attn": 4, "quant": 0}
    # the e4m3 switch at 32 rows: the bf16 wide kernel, no quantised copy; at 16 rows it quantises as before
    _decode(layer, 32, fp8=True)
    assert rec.n == {"narrow": 4, "wide": 16, "attn": 5, "quant": 0}
    assert layer.decode_operands(torch.zeros(32, 1, 64, dtype=torch.bfloat16), fp8=True)[1] is None and rec.n["quant"] == 0
    _decode(layer, 16, fp8=True)
    assert rec.n == {"narrow": 8, "wide": 16, "attn": 6, "quant": 4}
    # CAMBRIAN_AMD_DECODE_LINEAR=0 wins over the wide switch
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "0")
    env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "1")
    before = dict(rec.n)
    _decode(layer, 32)
    _decode(layer, 16)
    assert rec.n == before
    # the environment alone switches it on; a trainable projection keeps the stock sequence
    env.delenv("CAMBRIAN_AMD_DECODE_LINEAR")
    del cfg.decode_linear_wide
    _decode(layer, 32)
    assert rec.n["wide"] == before["wide"] + 4
    layer.mlp.down_proj.weight.requires_grad_(True)
    _decode(layer, 32)
    assert rec.n["wide"] == before["wide"] + 4


def test_logits_take_the_wide_function(built, env):
    from cambrian_amd.model.language_model import cambrian_llama as CL
    rec = _Rec(env)
    cfg = CL.CambrianConfig(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                            num_key_value_heads=2, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=64)
    model = CL.CambrianLlamaForCausalLM(cfg, device="cpu", llm_dtype=torch.bfloat16).requires_grad_(False)
    model.model.norm.forward = lambda x: x                                 # the stock line's norm is a GPU kernel
    x = torch.zeros(32, 1, 64, dtype=torch.bfloat16)
    with torch.no_grad():
        assert CL._decode_logits(model, x).shape == (32, 96) and rec.n["wide"] == 0
        assert CL._decode_logits_operands(model, x) is None
        cfg.decode_linear_wide = True
        out = CL._decode_logits(model, x, fp8=True)
        assert out.shape == (32, 96) and out.dtype == torch.float32
        assert rec.n == {"narrow": 0, "wide": 1, "attn": 0, "quant": 0}
        assert CL._decode_logits_operands(model, x, fp8=True) == (model.lm_head.weight, None) and rec.n["quant"] == 0
        CL._decode_logits(model, x[:16])
        assert rec.n == {"narrow": 1, "wide": 1, "attn": 0, "quant": 0}
    # the one-call step keeps refusing more than 16 rows
    assert CL.DecodeStepPlan.build(model, 32, [(None, None)], 64, False) is None
