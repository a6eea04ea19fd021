"""CPU: host side of the e4m3 K / V cache of the decode steps (``cmb_kv_quantize_e4m3``, ``cmb_decode_attn_kv8``,
decode_attn_kv8.hip; ``cmb_decode_step_kv8``, decode_step.hip) — symbols and bindings, the opt-in switch, and the argument
checks that run before anything is launched.  No kernel is launched here: every call below returns from the host-side checks,
and the pointers are addresses of host buffers that are never dereferenced."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_kv_quantize_e4m3", "cmb_decode_attn_kv8", "cmb_decode_step_kv8")
OK, BAD_ARG, ALIGNMENT, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def _aligned(nbytes=256):
    raw = (C.c_char * (nbytes + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


def test_symbols_are_declared_exported_and_bound(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    lib = built.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in built.SIGNATURES
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]       # resolves: the symbol left the library
        assert name in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    mk = open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()
    assert "decode_attn_kv8.hip" in mk
    body = re.search(r"typedef struct cmb_decode_kv8_factors \{(.*?)\} cmb_decode_kv8_factors;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in built.DecodeKv8Factors._fields_] == ["k_inv", "v_inv"]
    assert C.sizeof(built.DecodeKv8Factors) == 2 * C.sizeof(C.c_void_p)
    # the two layouts the new step entry shares with cmb_decode_step did not move
    assert C.sizeof(built.DecodeLayer) == 16 * 8 and C.sizeof(built.DecodeStepDesc) == 8 * 4 + 8 + 2 * 4 + 3 * 8 + 4 * 8


def test_switch_env_over_config(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_KV_FP8", raising=False)
    assert ops.decode_kv_fp8_enabled() is False and ops.decode_kv_fp8_enabled(False) is False
    assert ops.decode_kv_fp8_enabled(True) is True
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_KV_FP8", "")             # "" counts as unset
    assert ops.decode_kv_fp8_enabled(True) is True and ops.decode_kv_fp8_enabled(False) is False
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_KV_FP8", "0")
    assert ops.decode_kv_fp8_enabled(True) is False
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_KV_FP8", "1")
    assert ops.decode_kv_fp8_enabled(False) is True


def test_supported_geometries(built):
    from cambrian_amd import ops
    for nh, nkv, hd in ((32, 8, 128), (56, 8, 128), (32, 32, 96), (4, 2, 64)):
        assert ops.decode_attention_kv8_supported(torch.bfloat16, nh, nkv, hd)
        assert not ops.decode_attention_kv8_supported(torch.float32, nh, nkv, hd)      # bf16 activations only
    assert not ops.decode_attention_kv8_supported(torch.bfloat16, 32, 8, 80)
    assert not ops.decode_attention_kv8_supported(torch.bfloat16, 9, 1, 128)


def test_attn_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    keep, p = _aligned()

    def call(q=p, k=p, v=p, cos=p, sin=p, kc=p, vc=p, c_sb=1 << 20, c_sh=1 << 18, c_st=128, ki=p, vi=p, i_sb=1 << 13,
             i_sh=1 << 11, B=2, nh=8, nkv=2, hd=128, t=1030, kvalid=p, kv_ld=2048, splits=2, ws=p, ws_floats=1 << 30, out=p,
             q_ld=2048):
        return lib.cmb_decode_attn_kv8(q, q_ld, k, 2048, v, 2048, cos, sin, kc, vc, c_sb, c_sh, c_st, ki, vi, i_sb, i_sh, B, nh,
                                       nkv, hd, t, kvalid, kv_ld, 0.088, splits, ws, ws_floats, out, None)

    for name in ("q", "k", "v", "cos", "sin", "kc", "vc", "ki", "vi", "kvalid", "out"):
        assert call(**{name: None}) == BAD_ARG, f"NULL {name}"
    assert call(ws=None) == BAD_ARG                                     # split run without a workspace
    for hd in (0, 32, 80, 256):
        assert call(hd=hd, c_st=256) == BAD_ARG, hd
    assert call(nh=9, nkv=1) == BAD_ARG                                 # 9 query heads per KV head
    assert call(nh=7, nkv=2) == BAD_ARG
    assert call(c_st=112) == BAD_ARG                                    # c_st < hd
    assert call(c_st=64, hd=64, out=p + 8) == ALIGNMENT                 # ... and equal is fine: on to the alignment rules
    assert call(t=-1) == BAD_ARG
    assert call(kv_ld=1030) == BAD_ARG                                  # the mask row is shorter than t + 1
    need = lib.cmb_decode_attn_ws(2, 8, 2, 128, 1030, 2)
    assert need > 0 and call(ws_floats=need - 1) == BAD_ARG             # one float short
    assert call(splits=-1) == BAD_ARG and call(splits=10 ** 6) == BAD_ARG
    assert call(i_sb=-1) == BAD_ARG
    # byte strides are multiples of 16; pointers are aligned
    assert call(c_st=136) == ALIGNMENT and call(c_sh=(1 << 18) + 8) == ALIGNMENT and call(c_sb=(1 << 20) + 4) == ALIGNMENT
    for name in ("q", "k", "v", "kc", "vc", "out"):
        assert call(**{name: p + 8}) == ALIGNMENT, name
    assert call(ki=p + 2) == ALIGNMENT and call(vi=p + 1) == ALIGNMENT
    assert call(ki=p + 4, ws_floats=need - 1) == BAD_ARG                # a factor array needs 4 bytes only: on to the workspace rule
    assert call(q_ld=2052) == ALIGNMENT
    # B == 0 is a no-op
    assert call(B=0) == OK and call(B=0, ws=None, ws_floats=0) == OK
    del keep


def test_quantize_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    keep, p = _aligned()

    def call(src=p, s_sb=1 << 16, s_sh=1 << 13, s_st=128, B=2, nkv=2, L=37, hd=128, cache=p, c_sb=1 << 16, c_sh=1 << 13, c_st=128,
             inv=p, i_sb=128, i_sh=64):
        return lib.cmb_kv_quantize_e4m3(src, s_sb, s_sh, s_st, B, nkv, L, hd, cache, c_sb, c_sh, c_st, inv, i_sb, i_sh, None)

    for name in ("src", "cache", "inv"):
        assert call(**{name: None}) == BAD_ARG, f"NULL {name}"
    for hd in (0, 8, 72, 144):
        assert call(hd=hd) == BAD_ARG, hd
    assert call(c_st=112) == BAD_ARG and call(s_st=120) == BAD_ARG
    assert call(B=-1) == BAD_ARG and call(L=-1) == BAD_ARG and call(i_sh=-1) == BAD_ARG
    assert call(c_st=136) == ALIGNMENT and call(s_st=132) == ALIGNMENT
    assert call(src=p + 8) == ALIGNMENT and call(cache=p + 8) == ALIGNMENT and call(inv=p + 2) == ALIGNMENT
    assert call(B=0) == OK and call(L=0) == OK and call(L=0, src=None) == OK
    del keep


GEO = dict(B=3, H=256, I=512, nh=4, nkv=2, hd=64)


def _step_case(built, fp8=0, layers=2):
    keep, p = _aligned()
    table = (built.DecodeLayer * layers)()
    for row in table:
        for name, ld in (("qkv", 256), ("o", 256), ("gate_up", 256), ("down", 512)):
            setattr(row, "w_" + name, p)
            setattr(row, "ld_" + name, ld)
            setattr(row, "w_" + name + "_scale", p if fp8 else None)
        row.norm1 = row.norm2 = row.kcache = row.vcache = p
    factors = (built.DecodeKv8Factors * layers)(*[built.DecodeKv8Factors(p, p) for _ in range(layers)])
    desc = built.DecodeStepDesc(layers=layers, fp8=fp8, V=64, eps=1e-5, scale=0.125, c_sb=2 * 64 * 64, c_sh=64 * 64, c_st=64,
                                final_norm=p, head=p, ld_head=256, head_scale=p if fp8 else None, **GEO)
    return keep, p, desc, table, factors


def test_step_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    for fp8 in (0, 1, 2):
        keep, p, desc, table, factors = _step_case(built, fp8)
        t = 36
        need = lib.cmb_decode_step_ws(*GEO.values(), t)
        assert need > 0

        def call(d=desc, tab=table, fac=factors, i_sb=128, i_sh=64, x=p + (1 << 20), t=t, kv=p, kv_ld=64, ws=p,
                 ws_floats=need - 1, logits=p):
            return lib.cmb_decode_step_kv8(C.byref(d), tab, fac, i_sb, i_sh, x, 256, p, p, t, kv, kv_ld, ws, ws_floats, logits, 64,
                                           None)

        # the reference point: everything in order but the workspace, one float short — all three weight formats are accepted
        assert call() == WORKSPACE
        assert call(fac=None) == BAD_ARG                                 # a NULL factor array
        _, _, d3, _, _ = _step_case(built, fp8)
        d3.fp8 = 3
        assert call(d=d3) == BAD_ARG
        for field in ("k_inv", "v_inv"):
            _, _, _, _, fac = _step_case(built, fp8)
            setattr(fac[1], field, None)
            assert call(fac=fac) == BAD_ARG, field
            setattr(fac[1], field, p + 2)
            assert call(fac=fac) == ALIGNMENT, field
        assert call(i_sb=-1) == BAD_ARG and call(i_sh=-1) == BAD_ARG
        assert call(kv_ld=t) == BAD_ARG and call(t=-1) == BAD_ARG and call(x=None) == BAD_ARG
        for field, val, want in (("c_st", 48, BAD_ARG), ("c_st", 72, ALIGNMENT), ("c_sh", 64 * 64 + 8, ALIGNMENT), ("hd", 80, BAD_ARG)):
            _, _, d2, _, _ = _step_case(built, fp8)
            setattr(d2, field, val)
            assert call(d=d2) == want, (field, val)
        # cmb_decode_step itself behaves as before: its cache strides are elements, multiples of 8
        _, _, d2, _, _ = _step_case(built, fp8)
        d2.c_st = 72
        assert lib.cmb_decode_step(C.byref(d2), table, p + (1 << 20), 256, p, p, t, p, 64, p, need - 1, p, 64, None) == WORKSPACE
        del keep


def test_no_cpu_path(built):
    from cambrian_amd import ops
    B, nh, nkv, hd, n = 1, 4, 2, 64, 8
    q, k, v = (torch.zeros(B, x * hd, dtype=torch.bfloat16) for x in (nh, nkv, nkv))
    cs = torch.zeros(B, hd // 2)
    kc, vc = ops.KvCacheE4M3.empty(B, nkv, n, hd, "cpu"), ops.KvCacheE4M3.empty(B, nkv, n, hd, "cpu")
    with pytest.raises(built.CambrianAmdError):
        ops.decode_attention_kv8(q, k, v, cs, cs, kc, vc, 3, torch.ones(B, n, dtype=torch.bool))
    with pytest.raises(built.CambrianAmdError):
        ops.kv_quantize_e4m3(torch.zeros(B, nkv, 4, hd, dtype=torch.bfloat16), kc, 4)
    with pytest.raises(built.CambrianAmdError):
        ops.KvCacheE4M3(torch.zeros(1, 2, 8, 64), torch.zeros(1, 2, 8))             # bytes are uint8
