"""CPU: host side of the fused decode attention (``cmb_decode_attn``, decode_attn.hip) — the split plan, the argument
checks that run before anything is launched, and the absence of a CPU path.  No kernel is launched here."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_plan_is_deterministic_monotone_and_covers_the_keys(built):
    from cambrian_amd import ops
    mx = ops.decode_attention_max_splits()
    assert mx >= 8
    for B in (1, 16):
        for nkv in (1, 8):
            prev = 1
            for t in list(range(0, 600)) + list(range(600, 8193, 37)) + [8190, 8191, 8192]:
                s, ch = ops.decode_attention_plan(B, nkv, t)
                assert (s, ch) == ops.decode_attention_plan(B, nkv, t)
                assert 1 <= s <= mx
                assert s * ch >= t + 1 > (s - 1) * ch
                assert s >= prev, f"B={B} nkv={nkv} t={t}: {s} splits after {prev}"      # more keys never mean fewer chunks
                prev = s
            assert ops.decode_attention_plan(B, nkv, 8192)[0] > 1                          # a long cache is split ...
            assert ops.decode_attention_plan(B, nkv, 15)[0] == 1                           # ... a short one is not
    # more (batch row, KV head) pairs need fewer chunks each to fill the chip
    assert ops.decode_attention_plan(16, 8, 8192)[0] <= ops.decode_attention_plan(1, 8, 8192)[0]


def test_forced_splits_are_honoured_or_reduced(built):
    from cambrian_amd import ops
    mx = ops.decode_attention_max_splits()
    for t in (0, 1, 4, 129, 1030):
        for want in range(1, mx + 1):
            s, ch = ops.decode_attention_plan(2, 2, t, want)
            assert 1 <= s <= want and s * ch >= t + 1 > (s - 1) * ch
    assert ops.decode_attention_plan(2, 2, 1030, 3) == (3, 344)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_attention_plan(2, 2, 1030, mx + 1)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_attention_plan(2, 2, -1)


def test_workspace_query(built):
    lib = built.load()
    assert lib.cmb_decode_attn_ws(2, 8, 2, 128, 1030, 1) == 0
    assert lib.cmb_decode_attn_ws(2, 8, 2, 128, 1030, 3) == 2 * 8 * 3 * 130
    assert lib.cmb_decode_attn_ws(2, 8, 2, 32, 1030, 3) == -1          # head_dim outside the set
    assert lib.cmb_decode_attn_ws(2, 9, 1, 128, 1030, 3) == -1         # 9 query heads per KV head


def test_bad_arguments_are_rejected_before_any_launch(built):
    """Every case returns CMB_ERR_BAD_ARG from the host-side checks; the pointers are never dereferenced (this box may
    have no device at all)."""
    lib = built.load()
    bad = -1
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def call(dtype=built.F32, q=p, k=p, v=p, cos=p, sin=p, kc=p, vc=p, nh=8, nkv=2, hd=128, t=1030, kvalid=p, kv_ld=2048,
             splits=2, ws=p, ws_floats=1 << 30, out=p):
        return lib.cmb_decode_attn(dtype, q, 2048, k, 2048, v, 2048, cos, sin, kc, vc, 1 << 20, 1 << 18, 128, 2, nh, nkv, hd, t,
                                   kvalid, kv_ld, 0.088, splits, ws, ws_floats, out, None)

    for name in ("q", "k", "v", "cos", "sin", "kc", "vc", "kvalid", "out"):
        assert call(**{name: None}) == bad, f"NULL {name}"
    assert call(ws=None) == bad                                         # split run without a workspace
    assert call(dtype=2) == bad and call(dtype=built.FP8_E4M3) == bad and call(dtype=-1) == bad
    for hd in (0, 32, 80, 256):
        assert call(hd=hd) == bad
    assert call(nh=9, nkv=1) == bad                                     # G = 9
    assert call(nh=16, nkv=1) == bad
    assert call(nh=7, nkv=2) == bad                                     # nh % nkv != 0
    assert call(nh=0) == bad and call(nkv=0) == bad
    assert call(t=-1) == bad
    assert call(kv_ld=1030) == bad                                      # the mask row is shorter than t + 1
    need = lib.cmb_decode_attn_ws(2, 8, 2, 128, 1030, 2)
    assert need > 0 and call(ws_floats=need - 1) == bad
    assert call(splits=-1) == bad and call(splits=10 ** 6) == bad


def test_no_cpu_fallback(built):
    from cambrian_amd import ops
    B, nh, nkv, hd, n = 1, 4, 2, 64, 8
    q, k, v = torch.zeros(B, nh * hd), torch.zeros(B, nkv * hd), torch.zeros(B, nkv * hd)
    cs = torch.zeros(B, hd // 2)
    kc, vc = torch.zeros(B, nkv, n, hd), torch.zeros(B, nkv, n, hd)
    with pytest.raises(built.CambrianAmdError):
        ops.decode_attention(q, k, v, cs, cs, kc, vc, 3, torch.ones(B, n, dtype=torch.bool))


def test_supported_geometries(built):
    from cambrian_amd import ops
    for nh, nkv, hd in ((32, 8, 128), (56, 8, 128), (40, 40, 128), (32, 32, 96), (4, 2, 64)):   # Llama-3-8B, Yi-34B, Vicuna-13B, Phi-3
        assert ops.decode_attention_supported(torch.bfloat16, nh, nkv, hd)
        assert ops.decode_attention_supported(torch.float32, nh, nkv, hd)
    assert not ops.decode_attention_supported(torch.float16, 32, 8, 128)
    assert not ops.decode_attention_supported(torch.bfloat16, 32, 8, 32)
    assert not ops.decode_attention_supported(torch.bfloat16, 64, 4, 128)
    assert not ops.decode_attention_supported(torch.bfloat16, 7, 2, 128)
