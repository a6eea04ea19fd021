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


OK, BAD_ARG, ALIGNMENT = 0, -1, -2
ENTRIES = ("cmb_decode_attn", "cmb_decode_attn_kv8", "cmb_decode_attn_multi")


def _entry_call(lib_mod, entry, p):
    """``call(**overrides)`` of one entry point on a call that is valid as it stands — bf16, B 2, 8 / 2 heads of 128, slot 1030
    (``multi``: Q 2 rows at slots 1030 and 1031), two forced chunks, a large workspace, every pointer ``p`` (16-byte
    aligned) — and the workspace need of that call.  The valid call itself is never made: it would launch."""
    lib = lib_mod.load()
    base = dict(q=p, q_ld=2048, k=p, k_ld=2048, v=p, v_ld=2048, cos=p, sin=p, kc=p, vc=p, c_sb=1 << 20, c_sh=1 << 18, c_st=128,
                ki=p, vi=p, i_sb=1 << 13, i_sh=1 << 11, B=2, nh=8, nkv=2, hd=128, Q=2, t=1030, kvalid=p, kv_ld=2048,
                splits=2, ws=p, ws_floats=1 << 30, out=p)

    def call(**kw):
        a = dict(base, **kw)
        head = [a[n] for n in ("q", "q_ld", "k", "k_ld", "v", "v_ld", "cos", "sin", "kc", "vc", "c_sb", "c_sh", "c_st")]
        geo = [a[n] for n in ("B", "nh", "nkv", "hd")]
        tail = [a["kvalid"], a["kv_ld"], 0.088, a["splits"], a["ws"], a["ws_floats"], a["out"], None]
        if entry == "cmb_decode_attn":
            return lib.cmb_decode_attn(lib_mod.BF16, *head, *geo, a["t"], *tail)
        if entry == "cmb_decode_attn_kv8":
            return lib.cmb_decode_attn_kv8(*head, a["ki"], a["vi"], a["i_sb"], a["i_sh"], *geo, a["t"], *tail)
        return lib.cmb_decode_attn_multi(*head, *geo, a["Q"], a["t"], *tail)

    if entry == "cmb_decode_attn_multi":
        need = lib.cmb_decode_attn_multi_ws(2, 8, 2, 128, 2, 1030, 2)
        assert need == 2 * 2 * 8 * 2 * 130
    else:
        need = lib.cmb_decode_attn_ws(2, 8, 2, 128, 1030, 2)
        assert need == 2 * 8 * 2 * 130
    return call, need


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_argument_table_of_the_three_entry_points(built, entry):
    """The status of every host-side check of ``cmb_decode_attn``, ``cmb_decode_attn_kv8`` and ``cmb_decode_attn_multi``, as the
    library returned them before the three launchers shared their checks: CMB_ERR_BAD_ARG wins over CMB_ERR_ALIGNMENT, which
    is returned only when everything else is in order, and B == 0 is a no-op.  No case reaches a launch and no pointer is
    dereferenced (this box may have no device at all)."""
    raw = (C.c_char * 272)()
    p = (C.addressof(raw) + 15) & ~15
    call, need = _entry_call(built, entry, p)
    kv8, multi = entry == "cmb_decode_attn_kv8", entry == "cmb_decode_attn_multi"
    rows = 2 if multi else 1
    misaligned = dict(out=p + 8)                                        # the one fault of the ALIGNMENT cases below

    for name in ("q", "k", "v", "cos", "sin", "kc", "vc", "kvalid", "out") + (("ki", "vi") if kv8 else ()):
        assert call(**{name: None}) == BAD_ARG, f"NULL {name}"
        assert call(**{name: None}, B=0) == BAD_ARG, f"NULL {name} at B == 0"
    for hd in (0, 32, 80, 256):
        assert call(hd=hd) == BAD_ARG, hd
    assert call(nh=9, nkv=1) == BAD_ARG                                 # G = 9
    assert call(nh=7, nkv=2) == BAD_ARG                                 # nh % nkv != 0
    assert call(nh=0) == BAD_ARG and call(nkv=0) == BAD_ARG
    assert call(t=-1) == BAD_ARG
    assert call(B=-1) == BAD_ARG and call(B=65536) == BAD_ARG and call(nh=65536, nkv=65536) == BAD_ARG
    assert call(kv_ld=1030) == BAD_ARG                                  # the mask row is shorter than the slots of the step
    assert call(kv_ld=1030 + rows - 1) == BAD_ARG
    assert call(kv_ld=1030 + rows, **misaligned) == ALIGNMENT           # ... and exactly as long is fine
    assert call(ws=None) == BAD_ARG and call(ws_floats=0) == BAD_ARG    # a split run without a workspace
    assert call(ws_floats=need - 1) == BAD_ARG                          # one float short
    assert call(ws_floats=need, **misaligned) == ALIGNMENT              # ... and the need itself is enough
    assert call(splits=1, ws=None, ws_floats=0, **misaligned) == ALIGNMENT      # an unsplit run needs none
    mx = C.c_int32(0)
    built.load().cmb_decode_attn_plan(1, 1, 0, 0, None, None, C.byref(mx))
    assert call(splits=mx.value, **misaligned) == ALIGNMENT
    assert call(splits=-1) == BAD_ARG and call(splits=mx.value + 1) == BAD_ARG and call(splits=10 ** 6) == BAD_ARG
    if multi:
        assert call(Q=0) == BAD_ARG and call(Q=17) == BAD_ARG and call(Q=-1) == BAD_ARG
        assert call(Q=16, **misaligned) == ALIGNMENT
        assert call(nh=10, nkv=2, Q=13) == BAD_ARG                      # Q * G = 65 rows
        assert call(nh=16, nkv=2, Q=8, **misaligned) == ALIGNMENT       # ... and 64 are taken
    if kv8:
        assert call(c_st=112) == BAD_ARG and call(c_sb=-16) == BAD_ARG and call(i_sb=-1) == BAD_ARG and call(i_sh=-1) == BAD_ARG
        assert call(ki=p + 2) == ALIGNMENT and call(vi=p + 1) == ALIGNMENT
        assert call(ki=p + 4, ws_floats=need - 1) == BAD_ARG            # a factor array needs 4 bytes only
    # one misaligned pointer and one misaligned row stride at a time; with a second fault of the other kind it is BAD_ARG
    for name in ("q", "k", "v", "kc", "vc", "out"):
        assert call(**{name: p + 8}) == ALIGNMENT, name
    for name in ("q_ld", "k_ld", "v_ld"):
        assert call(**{name: 2052}) == ALIGNMENT, name                  # 4104 bytes
    for name, val in (("c_sb", (1 << 20) + 4), ("c_sh", (1 << 18) + 4), ("c_st", 132 if not kv8 else 136)):
        assert call(**{name: val}) == ALIGNMENT, name
    for other in (dict(ws_floats=need - 1), dict(ws=None), dict(splits=-1), dict(kv_ld=1030), dict(hd=80), dict(t=-1)):
        assert call(**misaligned, **other) == BAD_ARG, other
        assert call(q_ld=2052, **other) == BAD_ARG, other
    # B == 0: nothing to do.  What is checked before that point differs per entry point and stays as it was: all three have
    # looked at the pointers, the geometry and the mask row; cmb_decode_attn_kv8 alone has also planned the splits.
    assert call(B=0) == OK and call(B=0, ws=None, ws_floats=0) == OK
    assert call(B=0, **misaligned) == OK and call(B=0, q_ld=2052) == OK
    assert call(B=0, hd=80) == BAD_ARG and call(B=0, kv_ld=1030) == BAD_ARG and call(B=0, t=-1) == BAD_ARG
    assert call(B=0, splits=mx.value + 1) == (BAD_ARG if kv8 else OK)
    if kv8:
        assert call(B=0, c_st=112) == BAD_ARG
    del raw


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
