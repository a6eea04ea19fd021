"""CPU: the host side of ``cmb_extend_attn`` (extend_attn.hip) — ``ops.extend_mask`` against a double loop, the argument checks
and the two host queries through ctypes (nothing is launched), and the basis of test_extend_attn_gpu.py's per-16-row block
checks: ``attn_check.twin``, the one model of legal bf16 rounding, measured over exactly the cases that test runs.

Twin figures (worst block error over BLOCK_CASES, last Q rows, blocks of 16 rows from row t0): gauss 0.0024, peaked 0.0018,
diag 0.0017; attn_check.TOL["..."]["o"] is 9e-3 / 9e-3 / 8e-3, so the module's rule 3 x twin <= TOL holds."""
import ctypes as C

import pytest
import torch

import attn_check as A

# (nh, nkv, hd) x (t0, Q) of the per-block checks; B = 2: row 0 has masked cached keys, row 1 a left-padded chunk
BLOCK_HEADS = [(4, 2, 64), (8, 1, 128), (7, 1, 128), (3, 3, 96), (4, 4, 64)]
BLOCK_CHUNKS = [(0, 17), (1, 33), (127, 130), (300, 50), (64, 16)]


def block_key_valid(t0, Q):
    """bool [2, t0 + Q]: row 0 with ``attn_check.mutant_key_valid``'s holes in the cached part ([:5] and every third from 7),
    row 1 left-padded for the first Q // 3 slots of the chunk."""
    S = t0 + Q
    kv = torch.ones(2, S, dtype=torch.bool)
    holes = A.mutant_key_valid(1, S)[0]
    kv[0, :t0] = holes[:t0]
    kv[1, t0:t0 + Q // 3] = False
    return kv


def block_case(family, nh, nkv, hd, t0, Q):
    """(q, k, v [2, heads, S, hd] bf16, key_valid, fp64 reference of the last Q rows [2, nh, Q, hd], allow)."""
    S = t0 + Q
    q, k, v, w = A.inputs(family, 2, nh, nkv, S, hd, seed=1000 * t0 + Q)
    kv = block_key_valid(t0, Q)
    allow = A.causal_allow(S, kv)
    ref = A.reference(q, k, v, w, allow)[0][:, :, t0:]
    return q, k, v, w, kv, ref, allow


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_extend_mask_is_the_brute_force_rule():
    from cambrian_amd import ops
    g = torch.Generator().manual_seed(3)
    for B, t0, Q in ((1, 0, 1), (2, 0, 5), (3, 7, 1), (2, 9, 6), (2, 33, 17)):
        km = torch.rand(B, t0 + Q + 3, generator=g) < 0.6             # holes in the cached part and in the chunk
        km[B - 1, t0:t0 + Q // 3] = False                              # a left-padded chunk
        km[:, t0 + Q:] = True                                          # columns past the chunk are not looked at
        got = ops.extend_mask(km, t0, Q)
        assert got.shape == (B, Q, t0 + Q) and got.dtype == torch.bool
        for b in range(B):
            for j in range(Q):
                for s in range(t0 + Q):
                    want = s <= t0 + j and (bool(km[b, s]) or s == t0 + j)
                    assert bool(got[b, j, s]) == want, (B, t0, Q, b, j, s)


def test_extend_attn_arguments_are_checked_before_any_launch(built):
    """The status per kind of mistake and the order of the checks (cmb_decode_attn_multi's: NULL pointers, geometry and range,
    B == 0, the plan and the workspace, alignment).  Every case returns before anything is launched; the pointers are never
    dereferenced."""
    lib = built.load()
    ok, bad_arg, alignment = 0, -1, -2
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def f(q=p, k=p, v=p, cos=p, sin=p, kc=p, vc=p, kv=p, out=p, q_ld=1024, k_ld=1024, v_ld=1024, c_sb=65536, c_sh=8192, c_st=128,
          B=2, nh=8, nkv=2, hd=128, Q=40, t0=100, kv_ld=200, splits=1, ws=None, ws_floats=0):
        return lib.cmb_extend_attn(q, q_ld, k, k_ld, v, v_ld, cos, sin, kc, vc, c_sb, c_sh, c_st, B, nh, nkv, hd, Q, t0, kv, kv_ld,
                                   0.088, splits, ws, ws_floats, out, None)

    for name in ("q", "k", "v", "cos", "sin", "kc", "vc", "kv", "out"):
        assert f(**{name: None}) == bad_arg, f"NULL {name}"
        assert f(**{name: None}, B=0) == bad_arg                         # the null test comes first
    assert f(hd=80) == bad_arg and f(hd=256) == bad_arg
    assert f(nh=7, nkv=2) == bad_arg and f(nh=18, nkv=2) == bad_arg and f(nh=0) == bad_arg and f(nkv=0) == bad_arg
    assert f(Q=0) == bad_arg and f(Q=4097, kv_ld=5000) == bad_arg and f(Q=-1) == bad_arg
    assert f(B=-1) == bad_arg and f(B=65536) == bad_arg and f(nh=4 * 65536, nkv=65536) == bad_arg
    assert f(t0=-1) == bad_arg and f(kv_ld=139) == bad_arg
    assert f(B=0) == ok
    assert f(B=0, q_ld=4) == ok and f(B=0, splits=99) == ok and f(B=0, splits=2) == ok    # before the plan and the strides
    assert f(B=0, hd=80) == bad_arg and f(B=0, kv_ld=139) == bad_arg                       # after geometry and range
    mx = C.c_int32(0)
    assert lib.cmb_extend_attn_plan(1, 1, 0, 1, 0, None, None, C.byref(mx)) == ok and mx.value >= 2
    assert f(splits=-1) == bad_arg and f(splits=mx.value + 1) == bad_arg
    assert f(t0=2 ** 31 - 30, kv_ld=2 ** 31 + 50) == bad_arg
    need = lib.cmb_extend_attn_ws(2, 8, 2, 128, 40, 100, 2)
    assert need == 2 * 40 * 8 * 2 * 130
    assert f(splits=2) == bad_arg and f(splits=2, ws=p, ws_floats=need - 1) == bad_arg       # no / a short workspace
    assert f(splits=2, ws=p, ws_floats=need - 1, q_ld=4) == bad_arg                          # ... before the alignment test
    assert f(q_ld=4) == alignment and f(k_ld=1028) == alignment and f(v_ld=2) == alignment
    assert f(c_sb=4) == alignment and f(c_sh=12) == alignment and f(c_st=132) == alignment
    for name in ("q", "k", "v", "kc", "vc", "out"):
        assert f(**{name: p + 8}) == alignment, name


def test_extend_attn_plan_and_ws_are_pure_functions(built):
    lib = built.load()
    from cambrian_amd import ops
    mx = ops.decode_attention_max_splits()
    for B, nkv, t0, Q in ((1, 8, 0, 1), (1, 8, 640, 32), (8, 8, 640, 32), (1, 8, 2048, 256), (2, 2, 127, 130), (1, 1, 5000, 4096),
                          (1, 2, 991, 40), (3, 1, 0, 17)):
        for forced in (0, 1, 2, 3, mx):
            s, ch = ops.extend_attention_plan(B, nkv, t0, Q, forced)
            assert (s, ch) == ops.extend_attention_plan(B, nkv, t0, Q, forced)
            assert 1 <= s <= mx and s * ch >= t0 + Q > (s - 1) * ch, (B, nkv, t0, Q, forced, s, ch)
            if forced:
                assert s <= forced
            for nh, hd in ((nkv, 64), (4 * nkv, 128), (7 * nkv, 96)):
                need = lib.cmb_extend_attn_ws(B, nh, nkv, hd, Q, t0, forced)
                assert need == (0 if s == 1 else B * Q * nh * s * (hd + 2))
                assert need == lib.cmb_extend_attn_ws(B, nh, nkv, hd, Q, t0, forced)
    # the row blocks count as batch rows: a long chunk splits no more than a 16-token one of the same cache length
    assert ops.extend_attention_plan(1, 8, 2048, 256)[0] <= ops.extend_attention_plan(1, 8, 2048 + 240, 16)[0]
    s, ch = C.c_int32(7), C.c_int64(7)
    for bad in ((0, 8, 10, 4, 0), (1, 0, 10, 4, 0), (1, 8, -1, 4, 0), (1, 8, 10, 0, 0), (1, 8, 10, 4097, 0), (1, 8, 10, 4, -1),
                (1, 8, 10, 4, mx + 1), (1, 8, 2 ** 31, 4, 0)):
        assert lib.cmb_extend_attn_plan(*bad, C.byref(s), C.byref(ch), None) == -1, bad
    assert lib.cmb_extend_attn_ws(1, 8, 8, 80, 4, 10, 0) == -1 and lib.cmb_extend_attn_ws(1, 9, 2, 64, 4, 10, 0) == -1
    assert lib.cmb_extend_attn_ws(1, 8, 8, 64, 4097, 10, 0) == -1
    assert ops.extend_attention_supported(torch.bfloat16, 32, 8, 128, 4096)
    assert not ops.extend_attention_supported(torch.bfloat16, 32, 8, 128, 4097)
    assert not ops.extend_attention_supported(torch.bfloat16, 32, 8, 128, 0)
    assert not ops.extend_attention_supported(torch.float32, 32, 8, 128, 4)
    assert not ops.extend_attention_supported(torch.bfloat16, 36, 4, 128, 4)
    assert not ops.extend_attention_supported(torch.bfloat16, 8, 8, 80, 4)


@pytest.mark.parametrize("family", A.FAMILIES)
def test_twin_meets_the_block_tolerance_on_the_gpu_cases(family):
    """3 x (block error of attn_check.twin) <= attn_check.TOL[family]["o"] over the cases of
    test_extend_attn_gpu.py::test_block_errors: the tolerance comes from the model of legal rounding, never from a kernel."""
    worst = 0.0
    for nh, nkv, hd in BLOCK_HEADS:
        for t0, Q in BLOCK_CHUNKS:
            q, k, v, w, kv, ref, allow = block_case(family, nh, nkv, hd, t0, Q)
            tw = A.twin(q, k, v, w, allow)[0][:, :, t0:]
            e = A.block_err(tw, ref)
            worst = max(worst, e)
            assert 3 * e <= A.TOL[family]["o"], f"{family} {nh}/{nkv}/{hd} t0={t0} Q={Q}: twin block error {e}"
    print(f"{family}: worst twin block error {worst:.3g}")
