"""`-m gpu`: the decode-step linear on weight-only e4m3 weights — ``cmb_decode_linear_fp8`` (decode_linear_fp8.hip) through
``ops.decode_linear_fp8``, ``ops.decode_fp8_weight``, the decoder layers' ``decode(..., fp8=True)`` and the generate loop.

Kernel tests quantise on the CPU with ``torch.float8_e4m3fn`` (amax -> 448, inv_scale = amax / 448), so they do not depend on
the GPU quantiser, and compare with float64 computed from the operands AS STORED: ref = (x . q^T) * inv_scale, with seeded
randn rounded to bf16 and W scaled by K^-0.5 before it is quantised.  One weight matrix, one 16-row x and their float64
products are made per K and shared by every case of that K.

Plain epilogue, elementwise:  |out - ref| <= 2^-8 |ref| + (K + 2) 2^-24 (inv_scale sum_k |x_k q_k| + |r|)
— one bf16 rounding of the result (2^-23 |ref| for an fp32 store) plus the worst-case error of an fp32 sum of K + 1 terms in
any order plus the one multiplication by the row factor; derived, not tuned.  Every e4m3 value is a bf16 and every product of
two bf16 is exact in fp32, so the sum is the only place the kernel rounds before the factor.  ``_cpu_fp32_inside_bound``
evaluates the same operands with a plain fp32 torch.matmul, scaled and rounded to bf16 on the CPU: the seeds (31 + K) are ones
for which that evaluation stays inside the bound too, and the test re-checks it.
The lane-map test is bit-exact: a weight matrix with a single 1.0 per row makes out[m, n] = x[m, k(n)], so any byte order or
k permutation that differs between the converted weight fragment and the x fragment shows as a wrong element, which a
tolerance could hide.
Norm prologue / SwiGLU: ``rel_err < TOL["bf16"]`` AND a least-squares slope within 5e-3 against the float64 un-fused formula
on the dequantised weights (test_decode_linear_gpu.py's criteria).
``ops.decode_fp8_weight``: |w - q inv| <= 2^-4 |w| + 2^-10 amax / 448 + 2^-22 |w| — e4m3 has 3 mantissa bits, so a normal
value is within half an ulp = 2^-4 of itself; below 2^-6 (in quantised units) the grid is uniform with spacing 2^-9, half of
which is 2^-10, times the row factor amax / 448; the last term covers the three fp32 roundings of the scale, the scaled
value and the factor (3 x 2^-24).

The kernel has ONE instantiation in M, so batch invariance is bit-equality."""
import copy
import functools

import pytest
import torch

from conftest import TOL, fit_err, rel_err

pytestmark = pytest.mark.gpu

KS = [16, 112, 128, 144, 400, 4096, 14336]   # one chunk, a ragged step, one step, a step + a chunk, 3 steps + ragged, the real sizes
MS = [1, 3, 16]
NMAX = 4104                             # rows of the shared weight matrix (>= 4096 and 2048 + 1024 + slab)
UP0 = 2048                              # first "up" row the SwiGLU cases take from the shared matrix
EPS = 1e-5
SEED = 31
ONE = 0x38                              # e4m3fn code of 1.0


def _ops():
    from cambrian_amd import ops
    return ops


def _quant_cpu(w):
    """bf16 / fp32 [N, K] on the CPU -> (uint8 e4m3fn bytes, fp32 inv_scale), the format of cmb_quantize_fp8_rows."""
    wf = w.float()
    amax = wf.abs().amax(1)
    inv = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (wf * torch.where(amax > 0, 448.0 / amax, torch.ones_like(amax))[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), inv


def _e4m3(q):
    return q.view(torch.float8_e4m3fn)


@functools.lru_cache(maxsize=None)
def _data(K):
    """Shared per K, never modified: bf16 x [16, K] (row 1 is zero), e4m3 bytes q [NMAX, K] with their factors, norm
    weights, residual, and the float64 products (x q^T) inv, (|x| |q|^T) inv and (RMSNorm(x) q^T) inv."""
    g = torch.Generator().manual_seed(SEED + K)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    x[1] = 0
    w = (torch.randn(NMAX, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    res = torch.randn(16, NMAX, generator=g).to(torch.bfloat16)
    q, inv = _quant_cpu(w)
    xd, qd, invd = x.double(), _e4m3(q).double(), inv.double()
    y = (xd @ qd.t()) * invd
    ya = (xd.abs() @ qd.abs().t()) * invd
    xn = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double()
    yn = (xn @ qd.t()) * invd
    return dict(x=x, q=q, inv=inv, nw=nw, res=res, y=y, ya=ya, yn=yn)


@functools.lru_cache(maxsize=None)
def _dev_data(K, dev):
    d = _data(K)
    return {k: d[k].to(dev) for k in ("x", "q", "inv", "nw", "res")}


def _bound(ref, mag, K, f32):
    return (2.0 ** -23 if f32 else 2.0 ** -8) * ref.abs() + (K + 2) * 2.0 ** -24 * mag


def _cpu_fp32_inside_bound(d, K, M, N):
    y32 = ((d["x"][:M].float() @ _e4m3(d["q"][:N]).float().t()) * d["inv"][:N]).to(torch.bfloat16).double()
    return bool(((y32 - d["y"][:M, :N]).abs() <= _bound(d["y"][:M, :N], d["ya"][:M, :N], K, False)).all())


def _slab(K, act=None):
    return _ops().decode_linear_fp8_plan(1, 4096, K, act)[0]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_plain_epilogue_inside_the_derived_bound(dev, K, M):
    ops = _ops()
    d, g = _data(K), _dev_data(K, dev)
    slab = _slab(K)
    assert _cpu_fp32_inside_bound(d, K, M, 4096), "the seed's own fp32 evaluation leaves the bound: pick another seed"
    for N in sorted({1, 2, 30, slab - 1, slab, slab + 1, 4096}):
        for use_res in (False, True):
            for f32 in (False, True):
                out = ops.decode_linear_fp8(g["x"][:M], g["q"][:N], g["inv"][:N], residual=g["res"][:M, :N] if use_res else None,
                                            out_dtype=torch.float32 if f32 else None)
                assert out.shape == (M, N) and out.dtype == (torch.float32 if f32 else torch.bfloat16)
                ref, mag = d["y"][:M, :N], d["ya"][:M, :N]
                if use_res:
                    ref, mag = ref + d["res"][:M, :N].double(), mag + d["res"][:M, :N].double().abs()
                err = (out.double().cpu() - ref).abs()
                worst = float((err / _bound(ref, mag, K, f32).clamp_min(1e-300)).max())
                print(f"K={K} M={M} N={N} res={use_res} f32={f32}: max err / bound {worst:.3g}")
                assert torch.isfinite(out).all()
                assert worst <= 1.0, f"N={N} res={use_res} f32={f32}: error {worst:.3g} x the bound"
                if M > 1:                                                   # the zero row of x: exactly the residual, or 0
                    assert torch.equal(out[1], g["res"][1, :N].to(out.dtype)) if use_res else not out[1].any()


def test_lane_map_bit_for_bit(dev):
    """K = N = 400: q[n, k] = 1.0 where k == 7 n mod 400, else 0 — out[m, n] is x[m, 7 n mod 400], bit for bit."""
    ops = _ops()
    K = N = 400
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    n = torch.arange(N)
    k = (7 * n) % K
    assert len(set(k.tolist())) == N                      # 7 and 400 are coprime: every k is some row's
    q = torch.zeros(N, K, dtype=torch.uint8)
    q[n, k] = ONE
    assert float(_e4m3(q)[3, 21].float()) == 1.0
    want = x[:, k]
    xg, qg = x.to(dev), q.to(dev)
    out = ops.decode_linear_fp8(xg, qg, torch.ones(N, device=dev))
    bad = (out.cpu().view(torch.int16) != want.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first (m, n) = {bad[0].tolist()}: k = {int(k[bad[0][1]])}"
    inv = 2.0 ** -(n % 5).float()
    out = ops.decode_linear_fp8(xg, qg, inv.to(dev))
    scaled = (x[:, k].float() * inv).to(torch.bfloat16)   # a power of two: exact
    assert torch.equal(out.cpu().view(torch.int16), scaled.view(torch.int16))
    out = ops.decode_linear_fp8(xg, qg, inv.to(dev), out_dtype=torch.float32)
    assert torch.equal(out.cpu(), x[:, k].float() * inv)
    # every byte position of a lane's 16, one at a time, through the norm-free SwiGLU rows as well: gate row j picks k, up
    # row j picks k + 1 (mod K)
    qs = torch.zeros(2 * N, K, dtype=torch.uint8)
    qs[n, k] = ONE
    qs[N + n, (k + 1) % K] = ONE
    out = ops.decode_linear_fp8(xg, qs.to(dev), torch.ones(2 * N, device=dev), act="swiglu", out_dtype=torch.float32)
    gate, up = x[:, k].double(), x[:, (k + 1) % K].double()
    ref = gate * torch.sigmoid(gate) * up
    assert float(((out.double().cpu() - ref).abs() / ref.abs().clamp_min(1e-30)).max()) < 1e-5


@pytest.mark.parametrize("N,K", [(8200, 112), (16400, 272)])
def test_larger_slabs_inside_the_bound(dev, N, K):
    """The 32-row instantiation (N >= 32 x CUs), ragged last workgroup, M = 16 and a residual."""
    ops = _ops()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert ops.decode_linear_fp8_plan(16, N, K)[0] == ops.decode_linear_fp8_plan(16, N, K, None, cus)[0]
    if cus == 256:
        assert ops.decode_linear_fp8_plan(16, N, K)[0] == 32
    g = torch.Generator().manual_seed(SEED + N)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    q, inv = _quant_cpu((torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    r = torch.randn(16, (N + 7) // 8 * 8, generator=g).to(torch.bfloat16)             # row stride: a multiple of 8
    ref = (x.double() @ _e4m3(q).double().t()) * inv.double() + r[:, :N].double()
    mag = (x.double().abs() @ _e4m3(q).double().abs().t()) * inv.double() + r[:, :N].double().abs()
    out = ops.decode_linear_fp8(x.to(dev), q.to(dev), inv.to(dev), residual=r.to(dev)[:, :N])
    worst = float(((out.double().cpu() - ref).abs() / _bound(ref, mag, K, False)).max())
    print(f"N={N} K={K}: max err / bound {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_norm_prologue_and_swiglu(dev, K, M):
    ops = _ops()
    d, g = _data(K), _dev_data(K, dev)
    nslab, slab = _slab(K), _slab(K, "swiglu")
    tol = TOL["bf16"]

    def check(out, ref, what):
        e = rel_err(out, ref)
        slope, l2 = fit_err(out, ref)
        print(f"K={K} M={M} {what}: rel err {e:.3g} slope err {slope:.3g} l2 {l2:.3g}")
        assert torch.isfinite(out).all()
        assert e < tol and slope < 5e-3, f"{what}: rel err {e}, slope off by {slope}"

    for N in sorted({1, 2, 30, nslab - 1, nslab, nslab + 1, 4096}):             # norm prologue alone, with and without residual
        ref = d["yn"][:M, :N]
        check(ops.decode_linear_fp8(g["x"][:M], g["q"][:N], g["inv"][:N], norm_weight=g["nw"], eps=EPS), ref, f"norm N={N}")
        out = ops.decode_linear_fp8(g["x"][:M], g["q"][:N], g["inv"][:N], norm_weight=g["nw"], eps=EPS, residual=g["res"][:M, :N])
        check(out, ref + d["res"][:M, :N].double(), f"norm + residual N={N}")
        if M > 1:
            assert torch.equal(out[1], g["res"][1, :N])                         # the zero row: finite, exactly the residual
    for inter in sorted({1, 15, slab // 2 + 1, 1024}):
        q = torch.cat([g["q"][:inter], g["q"][UP0:UP0 + inter]], 0)
        # gate and up rows under different factors: the up rows' doubled (a power of two: the reference doubles exactly)
        inv = torch.cat([g["inv"][:inter], 2 * g["inv"][UP0:UP0 + inter]], 0)
        for norm in (False, True):
            y = d["yn"] if norm else d["y"]
            gate, up = y[:M, :inter], 2 * y[:M, UP0:UP0 + inter]
            ref = gate * torch.sigmoid(gate) * up
            out = ops.decode_linear_fp8(g["x"][:M], q, inv, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu")
            assert out.shape == (M, inter)
            check(out, ref, f"swiglu I={inter} norm={norm}")
            if M > 1:
                assert not out[1].any()                                         # the zero row gives silu(0) * 0 = 0
            f32 = ops.decode_linear_fp8(g["x"][:M], q, inv, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu",
                                        out_dtype=torch.float32)
            assert torch.equal(f32.to(torch.bfloat16), out)                     # one rounding at the store


def test_swiglu_32_row_slab(dev):
    ops = _ops()
    inter, K = 8200, 112
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    q, inv = _quant_cpu((torch.randn(2 * inter, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    inv[inter:] *= 0.5
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    xd = x.double()
    for norm in (False, True):
        xx = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double() if norm else xd
        y = (xx @ _e4m3(q).double().t()) * inv.double()
        ref = y[:, :inter] * torch.sigmoid(y[:, :inter]) * y[:, inter:]
        out = ops.decode_linear_fp8(x.to(dev), q.to(dev), inv.to(dev), act="swiglu", norm_weight=nw.to(dev) if norm else None, eps=EPS)
        assert rel_err(out, ref) < TOL["bf16"] and fit_err(out, ref)[0] < 5e-3, f"norm={norm}"


def test_views_touch_nothing_around_them(dev):
    """x is a column slice of a wider buffer whose other rows and columns are NaN, Wq has 0xFF (NaN) padding columns and
    rows, inv_scale is a slice of a longer vector of NaN, residual and out are slices of wider buffers; out's surroundings
    hold a sentinel and keep their bits."""
    ops = _ops()
    K, N, M = 272, 30, 3
    d = _data(K)
    nan = float("nan")
    xbuf = torch.full((M + 2, K + 24), nan, dtype=torch.bfloat16)
    xbuf[:M, 8:8 + K] = d["x"][2:2 + M]
    qbuf = torch.full((N + 1, K + 32), 0xFF, dtype=torch.uint8)
    qbuf[:N, 16:16 + K] = d["q"][:N]
    ibuf = torch.full((N + 5,), nan)
    ibuf[3:3 + N] = d["inv"][:N]
    rbuf = torch.full((M + 1, N + 18), nan, dtype=torch.bfloat16)
    rbuf[:M, 16:16 + N] = d["res"][:M, :N]
    xbuf, qbuf, ibuf, rbuf = xbuf.to(dev), qbuf.to(dev), ibuf.to(dev), rbuf.to(dev)
    x, q, inv, r = xbuf[:M, 8:8 + K], qbuf[:N, 16:16 + K], ibuf[3:3 + N], rbuf[:M, 16:16 + N]
    g = _dev_data(K, dev)
    cx, cq, ci = d["x"][2:2 + M].to(dev), d["q"][:N].to(dev), d["inv"][:N].to(dev)
    want = ops.decode_linear_fp8(cx, cq, ci, residual=g["res"][:M, :N])
    assert torch.isfinite(want).all()
    for dt, sentinel in ((torch.bfloat16, -1.5), (torch.float32, -1.5)):
        obuf = torch.full((M + 2, N + 26), sentinel, dtype=dt, device=dev)
        out = obuf[1:1 + M, 8:8 + N]
        got = ops.decode_linear_fp8(x, q, inv, residual=r, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.to(torch.bfloat16), want)
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[1:1 + M, 8:8 + N] = False
        assert bool((obuf[mask] == sentinel).all())
    # the norm prologue reads x and the norm weights under the same rules
    a = ops.decode_linear_fp8(x, q, inv, norm_weight=g["nw"], eps=EPS)
    b = ops.decode_linear_fp8(cx, cq, ci, norm_weight=g["nw"], eps=EPS)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("K,N", [(4096, 4096), (272, 30)])
def test_same_call_same_bits_and_batch_invariance(dev, K, N):
    ops = _ops()
    g = _dev_data(K, dev)
    q, inv = g["q"][:N], g["inv"][:N]
    qg = torch.cat([g["q"][:N // 2], g["q"][UP0:UP0 + N // 2]], 0)
    ig = torch.cat([g["inv"][:N // 2], g["inv"][UP0:UP0 + N // 2]], 0)
    variants = [dict(), dict(residual=True), dict(norm_weight=g["nw"], eps=EPS), dict(out_dtype=torch.float32),
                dict(act="swiglu"), dict(norm_weight=g["nw"], eps=EPS, act="swiglu")]
    for kw in variants:
        def run(rows):
            k2 = dict(kw)
            qq, ii = (qg, ig) if k2.get("act") else (q, inv)
            if k2.pop("residual", False):
                k2["residual"] = g["res"][rows, :N]
            return ops.decode_linear_fp8(g["x"][rows], qq, ii, **k2)
        full = run(slice(0, 16))
        assert torch.equal(full, run(slice(0, 16))), f"{kw}: two runs differ"
        for m in (0, 1, 7, 15):                       # row m alone (M = 1) against row m of the M = 16 call: the same bits
            assert torch.equal(run(slice(m, m + 1))[0], full[m]), f"{kw}: row {m} depends on the batch"
        assert torch.equal(run(slice(0, 3)), full[:3])


def test_batch_invariance_across_slabs(dev):
    """The order in which a row's k are summed does not depend on the slab: row m alone, row m of the 16-row call and the same
    row computed as part of a shorter weight matrix (which the plan gives 8-row slabs) agree bit for bit."""
    ops = _ops()
    N, K = 6200, 112
    if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        assert ops.decode_linear_fp8_plan(16, N, K)[0] == 16 and ops.decode_linear_fp8_plan(16, 1000, K)[0] == 8
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16).to(dev)
    q, inv = _quant_cpu((torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    q, inv = q.to(dev), inv.to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    for kw in (dict(), dict(norm_weight=nw, eps=EPS), dict(norm_weight=nw, eps=EPS, act="swiglu")):
        full = ops.decode_linear_fp8(x, q, inv, **kw)
        for m in (0, 9, 15):
            assert torch.equal(ops.decode_linear_fp8(x[m:m + 1], q, inv, **kw)[0], full[m]), f"{kw}: row {m}"
        assert torch.equal(ops.decode_linear_fp8(x[:4], q, inv, **kw), full[:4])
        if not kw.get("act"):                          # the first 1000 rows alone: smaller slabs, the same bits
            assert torch.equal(ops.decode_linear_fp8(x, q[:1000], inv[:1000], **kw), full[:, :1000])


def test_decode_fp8_weight_on_the_gpu(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    N, K = 67, 4096
    g = torch.Generator().manual_seed(SEED)
    w = (torch.randn(N, K, generator=g) * K ** -0.5 * (1 + torch.arange(N)[:, None] % 5)).to(torch.bfloat16)
    w[5] = 0
    w[6, 1:] = 0                                          # a single non-zero
    q, inv = ops.decode_fp8_weight(w.to(dev))
    assert q.shape == (N, K) and q.dtype == torch.uint8 and inv.shape == (N,) and inv.dtype == torch.float32
    assert ops.decode_linear_fp8_supported(torch.zeros(1, K, dtype=torch.bfloat16, device=dev), q, inv)
    q, inv = q.cpu(), inv.cpu()
    amax = w.double().abs().amax(1)
    assert float(inv[5]) == 1.0 and not q[5].any()        # a zero row: factor 1 and zero bytes
    live = amax > 0
    assert float(((inv.double() - amax / 448).abs() / (amax / 448).clamp_min(1e-300))[live].max()) <= 2.0 ** -23
    deq = _e4m3(q).double() * inv.double()[:, None]
    wd = w.double()
    bound = 2.0 ** -4 * wd.abs() + 2.0 ** -10 * (amax / 448)[:, None] + 2.0 ** -22 * wd.abs()
    worst = float(((deq - wd).abs() / bound.clamp_min(1e-300)).max())
    print(f"decode_fp8_weight: max |w - q inv| / bound {worst:.3g}")
    assert torch.isfinite(deq).all() and worst <= 1.0
    assert (_e4m3(q).float().abs().amax(1)[live] == 448).all()       # the row's largest magnitude maps to 448
    assert torch.equal(_quant_cpu(w)[1], inv)              # the CPU quantiser of these tests writes the same factors
    # the quantiser's reach ends at K = 16384: refused, not quantised in pieces
    big = torch.zeros(8, 20480, dtype=torch.bfloat16, device=dev)
    assert ops.decode_linear_fp8_weight_supported(1, big[:, :16384]) and not ops.decode_linear_fp8_weight_supported(1, big)
    with pytest.raises(CambrianAmdError):
        ops.decode_fp8_weight(big)
    with pytest.raises(CambrianAmdError):
        ops.decode_fp8_weight(w.to(dev).requires_grad_())
    with pytest.raises(CambrianAmdError):
        ops.decode_fp8_weight(w.to(dev).float())


# ---- the decoder layer's decode(..., fp8=True): four fp8 launches + attention against the stock sequence on a twin ----
def _spies(monkeypatch):
    ops = _ops()
    calls = {"fp8": 0, "bf16": 0}
    real8, real16 = ops.decode_linear_fp8, ops.decode_linear

    def counted8(*a, **kw):
        calls["fp8"] += 1
        return real8(*a, **kw)

    def counted16(*a, **kw):
        calls["bf16"] += 1
        return real16(*a, **kw)

    monkeypatch.setattr(ops, "decode_linear_fp8", counted8)
    monkeypatch.setattr(ops, "decode_linear", counted16)
    return calls


def _e4m3_round(v):
    """fp32 values of magnitude <= 448 rounded to the e4m3fn grid (nearest, ties to even), on any device and without the fp8
    dtype: 3 mantissa bits above 2^-6, the uniform 2^-9 grid below."""
    _, exp = torch.frexp(v.abs().clamp_min(2.0 ** -6))          # |v| = m 2^exp, m in [0.5, 1): the ulp is 2^(exp - 4)
    step = torch.exp2((exp - 4).float())
    return torch.round(v / step) * step


def _dequantised_twin(layer):
    """A copy of the layer whose matrices are the bf16-rounded dequantised ones (row by row: a packed [q; k; v] or
    [gate; up] has the rows of its parts), without the copies the original has cached."""
    twin = copy.deepcopy(layer)
    with torch.no_grad():
        for mod in twin.modules():
            for k in [k for k in mod.__dict__ if k.startswith("_w")]:
                del mod.__dict__[k]
        for p in twin.parameters():
            if p.dim() == 2:
                wf = p.detach().float()
                amax = wf.abs().amax(1, keepdim=True).clamp_min(1e-30)
                p.copy_((_e4m3_round(wf * (448.0 / amax)) * (amax / 448.0)).to(p.dtype))
    return twin


def _decode_inputs(dev, dt, hidden, nkv, hd, B):
    from test_decode_attn_gpu import TAIL, THETA, _masks
    ops = _ops()
    n = 37
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 1, hidden, generator=g).to(dt).to(dev)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    mask = _masks(B, n)[1][1].to(dev)
    cos, sin = ops.rope_table(torch.randint(20, 37, (B, 1), generator=g).to(dev), hd, THETA)
    return x, kc, vc, mask, cos, sin, n - 1


GEOMS = [("llama", 256, 512, 4, 4, 3), ("llama", 256, 512, 4, 2, 3), ("llama", 512, 1024, 4, 1, 3),
         ("phi3", 256, 512, 4, 4, 3), ("phi3", 256, 512, 4, 2, 3), ("phi3", 512, 1024, 4, 1, 3),
         ("llama", 4096, 14336, 32, 8, 1), ("llama", 4096, 14336, 32, 8, 16)]


@pytest.mark.parametrize("lm,hidden,inter,nh,nkv,B", GEOMS)
def test_layer_decode_fp8_vs_stock_sequence_on_dequantised_twin(dev, monkeypatch, lm, hidden, inter, nh, nkv, B):
    from test_decode_linear_gpu import _make_layer
    hd = hidden // nh
    dt = torch.bfloat16
    layer = _make_layer(dev, dt, lm, hidden, inter, nh, nkv, frozen=True)
    twin = _dequantised_twin(layer)
    calls = _spies(monkeypatch)
    x, kc, vc, mask, cos, sin, t = _decode_inputs(dev, dt, hidden, nkv, hd, B)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8", raising=False)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "1")
    k1, v1 = kc.clone(), vc.clone()
    with torch.no_grad():
        y1 = layer.decode(x, cos, sin, k1, v1, t, mask, fp8=True)
    assert (calls["fp8"], calls["bf16"]) == (4, 0), f"calls with the mode on: {calls}"
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "0")
    k0, v0 = kc.clone(), vc.clone()
    with torch.no_grad():
        y0 = twin.decode(x, cos, sin, k0, v0, t, mask)
    assert (calls["fp8"], calls["bf16"]) == (4, 0)
    assert y1.shape == y0.shape == (B, 1, hidden) and torch.isfinite(y1).all()
    e = rel_err(y1, y0)
    print(f"{lm} {hidden}/{inter} B={B}: layer out rel err {e:.3g}")
    assert e < TOL["bf16"]
    keep = torch.ones(k1.shape[2], dtype=torch.bool)
    keep[t] = False
    assert torch.equal(v1[:, :, keep], v0[:, :, keep]) and torch.equal(k1[:, :, keep], k0[:, :, keep])
    assert rel_err(v1[:, :, t], v0[:, :, t]) < TOL["bf16"] and rel_err(k1[:, :, t], k0[:, :, t]) < TOL["bf16"]
    # the copies are cached on their owners, and a second step makes none
    owners = [m for m in layer.modules() if any(k.endswith("_fp8") for k in m.__dict__)]
    assert sum(k.endswith("_fp8") for m in owners for k in m.__dict__) == 4
    ptrs = sorted(m.__dict__[k][1][0].data_ptr() for m in owners for k in m.__dict__ if k.endswith("_fp8"))
    with torch.no_grad():
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "1")
        y2 = layer.decode(x, cos, sin, kc.clone(), vc.clone(), t, mask, fp8=True)
    assert torch.equal(y2, y1)
    assert ptrs == sorted(m.__dict__[k][1][0].data_ptr() for m in owners for k in m.__dict__ if k.endswith("_fp8"))


@pytest.mark.parametrize("lm", ["llama", "phi3"])
@pytest.mark.parametrize("why", ["batch17", "fp32", "trainable"])
def test_layer_decode_fp8_is_not_taken_outside_the_conditions(dev, monkeypatch, lm, why):
    from test_decode_linear_gpu import _make_layer
    dt = torch.float32 if why == "fp32" else torch.bfloat16
    B = 17 if why == "batch17" else 3
    hidden, nh, nkv = 256, 4, 2
    layer = _make_layer(dev, dt, lm, hidden, 2 * hidden, nh, nkv, frozen=why != "trainable")
    calls = _spies(monkeypatch)
    x, kc, vc, mask, cos, sin, t = _decode_inputs(dev, dt, hidden, nkv, hidden // nh, B)
    res = []
    for fp8 in (True, False):
        k1, v1 = kc.clone(), vc.clone()
        with torch.no_grad():
            res.append((layer.decode(x, cos, sin, k1, v1, t, mask, fp8=fp8), k1, v1))
    assert calls == {"fp8": 0, "bf16": 0}
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert not any(k.endswith("_fp8") for m in layer.modules() for k in m.__dict__)       # and no copy was made


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_layer_with_one_refused_weight_makes_no_copy_and_runs_as_without_the_mode(dev, monkeypatch, lm):
    """intermediate = 520: down_proj has K = 520, a multiple of 8 (the bf16 five-launch step takes it) but not of 16.  The
    other three weights are acceptable and come first; none of them may be quantised or kept, the step is the bf16 one bit
    for bit, and the refusal is remembered: the second step asks the predicate nothing."""
    from test_decode_linear_gpu import _make_layer
    ops = _ops()
    dt = torch.bfloat16
    hidden, inter, nh, nkv, B = 256, 520, 4, 2, 3
    layer = _make_layer(dev, dt, lm, hidden, inter, nh, nkv, frozen=True)
    calls = _spies(monkeypatch)
    asked, made = [0], [0]
    real_ok, real_q = ops.decode_linear_fp8_weight_supported, ops.decode_fp8_weight
    monkeypatch.setattr(ops, "decode_linear_fp8_weight_supported", lambda *a, **k: (asked.__setitem__(0, asked[0] + 1), real_ok(*a, **k))[1])
    monkeypatch.setattr(ops, "decode_fp8_weight", lambda *a, **k: (made.__setitem__(0, made[0] + 1), real_q(*a, **k))[1])
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_LINEAR", raising=False)
    x, kc, vc, mask, cos, sin, t = _decode_inputs(dev, dt, hidden, nkv, hidden // nh, B)
    res = []
    for fp8 in (True, True, False):
        k1, v1 = kc.clone(), vc.clone()
        before = asked[0]
        with torch.no_grad():
            res.append((layer.decode(x, cos, sin, k1, v1, t, mask, fp8=fp8), k1, v1))
        res[-1] += (asked[0] - before,)
    assert calls == {"fp8": 0, "bf16": 12}, f"{calls}"            # three bf16 five-launch steps
    assert made[0] == 0, "a weight was quantised for a layer that does not take the mode"
    assert res[0][3] >= 1 and res[1][3] == 0 and res[2][3] == 0, f"predicate calls per step: {[r[3] for r in res]}"
    for a, b in ((res[0], res[2]), (res[1], res[2])):
        assert all(torch.equal(p, q) for p, q in zip(a[:3], b[:3]))
    assert not any(k.endswith("_fp8") for m in layer.modules() for k in m.__dict__)


def test_generate_decodes_on_fp8_weights(dev, monkeypatch):
    """With the mode on every decode step of the loop is 4 fp8 calls per layer plus the logits and no bf16 decode_linear;
    the first token comes from the bf16 prefill and equals the mode-off run's; the switch works from the config and from the
    environment (which overrides); the cached copies follow an in-place change of a weight."""
    from test_dynamic_gpu import _eval_batch
    from test_model_gpu import _build
    calls = _spies(monkeypatch)
    new = 4
    dt = torch.bfloat16
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8", raising=False)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_LINEAR", raising=False)
    model, cfg, towers = _build(dev, dt, monkeypatch, lm="llama", nkv=2)
    model.eval()
    layers = cfg.num_hidden_layers
    ids, att, sizes, images = _eval_batch(dev, dt, towers)
    ids, sizes, images = ids[:1], sizes[1:2], [i[1:2] for i in images]
    kw = dict(images=[i.to(dev, dt) for i in images], image_sizes=sizes, max_new_tokens=new)
    steps = (new - 1) * (4 * layers + 1)

    def run():
        calls["fp8"] = calls["bf16"] = 0
        toks = model.generate(ids.to(dev), **kw)
        assert toks.shape == (1, new)
        return toks, (calls["fp8"], calls["bf16"])

    off, n_off = run()
    assert n_off == (0, steps), f"mode off: {n_off}"
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    on, n_on = run()
    assert n_on == (steps, 0), f"CAMBRIAN_AMD_DECODE_FP8=1: {n_on}"
    assert torch.equal(on[:, 0], off[:, 0])                # the first token is the bf16 prefill's
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8")
    model.config.decode_fp8_weights = True
    on2, n_on2 = run()
    assert n_on2 == (steps, 0) and torch.equal(on2, on)    # the config flag; the same copies, the same tokens
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP8", "0")
    assert run()[1] == (0, steps)                          # the environment overrides the config
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8")

    # the cached copies follow their weights: an in-place change bumps _version and the next step requantises
    head = model.lm_head
    down = model.model.layers[0].mlp.down_proj
    att = model.model.layers[0].self_attn
    q_head, q_down, q_qkv = head.__dict__["_w_fp8"][1], down.__dict__["_w_fp8"][1], att.__dict__["_w_qkv_fp8"][1]
    with torch.no_grad():
        down.weight.mul_(2.0)
        head.weight[0].zero_()
        att.q_proj.weight.mul_(2.0)                        # one part of the packed [q; k; v]
    run()
    q_qkv2, nq = att.__dict__["_w_qkv_fp8"][1], att.q_proj.weight.shape[0]
    assert torch.equal(q_qkv2[0], q_qkv[0]) and torch.equal(q_qkv2[1][:nq], 2 * q_qkv[1][:nq])
    assert torch.equal(q_qkv2[1][nq:], q_qkv[1][nq:])
    q_head2, q_down2 = head.__dict__["_w_fp8"][1], down.__dict__["_w_fp8"][1]
    assert q_down2[0] is not q_down[0] and q_head2[0] is not q_head[0]
    assert torch.equal(q_down2[1], 2 * q_down[1])          # doubled weights: the same bytes, doubled factors
    assert torch.equal(q_down2[0], q_down[0])
    assert not q_head2[0][0].any() and float(q_head2[1][0]) == 1.0 and torch.equal(q_head2[0][1:], q_head[0][1:])


def test_bad_operands_raise(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(32, 64, dtype=torch.uint8, device=dev)
    inv = torch.ones(32, device=dev)
    assert ops.decode_linear_fp8(x, q, inv).shape == (2, 32)
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_linear_fp8(x.clone().requires_grad_(), q, inv)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp8(x, q, inv, act="swiglu", residual=torch.zeros(2, 16, dtype=torch.bfloat16, device=dev))
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp8(torch.zeros(17, 64, dtype=torch.bfloat16, device=dev), q, inv)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp8(x, q.to(torch.int8), inv)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp8(x, q, inv[:31])
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp8(x, q, inv.double())
    with pytest.raises(CambrianAmdError):                  # K = 24: a multiple of 8 that the bf16 kernel takes, not this one
        ops.decode_linear_fp8(x[:, :24], q[:, :32][:, :24], inv)
