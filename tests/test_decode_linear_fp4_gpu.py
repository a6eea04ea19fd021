"""`-m gpu`: the decode-step linear on MXFP4 weights — ``cmb_decode_linear_fp4`` (decode_linear_fp4.hip) through
``ops.decode_linear_fp4``, the quantiser ``cmb_quantize_mxfp4_rows`` through ``ops.decode_fp4_weight``, the decoder layers'
``decode(..., fp4=True)``, the one-call step with ``fp8`` = 2 and the generate loop, beam search included.  It mirrors
test_decode_linear_fp8_gpu.py case for case.

Kernel tests quantise on the CPU with tests/mxfp4_ref.py, so they do not depend on the GPU quantiser, and compare with float64
computed from the operands AS STORED: ref = x . deq^T with deq = e2m1(q) 2^(s - 127), seeded randn rounded to bf16 and W scaled
by K^-0.5 before it is quantised.  One weight matrix, one 16-row x and their float64 products are made per K and shared by
every case of that K.

Plain epilogue, elementwise:  |out - ref| <= 2^-8 |ref| + (K + 2) 2^-24 (sum_k |x_k w_k| + |r|)
— one bf16 rounding of the result (2^-23 |ref| for an fp32 store) plus the worst-case error of an fp32 sum of K + 1 terms in
any order; derived, not tuned.  Every dequantised value is a bf16 and every product of two bf16 is exact in fp32, so the sum is
the only place the kernel rounds.  ``_cpu_fp32_inside_bound`` evaluates the same operands with a plain fp32 torch.matmul
rounded to bf16 on the CPU: the seeds (31 + K) are ones for which that evaluation stays inside the bound too, and the test
re-checks it.
The lane-map test is bit-exact: a weight matrix with a single non-zero nibble per row makes out[m, n] = x[m, k(n)] value 2^s
rounded once, so any nibble order, byte order, k permutation or scale-byte mix-up between the converted weight fragment and
the x fragment shows as a wrong element, which a tolerance could hide.  It runs once per non-zero e2m1 code.
Norm prologue / SwiGLU: ``rel_err < TOL["bf16"]`` AND a least-squares slope within 5e-3 against the float64 un-fused formula on
the dequantised weights (test_decode_linear_gpu.py's criteria).
The GPU quantiser is compared bit for bit with the CPU restatement.

The kernel has ONE instantiation in M, so batch invariance is bit-equality."""
import copy
import functools

import pytest
import torch

import mxfp4_ref as R
from conftest import TOL, fit_err, rel_err

pytestmark = pytest.mark.gpu

KS = [32, 224, 256, 288, 800, 4096, 14336]   # one block, a ragged step, one step, a step + a block, 3 steps + ragged, the real sizes
MS = [1, 3, 16]
NMAX = 4104                             # rows of the shared weight matrix (>= 4096 and 2048 + 1024 + slab)
UP0 = 2048                              # first "up" row the SwiGLU cases take from the shared matrix
EPS = 1e-5
SEED = 31


def _ops():
    from cambrian_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _data(K):
    """Shared per K, never modified: bf16 x [16, K] (row 1 is zero), MXFP4 (q, s) of NMAX rows, norm weights, residual, and
    the float64 products x deq^T, |x| |deq|^T and RMSNorm(x) deq^T."""
    g = torch.Generator().manual_seed(SEED + K)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    x[1] = 0
    w = (torch.randn(NMAX, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    res = torch.randn(16, NMAX, generator=g).to(torch.bfloat16)
    q, s = R.quantize(w)
    xd, wd = x.double(), R.dequantize(q, s)
    y = xd @ wd.t()
    ya = xd.abs() @ wd.abs().t()
    xn = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double()
    yn = xn @ wd.t()
    return dict(x=x, q=q, s=s, w32=wd.float(), nw=nw, res=res, y=y, ya=ya, yn=yn)


@functools.lru_cache(maxsize=None)
def _dev_data(K, dev):
    d = _data(K)
    return {k: d[k].to(dev) for k in ("x", "q", "s", "nw", "res")}


def _bound(ref, mag, K, f32):
    return (2.0 ** -23 if f32 else 2.0 ** -8) * ref.abs() + (K + 2) * 2.0 ** -24 * mag


def _cpu_fp32_inside_bound(d, K, M, N):
    y32 = (d["x"][:M].float() @ d["w32"][:N].t()).to(torch.bfloat16).double()
    return bool(((y32 - d["y"][:M, :N]).abs() <= _bound(d["y"][:M, :N], d["ya"][:M, :N], K, False)).all())


def _slab(K, act=None):
    return _ops().decode_linear_fp4_plan(1, 4096, K, act)[0]


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
                out = ops.decode_linear_fp4(g["x"][:M], g["q"][:N], g["s"][:N], residual=g["res"][:M, :N] if use_res else None,
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
    """K = N = 800: row n holds one non-zero nibble, at k = 7 n mod 800 — out[m, n] is x[m, k] value 2^s rounded once to bf16
    (exact in fp32), bit for bit; once per non-zero e2m1 code, then with scale codes 120 .. 131 by block, then through SwiGLU."""
    ops = _ops()
    K = N = 800
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    n = torch.arange(N)
    k = (7 * n) % K
    assert len(set(k.tolist())) == N                      # 7 and 800 are coprime: every k is some row's
    assert len(set((k % 32).tolist())) == 32              # both nibble positions of all 16 bytes of a lane
    xg = x.to(dev)
    flat = torch.full((N, K // 32), 127, dtype=torch.uint8)
    by_block = (120 + torch.arange(K // 32) % 12).to(torch.uint8).repeat(N, 1)
    assert by_block.min() == 120 and by_block.max() == 131
    for code in range(1, 16):
        codes = torch.zeros(N, K, dtype=torch.uint8)
        codes[n, k] = code
        q = R.pack(codes)
        value = float(R.code_values(torch.tensor([code]))[0])
        for s in (flat, by_block):
            if code == 8:                                 # -0: a sum of zeros of either sign, equal to zero
                assert not ops.decode_linear_fp4(xg, q.to(dev), s.to(dev)).any()
                continue
            factor = torch.ldexp(torch.tensor(value), s[n, k // 32].to(torch.int32) - 127)        # value 2^(s - 127), per row n
            want32 = x[:, k].float() * factor                                                     # <= 10 significant bits: exact
            assert torch.equal(want32.double(), x[:, k].double() * factor.double())
            out = ops.decode_linear_fp4(xg, q.to(dev), s.to(dev))
            bad = (out.cpu().view(torch.int16) != want32.to(torch.bfloat16).view(torch.int16)).nonzero()
            assert bad.numel() == 0, (f"code {code}: {bad.shape[0]} elements differ, first (m, n) = {bad[0].tolist()}: "
                                      f"k = {int(k[bad[0][1]])}")
            out = ops.decode_linear_fp4(xg, q.to(dev), s.to(dev), out_dtype=torch.float32)
            assert torch.equal(out.cpu(), want32), f"code {code}: fp32 store"
    # through the norm-free SwiGLU rows as well: gate row j picks k, up row j picks k + 1 (mod K), both 1.0 under scale 2^0
    cs = torch.zeros(2 * N, K, dtype=torch.uint8)
    cs[n, k] = 2
    cs[N + n, (k + 1) % K] = 2
    out = ops.decode_linear_fp4(xg, R.pack(cs).to(dev), torch.full((2 * N, K // 32), 127, dtype=torch.uint8, device=dev),
                                act="swiglu", out_dtype=torch.float32)
    gate, up = x[:, k].double(), x[:, (k + 1) % K].double()
    ref = gate * torch.sigmoid(gate) * up
    assert float(((out.double().cpu() - ref).abs() / ref.abs().clamp_min(1e-30)).max()) < 1e-5


def _first_n_with_slab(rows, act=None):
    """The smallest N at which this device's plan first picks ``rows``-row slabs."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    per = rows // 2 if act else rows
    cols = (cus - 1) * per + 1                            # the first N' with cus workgroups of `per` columns
    return 2 * cols if act else cols


@pytest.mark.parametrize("rows,K", [(16, 224), (32, 288)])
def test_larger_slabs_inside_the_bound(dev, rows, K):
    """The N at which the plan first picks 16- and 32-row slabs, plus 5: a ragged last workgroup, M = 16 and a residual."""
    ops = _ops()
    N0 = _first_n_with_slab(rows)
    assert ops.decode_linear_fp4_plan(16, N0, K)[0] == rows and ops.decode_linear_fp4_plan(16, N0 - 1, K)[0] == rows // 2
    N = N0 + 5
    assert ops.decode_linear_fp4_plan(16, N, K)[0] == rows and N % rows
    g = torch.Generator().manual_seed(SEED + N)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    q, s = R.quantize((torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    wd = R.dequantize(q, s)
    r = torch.randn(16, (N + 7) // 8 * 8, generator=g).to(torch.bfloat16)             # row stride: a multiple of 8
    ref = x.double() @ wd.t() + r[:, :N].double()
    mag = x.double().abs() @ wd.abs().t() + r[:, :N].double().abs()
    out = ops.decode_linear_fp4(x.to(dev), q.to(dev), s.to(dev), residual=r.to(dev)[:, :N])
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
        check(ops.decode_linear_fp4(g["x"][:M], g["q"][:N], g["s"][:N], norm_weight=g["nw"], eps=EPS), ref, f"norm N={N}")
        out = ops.decode_linear_fp4(g["x"][:M], g["q"][:N], g["s"][:N], norm_weight=g["nw"], eps=EPS, residual=g["res"][:M, :N])
        check(out, ref + d["res"][:M, :N].double(), f"norm + residual N={N}")
        if M > 1:
            assert torch.equal(out[1], g["res"][1, :N])                         # the zero row: finite, exactly the residual
    for inter in sorted({1, 15, slab // 2 + 1, 1024}):
        q = torch.cat([g["q"][:inter], g["q"][UP0:UP0 + inter]], 0)
        # gate and up rows under different scales: the up rows' codes + 1 (doubled: the reference doubles exactly)
        s = torch.cat([g["s"][:inter], g["s"][UP0:UP0 + inter] + 1], 0)
        for norm in (False, True):
            y = d["yn"] if norm else d["y"]
            gate, up = y[:M, :inter], 2 * y[:M, UP0:UP0 + inter]
            ref = gate * torch.sigmoid(gate) * up
            out = ops.decode_linear_fp4(g["x"][:M], q, s, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu")
            assert out.shape == (M, inter)
            check(out, ref, f"swiglu I={inter} norm={norm}")
            if M > 1:
                assert not out[1].any()                                         # the zero row gives silu(0) * 0 = 0
            f32 = ops.decode_linear_fp4(g["x"][:M], q, s, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu",
                                        out_dtype=torch.float32)
            assert torch.equal(f32.to(torch.bfloat16), out)                     # one rounding at the store


def test_swiglu_32_row_slab(dev):
    """The 32-row SwiGLU slab (with the norm: the instantiation that runs one workgroup per CU) at the N that first takes it."""
    ops = _ops()
    K = 224
    N = _first_n_with_slab(32, "swiglu") + 10
    inter = N // 2
    assert ops.decode_linear_fp4_plan(16, N, K, "swiglu")[0] == 32 and inter % 16
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    q, s = R.quantize((torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    s[inter:] -= 1
    wd = R.dequantize(q, s)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    xd = x.double()
    for norm in (False, True):
        xx = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double() if norm else xd
        y = xx @ wd.t()
        ref = y[:, :inter] * torch.sigmoid(y[:, :inter]) * y[:, inter:]
        out = ops.decode_linear_fp4(x.to(dev), q.to(dev), s.to(dev), act="swiglu", norm_weight=nw.to(dev) if norm else None, eps=EPS)
        assert rel_err(out, ref) < TOL["bf16"] and fit_err(out, ref)[0] < 5e-3, f"norm={norm}"
    # and the plain 32-row slab with the norm
    N = _first_n_with_slab(32) + 3
    assert ops.decode_linear_fp4_plan(16, N, K)[0] == 32
    q, s = R.quantize((torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    xx = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double()
    ref = xx @ R.dequantize(q, s).t()
    out = ops.decode_linear_fp4(x.to(dev), q.to(dev), s.to(dev), norm_weight=nw.to(dev), eps=EPS)
    assert rel_err(out, ref) < TOL["bf16"] and fit_err(out, ref)[0] < 5e-3


def test_views_touch_nothing_around_them(dev):
    """x is a column slice of a wider buffer whose other rows and columns are NaN, Wq has 0xFF padding columns and rows, Ws is a
    slice of a wider matrix of code 255 (NaN in e8m0), residual and out are slices of wider buffers; out's surroundings hold a
    sentinel and keep their bits."""
    ops = _ops()
    K, N, M = 288, 30, 3
    d = _data(K)
    nan = float("nan")
    xbuf = torch.full((M + 2, K + 24), nan, dtype=torch.bfloat16)
    xbuf[:M, 8:8 + K] = d["x"][2:2 + M]
    qbuf = torch.full((N + 1, K // 2 + 32), 0xFF, dtype=torch.uint8)
    qbuf[:N, 16:16 + K // 2] = d["q"][:N]
    sbuf = torch.full((N + 2, K // 32 + 5), 255, dtype=torch.uint8)
    sbuf[1:1 + N, 3:3 + K // 32] = d["s"][:N]
    rbuf = torch.full((M + 1, N + 18), nan, dtype=torch.bfloat16)
    rbuf[:M, 16:16 + N] = d["res"][:M, :N]
    xbuf, qbuf, sbuf, rbuf = xbuf.to(dev), qbuf.to(dev), sbuf.to(dev), rbuf.to(dev)
    x, q, s, r = xbuf[:M, 8:8 + K], qbuf[:N, 16:16 + K // 2], sbuf[1:1 + N, 3:3 + K // 32], rbuf[:M, 16:16 + N]
    g = _dev_data(K, dev)
    cx, cq, cs = d["x"][2:2 + M].to(dev), d["q"][:N].to(dev), d["s"][:N].to(dev)
    want = ops.decode_linear_fp4(cx, cq, cs, residual=g["res"][:M, :N])
    assert torch.isfinite(want).all()
    for dt, sentinel in ((torch.bfloat16, -1.5), (torch.float32, -1.5)):
        obuf = torch.full((M + 2, N + 26), sentinel, dtype=dt, device=dev)
        out = obuf[1:1 + M, 8:8 + N]
        got = ops.decode_linear_fp4(x, q, s, residual=r, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.to(torch.bfloat16), want)
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[1:1 + M, 8:8 + N] = False
        assert bool((obuf[mask] == sentinel).all())
    # the norm prologue reads x and the norm weights under the same rules
    a = ops.decode_linear_fp4(x, q, s, norm_weight=g["nw"], eps=EPS)
    b = ops.decode_linear_fp4(cx, cq, cs, norm_weight=g["nw"], eps=EPS)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("K,N", [(4096, 4096), (288, 30)])
def test_same_call_same_bits_and_batch_invariance(dev, K, N):
    ops = _ops()
    g = _dev_data(K, dev)
    q, s = g["q"][:N], g["s"][:N]
    qg = torch.cat([g["q"][:N // 2], g["q"][UP0:UP0 + N // 2]], 0)
    sg = torch.cat([g["s"][:N // 2], g["s"][UP0:UP0 + N // 2]], 0)
    variants = [dict(), dict(residual=True), dict(norm_weight=g["nw"], eps=EPS), dict(out_dtype=torch.float32),
                dict(act="swiglu"), dict(norm_weight=g["nw"], eps=EPS, act="swiglu")]
    for kw in variants:
        def run(rows):
            k2 = dict(kw)
            qq, ss = (qg, sg) if k2.get("act") else (q, s)
            if k2.pop("residual", False):
                k2["residual"] = g["res"][rows, :N]
            return ops.decode_linear_fp4(g["x"][rows], qq, ss, **k2)
        full = run(slice(0, 16))
        assert torch.equal(full, run(slice(0, 16))), f"{kw}: two runs differ"
        for m in (0, 1, 7, 15):                       # row m alone (M = 1) against row m of the M = 16 call: the same bits
            assert torch.equal(run(slice(m, m + 1))[0], full[m]), f"{kw}: row {m} depends on the batch"
        assert torch.equal(run(slice(0, 3)), full[:3])


def test_batch_invariance_across_slabs(dev):
    """The order in which a row's k are summed does not depend on the slab: row m alone, row m of the 16-row call and the same
    row computed as part of shorter weight matrices (which the plan gives 16- and 8-row slabs) agree bit for bit."""
    ops = _ops()
    K = 288
    N = _first_n_with_slab(32) + 9                        # even: the SwiGLU variant takes the same matrix
    n16, n8 = _first_n_with_slab(16) + 8, 1000
    assert [ops.decode_linear_fp4_plan(16, v, K)[0] for v in (N, n16, n8)] == [32, 16, 8]
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16).to(dev)
    q, s = R.quantize((torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    q, s = q.to(dev), s.to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    for kw in (dict(), dict(norm_weight=nw, eps=EPS), dict(norm_weight=nw, eps=EPS, act="swiglu")):
        full = ops.decode_linear_fp4(x, q, s, **kw)
        for m in (0, 9, 15):
            assert torch.equal(ops.decode_linear_fp4(x[m:m + 1], q, s, **kw)[0], full[m]), f"{kw}: row {m}"
        assert torch.equal(ops.decode_linear_fp4(x[:4], q, s, **kw), full[:4])
        if not kw.get("act"):                          # the first rows alone: smaller slabs, the same bits
            for part in (n16, n8):
                assert torch.equal(ops.decode_linear_fp4(x, q[:part], s[:part], **kw), full[:, :part])


def test_quantiser_on_the_gpu_equals_the_cpu_restatement(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    N, K = 67, 4096
    g = torch.Generator().manual_seed(SEED)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * (1 + torch.arange(N)[:, None] % 5) * 2.0 ** (torch.arange(N)[:, None] % 7 * 5 - 15)
    w[5] = 0                                              # a zero row
    w[6, 1:] = 0                                          # a single non-zero
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[7] = 0
    w[7, :7], w[7, 7:14], w[7, 14] = ties * 2.0 ** -5, -ties * 2.0 ** -5, 6 * 2.0 ** -5          # ties under e = -5
    w[7, 32:39], w[7, 39] = ties * 2.0 ** 3, -7 * 2.0 ** 3                                       # amax 7 x 2^3: clamps
    w[8, 64:96] = 2.0 ** -133                             # a block of fp32 subnormals
    for dt in (torch.bfloat16, torch.float32):
        wt = w.to(dt)
        q, s = ops.k_quantize_mxfp4_rows(wt.to(dev))
        assert q.shape == (N, K // 2) and s.shape == (N, K // 32) and q.dtype == s.dtype == torch.uint8
        rq, rs = R.quantize(wt)
        assert torch.equal(s.cpu(), rs), f"{dt}: scale codes differ at {(s.cpu() != rs).nonzero()[:4].tolist()}"
        assert torch.equal(q.cpu(), rq), f"{dt}: nibbles differ at {(q.cpu() != rq).nonzero()[:4].tolist()}"
        assert int(rs.min()) >= 1 and int(rs.max()) <= 254 and not rq[5].any() and bool((rs[5] == 127).all())
        codes = R.unpack(rq)
        assert codes[7, :15].tolist() == [0, 2, 2, 4, 4, 6, 6, 0, 10, 10, 12, 12, 14, 14, 7]
        assert codes[7, 32:40].tolist() == [0, 2, 2, 4, 4, 6, 6, 15] and int(rs[7, 1]) == 127 + 3
    # a frozen bf16 weight through ops.decode_fp4_weight: the same bytes, and operands the kernel takes
    wb = w.to(torch.bfloat16).to(dev)
    q, s = ops.decode_fp4_weight(wb)
    assert torch.equal(q.cpu(), R.quantize(w.to(torch.bfloat16))[0])
    assert ops.decode_linear_fp4_supported(torch.zeros(1, K, dtype=torch.bfloat16, device=dev), q, s)
    # K = 20480 (Yi-34B's down_proj, past the e4m3 quantiser's reach) with 8 rows
    big = (torch.randn(8, 20480, generator=g) * 0.02).to(torch.bfloat16)
    assert ops.decode_linear_fp4_weight_supported(1, big.to(dev)) and not ops.decode_linear_fp8_weight_supported(1, big.to(dev))
    q, s = ops.decode_fp4_weight(big.to(dev))
    rq, rs = R.quantize(big)
    assert torch.equal(q.cpu(), rq) and torch.equal(s.cpu(), rs)
    with pytest.raises(CambrianAmdError):
        ops.decode_fp4_weight(wb.clone().requires_grad_())
    with pytest.raises(CambrianAmdError):
        ops.decode_fp4_weight(wb.float())
    with pytest.raises(CambrianAmdError):
        ops.decode_fp4_weight(wb[:, :48])                 # K % 32


# ---- the decoder layer's decode(..., fp4=True): four fp4 launches + attention against the stock sequence on a twin ----
def _spies(monkeypatch):
    ops = _ops()
    calls = {"fp4": 0, "fp8": 0, "bf16": 0}
    for key, name in (("fp4", "decode_linear_fp4"), ("fp8", "decode_linear_fp8"), ("bf16", "decode_linear")):
        real = getattr(ops, name)

        def counted(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)
    return calls


def _fp4_keys(layer):
    return [(m, k) for m in layer.modules() for k in m.__dict__ if k.endswith("_fp4")]


def _dequantised_twin(layer):
    """A copy of the layer whose matrices are the dequantised ones (every value is exactly a bf16; blocks run along a row, so
    a packed [q; k; v] or [gate; up] has the rows of its parts), without the copies the original has cached."""
    twin = copy.deepcopy(layer)
    with torch.no_grad():
        for mod in twin.modules():
            for k in [k for k in mod.__dict__ if k.startswith("_w")]:
                del mod.__dict__[k]
        for p in twin.parameters():
            if p.dim() == 2:
                p.copy_(R.dequantize(*R.quantize(p.detach().cpu()), dtype=torch.float32).to(p.dtype))
    return twin


def _decode_inputs(dev, dt, hidden, nkv, hd, B):
    from test_decode_linear_fp8_gpu import _decode_inputs as inputs
    return inputs(dev, dt, hidden, nkv, hd, B)


# the small geometries of the e4m3 file, then a layer whose down_proj has K = 20480 > 16384 (Yi-34B's intermediate size; the
# hidden size shrunk to 256: N = 256 and 2 x 20480 rows of K = 256 is as small as a layer with that K gets)
GEOMS = [("llama", 256, 512, 4, 4, 3), ("llama", 256, 512, 4, 2, 3), ("llama", 512, 1024, 4, 1, 3),
         ("phi3", 256, 512, 4, 4, 3), ("phi3", 256, 512, 4, 2, 3), ("phi3", 512, 1024, 4, 1, 3),
         ("llama", 256, 20480, 4, 2, 3)]


@pytest.mark.parametrize("lm,hidden,inter,nh,nkv,B", GEOMS)
def test_layer_decode_fp4_vs_stock_sequence_on_dequantised_twin(dev, monkeypatch, lm, hidden, inter, nh, nkv, B):
    from test_decode_linear_gpu import _make_layer
    ops = _ops()
    hd = hidden // nh
    dt = torch.bfloat16
    layer = _make_layer(dev, dt, lm, hidden, inter, nh, nkv, frozen=True)
    twin = _dequantised_twin(layer)
    calls = _spies(monkeypatch)
    x, kc, vc, mask, cos, sin, t = _decode_inputs(dev, dt, hidden, nkv, hd, B)
    for name in ("CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_FP8"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "1")
    if inter > 16384:                                       # the case the e4m3 mode leaves on bf16
        assert not ops.decode_linear_fp8_weight_supported(B, layer.mlp.down_proj.weight)
    k1, v1 = kc.clone(), vc.clone()
    with torch.no_grad():
        y1 = layer.decode(x, cos, sin, k1, v1, t, mask, fp4=True)
    assert calls == {"fp4": 4, "fp8": 0, "bf16": 0}, f"calls with the mode on: {calls}"
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "0")
    k0, v0 = kc.clone(), vc.clone()
    with torch.no_grad():
        y0 = twin.decode(x, cos, sin, k0, v0, t, mask)
    assert calls == {"fp4": 4, "fp8": 0, "bf16": 0}
    assert y1.shape == y0.shape == (B, 1, hidden) and torch.isfinite(y1).all()
    e = rel_err(y1, y0)
    print(f"{lm} {hidden}/{inter} B={B}: layer out rel err {e:.3g}")
    assert e < TOL["bf16"]
    keep = torch.ones(k1.shape[2], dtype=torch.bool)
    keep[t] = False
    assert torch.equal(v1[:, :, keep], v0[:, :, keep]) and torch.equal(k1[:, :, keep], k0[:, :, keep])
    assert rel_err(v1[:, :, t], v0[:, :, t]) < TOL["bf16"] and rel_err(k1[:, :, t], k0[:, :, t]) < TOL["bf16"]
    # the copies are cached on their owners under keys of their own, and a second step makes none
    assert len(_fp4_keys(layer)) == 4 and not any(k.endswith("_fp8") for m in layer.modules() for k in m.__dict__)
    ptrs = sorted(m.__dict__[k][1][0].data_ptr() for m, k in _fp4_keys(layer))
    with torch.no_grad():
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", "1")
        y2 = layer.decode(x, cos, sin, kc.clone(), vc.clone(), t, mask, fp4=True)
    assert torch.equal(y2, y1)
    assert ptrs == sorted(m.__dict__[k][1][0].data_ptr() for m, k in _fp4_keys(layer))


@pytest.mark.parametrize("lm", ["llama", "phi3"])
@pytest.mark.parametrize("why", ["batch17", "fp32", "trainable"])
def test_layer_decode_fp4_is_not_taken_outside_the_conditions(dev, monkeypatch, lm, why):
    from test_decode_linear_gpu import _make_layer
    dt = torch.float32 if why == "fp32" else torch.bfloat16
    B = 17 if why == "batch17" else 3
    hidden, nh, nkv = 256, 4, 2
    layer = _make_layer(dev, dt, lm, hidden, 2 * hidden, nh, nkv, frozen=why != "trainable")
    calls = _spies(monkeypatch)
    x, kc, vc, mask, cos, sin, t = _decode_inputs(dev, dt, hidden, nkv, hidden // nh, B)
    res = []
    for fp4 in (True, False):
        k1, v1 = kc.clone(), vc.clone()
        with torch.no_grad():
            res.append((layer.decode(x, cos, sin, k1, v1, t, mask, fp4=fp4), k1, v1))
    assert calls == {"fp4": 0, "fp8": 0, "bf16": 0}
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert not _fp4_keys(layer)                            # and no copy was made


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_layer_with_one_refused_weight_makes_no_copy_and_runs_as_without_the_mode(dev, monkeypatch, lm):
    """intermediate = 528: down_proj has K = 528, a multiple of 16 (the e4m3 mode takes the layer) but not of 32.  The other
    three weights are acceptable and come first; none of them may be quantised or kept, the step is the bf16 one bit for bit,
    and the refusal is remembered: the second step asks the predicate nothing."""
    from test_decode_linear_gpu import _make_layer
    ops = _ops()
    dt = torch.bfloat16
    hidden, inter, nh, nkv, B = 256, 528, 4, 2, 3
    layer = _make_layer(dev, dt, lm, hidden, inter, nh, nkv, frozen=True)
    assert ops.decode_linear_fp8_weight_supported(B, layer.mlp.down_proj.weight)
    assert not ops.decode_linear_fp4_weight_supported(B, layer.mlp.down_proj.weight)
    calls = _spies(monkeypatch)
    asked, made = [0], [0]
    real_ok, real_q = ops.decode_linear_fp4_weight_supported, ops.decode_fp4_weight
    monkeypatch.setattr(ops, "decode_linear_fp4_weight_supported", lambda *a, **k: (asked.__setitem__(0, asked[0] + 1), real_ok(*a, **k))[1])
    monkeypatch.setattr(ops, "decode_fp4_weight", lambda *a, **k: (made.__setitem__(0, made[0] + 1), real_q(*a, **k))[1])
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_LINEAR", raising=False)
    x, kc, vc, mask, cos, sin, t = _decode_inputs(dev, dt, hidden, nkv, hidden // nh, B)
    res = []
    for fp4 in (True, True, False):
        k1, v1 = kc.clone(), vc.clone()
        before = asked[0]
        with torch.no_grad():
            res.append((layer.decode(x, cos, sin, k1, v1, t, mask, fp4=fp4), k1, v1))
        res[-1] += (asked[0] - before,)
    assert calls == {"fp4": 0, "fp8": 0, "bf16": 12}, f"{calls}"            # three bf16 five-launch steps
    assert made[0] == 0, "a weight was quantised for a layer that does not take the mode"
    assert res[0][3] >= 1 and res[1][3] == 0 and res[2][3] == 0, f"predicate calls per step: {[r[3] for r in res]}"
    for a, b in ((res[0], res[2]), (res[1], res[2])):
        assert all(torch.equal(p, q) for p, q in zip(a[:3], b[:3]))
    assert not _fp4_keys(layer)


def test_generate_decodes_on_fp4_weights(dev, monkeypatch):
    """With the mode on every decode step of the loop is 4 fp4 calls per layer plus the logits and no bf16 or e4m3
    decode_linear; the first token comes from the bf16 prefill and equals the mode-off run's; the switch works from the config
    and from the environment (which overrides); both modes together raise; the cached copies follow an in-place change of a
    weight."""
    from cambrian_amd.lib import CambrianAmdError
    from test_dynamic_gpu import _eval_batch
    from test_model_gpu import _build
    calls = _spies(monkeypatch)
    new = 4
    dt = torch.bfloat16
    for name in ("CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_STEP"):
        monkeypatch.delenv(name, raising=False)
    model, cfg, towers = _build(dev, dt, monkeypatch, lm="llama", nkv=2)
    model.eval()
    layers = cfg.num_hidden_layers
    ids, att, sizes, images = _eval_batch(dev, dt, towers)
    ids, sizes, images = ids[:1], sizes[1:2], [i[1:2] for i in images]
    kw = dict(images=[i.to(dev, dt) for i in images], image_sizes=sizes, max_new_tokens=new)
    steps = (new - 1) * (4 * layers + 1)

    def run():
        for k in calls:
            calls[k] = 0
        toks = model.generate(ids.to(dev), **kw)
        assert toks.shape == (1, new)
        return toks, (calls["fp4"], calls["fp8"], calls["bf16"])

    off, n_off = run()
    assert n_off == (0, 0, steps), f"mode off: {n_off}"
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "1")
    on, n_on = run()
    assert n_on == (steps, 0, 0), f"CAMBRIAN_AMD_DECODE_FP4=1: {n_on}"
    assert torch.equal(on[:, 0], off[:, 0])                # the first token is the bf16 prefill's
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    with pytest.raises(CambrianAmdError, match="CAMBRIAN_AMD_DECODE_FP8"):
        run()
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8")
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP4")
    model.config.decode_fp4_weights = True
    on2, n_on2 = run()
    assert n_on2 == (steps, 0, 0) and torch.equal(on2, on)  # the config flag; the same copies, the same tokens
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "0")
    assert run()[1] == (0, 0, steps)                       # the environment overrides the config
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP4")

    # the cached copies follow their weights: an in-place change bumps _version and the next step requantises
    head = model.lm_head
    down = model.model.layers[0].mlp.down_proj
    att = model.model.layers[0].self_attn
    q_head, q_down, q_qkv = head.__dict__["_w_fp4"][1], down.__dict__["_w_fp4"][1], att.__dict__["_w_qkv_fp4"][1]
    with torch.no_grad():
        down.weight.mul_(2.0)
        head.weight[0].zero_()
        att.q_proj.weight.mul_(2.0)                        # one part of the packed [q; k; v]
    run()
    q_qkv2, nq = att.__dict__["_w_qkv_fp4"][1], att.q_proj.weight.shape[0]
    live = q_qkv[0].reshape(q_qkv[0].shape[0], -1, 16).any(-1)            # a zero block keeps code 127 when it is doubled
    assert torch.equal(q_qkv2[0], q_qkv[0]) and torch.equal(q_qkv2[1][:nq], q_qkv[1][:nq] + live[:nq].to(torch.uint8))
    assert torch.equal(q_qkv2[1][nq:], q_qkv[1][nq:])
    q_head2, q_down2 = head.__dict__["_w_fp4"][1], down.__dict__["_w_fp4"][1]
    assert q_down2[0] is not q_down[0] and q_head2[0] is not q_head[0]
    assert torch.equal(q_down2[0], q_down[0])              # doubled weights: the same nibbles, every scale code one higher
    assert torch.equal(q_down2[1], q_down[1] + q_down[0].reshape(q_down[0].shape[0], -1, 16).any(-1).to(torch.uint8))
    assert not q_head2[0][0].any() and bool((q_head2[1][0] == 127).all()) and torch.equal(q_head2[0][1:], q_head[0][1:])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_one_call_step_equals_the_per_launch_fp4_loop(dev, monkeypatch, lm, B):
    """``cmb_decode_step`` with ``fp8`` = 2: one step's logits and caches, then generate()'s tokens, equal the per-launch fp4 loop
    bit for bit."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    from test_decode_step_gpu import _lm, _prompt
    ops = _ops()
    for name in ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_LINEAR",
                 "CAMBRIAN_AMD_DECODE_ATTN"):
        monkeypatch.delenv(name, raising=False)
    model = _lm(dev, lm)
    cfg = model.config
    a0 = model.model.layers[0].self_attn
    nkv, hd, H, V, t = a0.nkv, a0.hd, cfg.hidden_size, cfg.vocab_size, 36
    gen = torch.Generator().manual_seed(11 * B + t)
    Lmax = t + 5
    caches = [(torch.randn(B, nkv, Lmax, hd, generator=gen).to(torch.bfloat16).to(dev),
               torch.randn(B, nkv, Lmax, hd, generator=gen).to(torch.bfloat16).to(dev)) for _ in model.model.layers]
    x = torch.randn(B, 1, H, generator=gen).to(torch.bfloat16).to(dev)
    mask = (torch.rand(B, Lmax, generator=gen) > 0.15).to(dev)
    cos, sin = ops.rope_table(torch.randint(0, t + 1, (B, 1), generator=gen).to(dev), hd, float(cfg.rope_theta))
    calls = _spies(monkeypatch)
    n_layers = len(model.model.layers)
    ref_caches = [(k.clone(), v.clone()) for k, v in caches]
    with torch.no_grad():
        h = x
        for layer, (kc, vc) in zip(model.model.layers, ref_caches):
            h = layer.decode(h, cos, sin, kc, vc, t, mask, fp4=True)
        want = CL._decode_logits(model, h, fp4=True)
    assert calls == {"fp4": 4 * n_layers + 1, "fp8": 0, "bf16": 0}, calls
    got_caches = [(k.clone(), v.clone()) for k, v in caches]
    with torch.no_grad():
        plan = CL.DecodeStepPlan.build(model, B, got_caches, Lmax - 1, False, fp4=True)
        assert plan is not None and plan.desc.fp8 == 2
        got = plan.step(x[:, 0], cos, sin, t, mask)
    torch.cuda.synchronize()
    assert calls == {"fp4": 4 * n_layers + 1, "fp8": 0, "bf16": 0}, calls            # the step calls the library, not ops
    assert got.shape == want.shape == (B, V) and torch.isfinite(got).all()
    assert torch.equal(got, want)
    for (k1, v1), (k0, v0) in zip(got_caches, ref_caches):
        assert torch.equal(k1, k0) and torch.equal(v1, v0)
    # generate(): tokens of the fused loop against the per-launch loop, the mode on in both
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "1")
    ids, att = _prompt(dev, B)
    new = 12
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "0")
    for k in calls:
        calls[k] = 0
    off = model.generate(ids, attention_mask=att, max_new_tokens=new)
    assert calls == {"fp4": (new - 1) * (4 * n_layers + 1), "fp8": 0, "bf16": 0}, calls
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "1")
    for k in calls:
        calls[k] = 0
    on = model.generate(ids, attention_mask=att, max_new_tokens=new)
    assert calls == {"fp4": 0, "fp8": 0, "bf16": 0}, calls
    assert torch.equal(on, off), (on.tolist(), off.tolist())
    assert len(set(off[0].tolist())) > 1, "a constant sequence would not show a wrong step"


def test_a_refused_layer_keeps_the_one_call_step_off(dev, monkeypatch):
    """intermediate = 528 under the mode: no plan, and generate() gives the bf16 loop's tokens."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    from test_decode_step_gpu import _lm, _prompt
    for name in ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_LINEAR"):
        monkeypatch.delenv(name, raising=False)
    model = _lm(dev, "llama", inter=528)
    ids, att = _prompt(dev, 1)
    off = model.generate(ids, attention_mask=att, max_new_tokens=6)
    calls = _spies(monkeypatch)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "1")
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "1")
    on = model.generate(ids, attention_mask=att, max_new_tokens=6)
    n_layers = len(model.model.layers)
    # the layers run bf16; the lm_head (K = 256) is taken by the mode on its own, as in the e4m3 mode
    assert calls["bf16"] == 5 * 4 * n_layers and calls["fp8"] == 0 and calls["fp4"] == 5, calls
    assert torch.equal(on[:, 0], off[:, 0])
    assert not any(_fp4_keys(layer) for layer in model.model.layers)


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_beam_search_fused_equals_the_torch_selection_loop_with_the_mode_on(dev, monkeypatch, lm):
    from test_decode_step_gpu import _lm, _prompt
    for name in ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_SAMPLE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_FP4", "1")
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    model = _lm(dev, lm)
    calls = _spies(monkeypatch)
    ids, att = _prompt(dev, 2)
    kw = dict(attention_mask=att, num_beams=3, max_new_tokens=8)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "0")
    host = model.generate(ids, **kw)
    n_layers = len(model.model.layers)
    assert calls["fp4"] > 0 and calls["fp4"] % (4 * n_layers + 1) == 0 and calls["fp8"] == calls["bf16"] == 0, calls
    for k in calls:
        calls[k] = 0
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "1")
    fused = model.generate(ids, **kw)
    assert calls == {"fp4": 0, "fp8": 0, "bf16": 0}, calls
    assert torch.equal(fused, host), (fused.tolist(), host.tolist())


def test_bad_operands_raise(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(32, 32, dtype=torch.uint8, device=dev)
    s = torch.full((32, 2), 127, dtype=torch.uint8, device=dev)
    assert ops.decode_linear_fp4(x, q, s).shape == (2, 32)
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_linear_fp4(x.clone().requires_grad_(), q, s)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp4(x, q, s, act="swiglu", residual=torch.zeros(2, 16, dtype=torch.bfloat16, device=dev))
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp4(torch.zeros(17, 64, dtype=torch.bfloat16, device=dev), q, s)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp4(x, q.to(torch.int8), s)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp4(x, q, s[:31])
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp4(x, q, s[:, :1])
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_fp4(x, q, s.float())
    with pytest.raises(CambrianAmdError):                  # K = 48: a multiple of 16 that the e4m3 kernel takes, not this one
        ops.decode_linear_fp4(x[:, :48], q[:, :24], s)
