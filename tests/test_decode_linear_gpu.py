"""`-m gpu`: the decode-step linear — ``cmb_decode_linear`` (decode_linear.hip) through ``ops.decode_linear``, the decoder
layers' five-launch ``decode`` and the generate loop.

Kernel tests compare with float64 on the CPU computed from the inputs AS STORED (seeded randn rounded to bf16, W scaled by
K^-0.5).  One weight matrix, one 16-row x and their float64 products are made per K and shared by every case of that K.

Plain epilogue, elementwise:  |out - ref| <= 2^-8 |ref| + (K + 1) 2^-24 (sum_k |x_k w_k| + |r|)
— one bf16 rounding of the result (2^-23 |ref| for an fp32 store) plus the worst-case error of an fp32 sum of K + 1 terms in
any order; derived, not tuned.  ``_cpu_fp32_inside_bound`` evaluates the same inputs with a plain fp32 torch.matmul rounded
to bf16 on the CPU: the seeds below are ones for which that evaluation stays inside the bound too, and the test re-checks it.
Norm prologue / SwiGLU: ``rel_err < TOL["bf16"]`` AND a least-squares slope within 5e-3 against the float64 un-fused formula,
on every case — the one-number ones (M = 1 with N = 1 or I = 1) included, where the slope is that number's relative error, an
elementwise bound of 5e-3.  One bf16 rounding is at most 2^-8 = 3.9e-3 of the result, so such a case leaves 1.1e-3 for
everything before the store: the kernel meets it because it never rounds the normalised row (x[k] norm_w[k] goes through the
matrix unit exactly, as two bf16 operands) and sums in fp32.  An evaluation that does round that row to bf16 — the un-fused
sequence, on the CPU — misses them on nine to fourteen of the few-number cases at each of the seeds scanned (0 - 5, 31, 32).

The kernel has ONE instantiation in M (x is the 16-wide MFMA operand whatever M is), so batch invariance is bit-equality."""
import functools

import pytest
import torch

from conftest import TOL, fit_err, rel_err

pytestmark = pytest.mark.gpu

KS = [8, 64, 72, 264, 4096, 14336]      # fewer chunks than waves, one step, a ragged one, two steps + ragged, the real sizes
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
    """Shared per K, never modified: bf16 x [16, K] (row 1 is zero), W [NMAX, K], norm weights, residual, and the float64
    products x W^T, |x| |W|^T and RMSNorm(x) W^T."""
    g = torch.Generator().manual_seed(SEED + K)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    x[1] = 0
    w = (torch.randn(NMAX, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    res = torch.randn(16, NMAX, generator=g).to(torch.bfloat16)
    xd, wd = x.double(), w.double()
    y = xd @ wd.t()
    ya = xd.abs() @ wd.abs().t()
    xn = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double()
    yn = xn @ wd.t()
    return dict(x=x, w=w, nw=nw, res=res, y=y, ya=ya, yn=yn)


@functools.lru_cache(maxsize=None)
def _dev_data(K, dev):
    d = _data(K)
    return {k: d[k].to(dev) for k in ("x", "w", "nw", "res")}


def _bound(ref, mag, K, f32):
    return (2.0 ** -23 if f32 else 2.0 ** -8) * ref.abs() + (K + 1) * 2.0 ** -24 * mag


def _cpu_fp32_inside_bound(d, K, M, N):
    y32 = (d["x"][:M].float() @ d["w"][:N].float().t()).to(torch.bfloat16).double()
    return bool(((y32 - d["y"][:M, :N]).abs() <= _bound(d["y"][:M, :N], d["ya"][:M, :N], K, False)).all())


def _slab(K, act=None):
    return _ops().decode_linear_plan(1, 4096, K, act)[0]


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
                out = ops.decode_linear(g["x"][:M], g["w"][:N], residual=g["res"][:M, :N] if use_res else None,
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
                if M > 1 and not f32:                                       # the zero row of x: exactly the residual, or 0
                    assert torch.equal(out[1], g["res"][1, :N]) if use_res else not out[1].any()


@pytest.mark.parametrize("N,K,rows", [(8200, 72, 16), (16390, 264, 32)])
def test_larger_slabs_inside_the_bound(dev, N, K, rows):
    """The 16- and 32-row instantiations (N >= 2 x 2 x CUs x 8), ragged last workgroup, M = 16 and a residual."""
    ops = _ops()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert ops.decode_linear_plan(16, N, K)[0] == ops.decode_linear_plan(16, N, K, None, cus)[0]
    if cus == 256:
        assert ops.decode_linear_plan(16, N, K)[0] == rows
    g = torch.Generator().manual_seed(SEED + N)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    r = torch.randn(16, (N + 7) // 8 * 8, generator=g).to(torch.bfloat16)             # row stride: a multiple of 8
    ref = x.double() @ w.double().t() + r[:, :N].double()
    mag = x.double().abs() @ w.double().abs().t() + r[:, :N].double().abs()
    out = ops.decode_linear(x.to(dev), w.to(dev), residual=r.to(dev)[:, :N])
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
        check(ops.decode_linear(g["x"][:M], g["w"][:N], norm_weight=g["nw"], eps=EPS), ref, f"norm N={N}")
        out = ops.decode_linear(g["x"][:M], g["w"][:N], norm_weight=g["nw"], eps=EPS, residual=g["res"][:M, :N])
        check(out, ref + d["res"][:M, :N].double(), f"norm + residual N={N}")
        if M > 1:
            assert torch.equal(out[1], g["res"][1, :N])                         # the zero row: finite, exactly the residual
    for inter in sorted({1, 15, slab // 2 + 1, 1024}):
        w = torch.cat([g["w"][:inter], g["w"][UP0:UP0 + inter]], 0)
        for norm in (False, True):
            y = d["yn"] if norm else d["y"]
            gate, up = y[:M, :inter], y[:M, UP0:UP0 + inter]
            ref = gate * torch.sigmoid(gate) * up
            out = ops.decode_linear(g["x"][:M], w, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu")
            assert out.shape == (M, inter)
            check(out, ref, f"swiglu I={inter} norm={norm}")
            if M > 1:
                assert not out[1].any()                                         # the zero row gives silu(0) * 0 = 0
            f32 = ops.decode_linear(g["x"][:M], w, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu",
                                    out_dtype=torch.float32)
            assert torch.equal(f32.to(torch.bfloat16), out)                     # one rounding at the store


def test_swiglu_32_row_slab(dev):
    ops = _ops()
    inter, K = 8200, 72
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(2 * inter, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    y = x.double() @ w.double().t()
    ref = y[:, :inter] * torch.sigmoid(y[:, :inter]) * y[:, inter:]
    out = ops.decode_linear(x.to(dev), w.to(dev), act="swiglu")
    assert rel_err(out, ref) < TOL["bf16"] and fit_err(out, ref)[0] < 5e-3


def test_views_touch_nothing_around_them(dev):
    """x is a column slice of a wider buffer whose other rows and columns are NaN, W has NaN padding columns, residual and out
    are slices of wider buffers; out's surroundings hold a sentinel and keep their bits."""
    ops = _ops()
    K, N, M = 264, 30, 3
    d = _data(K)
    nan = float("nan")
    xbuf = torch.full((M + 2, K + 24), nan, dtype=torch.bfloat16)
    xbuf[:M, 8:8 + K] = d["x"][2:2 + M]
    wbuf = torch.full((N + 1, K + 16), nan, dtype=torch.bfloat16)
    wbuf[:N, :K] = d["w"][:N]
    rbuf = torch.full((M + 1, N + 18), nan, dtype=torch.bfloat16)
    rbuf[:M, 16:16 + N] = d["res"][:M, :N]
    xbuf, wbuf, rbuf = xbuf.to(dev), wbuf.to(dev), rbuf.to(dev)
    x, w, r = xbuf[:M, 8:8 + K], wbuf[:N, :K], rbuf[:M, 16:16 + N]
    want = ops.decode_linear(d["x"][2:2 + M].to(dev), d["w"][:N].to(dev), residual=_dev_data(K, dev)["res"][:M, :N])
    assert torch.isfinite(want).all()
    for dt, sentinel in ((torch.bfloat16, -1.5), (torch.float32, -1.5)):
        obuf = torch.full((M + 2, N + 26), sentinel, dtype=dt, device=dev)
        out = obuf[1:1 + M, 8:8 + N]
        got = ops.decode_linear(x, w, residual=r, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.to(torch.bfloat16), want)
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[1:1 + M, 8:8 + N] = False
        assert bool((obuf[mask] == sentinel).all())
    # the norm prologue reads x and the norm weights under the same rules
    a = ops.decode_linear(x, w, norm_weight=_dev_data(K, dev)["nw"], eps=EPS)
    b = ops.decode_linear(d["x"][2:2 + M].to(dev), d["w"][:N].to(dev), norm_weight=_dev_data(K, dev)["nw"], eps=EPS)
    assert torch.equal(a, b)


@pytest.mark.parametrize("K,N", [(4096, 4096), (264, 30)])
def test_same_call_same_bits_and_batch_invariance(dev, K, N):
    ops = _ops()
    g = _dev_data(K, dev)
    w, wg = g["w"][:N], torch.cat([g["w"][:N // 2], g["w"][UP0:UP0 + N // 2]], 0)
    variants = [dict(), dict(residual=True), dict(norm_weight=g["nw"], eps=EPS), dict(out_dtype=torch.float32),
                dict(norm_weight=g["nw"], eps=EPS, act="swiglu")]
    for kw in variants:
        def run(rows):
            k2 = dict(kw)
            ww = wg if k2.get("act") else w
            if k2.pop("residual", False):
                k2["residual"] = g["res"][rows, :N]
            return ops.decode_linear(g["x"][rows], ww, **k2)
        full = run(slice(0, 16))
        assert torch.equal(full, run(slice(0, 16))), f"{kw}: two runs differ"
        for m in (0, 1, 7, 15):                       # row m alone (M = 1) against row m of the M = 16 call: the same bits
            assert torch.equal(run(slice(m, m + 1))[0], full[m]), f"{kw}: row {m} depends on the batch"
        assert torch.equal(run(slice(0, 3)), full[:3])


def test_batch_invariance_across_slabs(dev):
    """The plan takes larger slabs above 4 rows of x; the order in which a row's k are summed does not depend on the slab, so
    row m alone and row m of the 16-row call still agree bit for bit."""
    ops = _ops()
    N, K = 6200, 72
    if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        assert ops.decode_linear_plan(1, N, K)[0] == 8 and ops.decode_linear_plan(16, N, K)[0] == 16
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    for kw in (dict(), dict(norm_weight=nw, eps=EPS), dict(norm_weight=nw, eps=EPS, act="swiglu")):
        full = ops.decode_linear(x, w, **kw)
        for m in (0, 9, 15):
            assert torch.equal(ops.decode_linear(x[m:m + 1], w, **kw)[0], full[m]), f"{kw}: row {m}"
        assert torch.equal(ops.decode_linear(x[:4], w, **kw), full[:4])


# ---- the decoder layer's decode(): five launches against the stock sequence ----
def _make_layer(dev, dt, lm, hidden, inter, nh, nkv, frozen):
    from cambrian_amd.model.language_model import cambrian_llama as CL, cambrian_phi3 as CP
    from test_decode_attn_gpu import THETA
    mod = CP if lm == "phi3" else CL
    cfg = mod.CambrianConfig(vocab_size=64, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=1,
                             num_attention_heads=nh, num_key_value_heads=nkv, rms_norm_eps=1e-5, rope_theta=THETA,
                             max_position_embeddings=256)
    torch.manual_seed(1)
    layer = (CP.Phi3DecoderLayer if lm == "phi3" else CL.LlamaDecoderLayer)(cfg, dev, dt)
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return layer.requires_grad_(not frozen)


def _spy(monkeypatch):
    ops = _ops()
    calls = [0]
    real = ops.decode_linear

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "decode_linear", counted)
    return calls


def _decode_ab(dev, dt, layer, hidden, nkv, hd, B, monkeypatch, calls):
    """layer.decode with CAMBRIAN_AMD_DECODE_LINEAR at 1 and at 0 from identical caches -> [(y, kcache, vcache, calls)] * 2"""
    from test_decode_attn_gpu import TAIL, THETA, _masks
    ops = _ops()
    n = 37
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 1, hidden, generator=g).to(dt).to(dev)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    mask = _masks(B, n)[1][1].to(dev)
    cos, sin = ops.rope_table(torch.randint(20, 37, (B, 1), generator=g).to(dev), hd, THETA)
    res = []
    for env in ("1", "0"):
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", env)
        k1, v1 = kc.clone(), vc.clone()
        before = calls[0]
        with torch.no_grad():
            y = layer.decode(x, cos, sin, k1, v1, n - 1, mask)
        res.append((y, k1, v1, calls[0] - before))
    return res, n - 1


GEOMS = [("llama", 256, 512, 4, 4, 3), ("llama", 256, 512, 4, 2, 3), ("llama", 512, 1024, 4, 1, 3),
         ("phi3", 256, 512, 4, 4, 3), ("phi3", 256, 512, 4, 2, 3), ("phi3", 512, 1024, 4, 1, 3),
         ("llama", 4096, 14336, 32, 8, 1), ("llama", 4096, 14336, 32, 8, 16)]


@pytest.mark.parametrize("lm,hidden,inter,nh,nkv,B", GEOMS)
def test_layer_decode_five_launches_vs_stock_sequence(dev, monkeypatch, lm, hidden, inter, nh, nkv, B):
    hd = hidden // nh
    dt = torch.bfloat16
    layer = _make_layer(dev, dt, lm, hidden, inter, nh, nkv, frozen=True)
    calls = _spy(monkeypatch)
    ((y1, k1, v1, n1), (y0, k0, v0, n0)), t = _decode_ab(dev, dt, layer, hidden, nkv, hd, B, monkeypatch, calls)
    assert (n1, n0) == (4, 0), f"decode_linear calls: {n1} with the switch at 1, {n0} at 0"
    assert y1.shape == y0.shape == (B, 1, hidden) and torch.isfinite(y1).all()
    e = rel_err(y1, y0)
    print(f"{lm} {hidden}/{inter} B={B}: layer out rel err {e:.3g}")
    assert e < TOL["bf16"]
    keep = torch.ones(k1.shape[2], dtype=torch.bool)
    keep[t] = False
    assert torch.equal(v1[:, :, keep], v0[:, :, keep]) and torch.equal(k1[:, :, keep], k0[:, :, keep])
    assert rel_err(v1[:, :, t], v0[:, :, t]) < TOL["bf16"] and rel_err(k1[:, :, t], k0[:, :, t]) < TOL["bf16"]


@pytest.mark.parametrize("lm", ["llama", "phi3"])
@pytest.mark.parametrize("why", ["batch17", "fp32", "trainable"])
def test_layer_decode_keeps_the_stock_sequence_outside_the_conditions(dev, monkeypatch, lm, why):
    dt = torch.float32 if why == "fp32" else torch.bfloat16
    B = 17 if why == "batch17" else 3
    hidden, nh, nkv = 256, 4, 2
    layer = _make_layer(dev, dt, lm, hidden, 2 * hidden, nh, nkv, frozen=why != "trainable")
    calls = _spy(monkeypatch)
    ((y1, k1, v1, n1), (y0, k0, v0, n0)), _ = _decode_ab(dev, dt, layer, hidden, nkv, hidden // nh, B, monkeypatch, calls)
    assert (n1, n0) == (0, 0)
    assert torch.equal(y1, y0) and torch.equal(k1, k0) and torch.equal(v1, v0)


def test_generate_decodes_on_the_kernel(dev, monkeypatch):
    """bf16: every decode step of the loop is 4 calls per layer plus the logits; fp32: the path is not taken and the tokens of
    the two switch positions are equal."""
    from test_dynamic_gpu import _eval_batch
    from test_model_gpu import _build
    calls = _spy(monkeypatch)
    new = 4
    toks = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        model, cfg, towers = _build(dev, dt, monkeypatch, lm="llama", nkv=2)
        model.eval()
        layers = cfg.num_hidden_layers
        ids, att, sizes, images = _eval_batch(dev, dt, towers)
        ids, sizes, images = ids[:1], sizes[1:2], [i[1:2] for i in images]
        kw = dict(images=[i.to(dev, dt) for i in images], image_sizes=sizes, max_new_tokens=new)
        for env in ("1", "0"):
            monkeypatch.setenv("CAMBRIAN_AMD_DECODE_LINEAR", env)
            calls[0] = 0
            toks[name, env] = model.generate(ids.to(dev), **kw)
            assert toks[name, env].shape == (1, new)
            want = (new - 1) * (4 * layers + 1) if (name, env) == ("bf16", "1") else 0
            assert calls[0] == want, f"{name} CAMBRIAN_AMD_DECODE_LINEAR={env}: {calls[0]} calls, expected {want}"
    assert torch.equal(toks["fp32", "1"], toks["fp32", "0"])


def test_requires_grad_inputs_raise(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(32, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_linear(x, w.clone().requires_grad_())
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_linear(x.clone().requires_grad_(), w)
    with torch.no_grad():
        assert ops.decode_linear(x, w.clone().requires_grad_()).shape == (2, 32)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear(x, w, act="swiglu", residual=torch.zeros(2, 16, dtype=torch.bfloat16, device=dev))
    with pytest.raises(CambrianAmdError):
        ops.decode_linear(torch.zeros(17, 64, dtype=torch.bfloat16, device=dev), w)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear(x.float(), w.float())
