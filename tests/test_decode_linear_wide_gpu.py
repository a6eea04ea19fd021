"""`-m gpu`: the wide decode-step linear — ``cmb_decode_linear_wide`` (decode_linear_wide.hip) through
``ops.decode_linear_wide``, the decoder layers' five-launch ``decode`` at 17-64 rows and the generate loop behind the wide
switch.  The scheme is tests/test_decode_linear_gpu.py's.

Kernel tests compare with float64 on the CPU computed from the inputs AS STORED (seeded randn rounded to bf16, W scaled by
K^-0.5).  One weight matrix, one 64-row x (row 1 is zero) and their float64 products are made per K and shared by every case
of that K.

Plain epilogue, elementwise:  |out - ref| <= 2^-8 |ref| + (K + 1) 2^-24 (sum_k |x_k w_k| + |r|)
— one bf16 rounding of the result (2^-23 |ref| for an fp32 store) plus the worst-case error of an fp32 sum of K + 1 terms in
any order; derived, not tuned.  ``_cpu_fp32_inside_bound`` evaluates the same inputs with a plain fp32 torch.matmul rounded
to bf16 on the CPU and the test re-asserts that it stays inside the bound for this seed.
Norm prologue / SwiGLU: ``rel_err < TOL["bf16"]`` AND a least-squares slope within 5e-3 against the float64 un-fused formula.

The kernel has one instantiation per number of 16-row blocks of x; the order of a row's sum is the same in all of them, so
batch invariance is bit-equality: rows [:m] of the 64-row call against the m-row call, across 1, 2 and 3 blocks."""
import functools

import pytest
import torch

from conftest import TOL, fit_err, rel_err

pytestmark = pytest.mark.gpu

KS = [8, 64, 72, 264, 4096, 14336]      # fewer chunks than waves, one step, a ragged one, two steps + ragged, the real sizes
MS = [17, 32, 33, 48, 49, 64]
ROWS = 64
NMAX = 4104                             # rows of the shared weight matrix (>= 4096 and 2048 + 1024 + slab)
UP0 = 2048                              # first "up" row the SwiGLU cases take from the shared matrix
EPS = 1e-5
SEED = 31
ENV = ("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8",
       "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_KV_FP8", "CAMBRIAN_AMD_DECODE_SAMPLE",
       "CAMBRIAN_AMD_DECODE_BEAM")


def _ops():
    from cambrian_amd import ops
    return ops


@pytest.fixture()
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@functools.lru_cache(maxsize=None)
def _data(K):
    """Shared per K, never modified: bf16 x [64, K] (row 1 is zero), W [NMAX, K], norm weights, residual, and the float64
    products x W^T, |x| |W|^T and RMSNorm(x) W^T."""
    g = torch.Generator().manual_seed(SEED + K)
    x = torch.randn(ROWS, K, generator=g).to(torch.bfloat16)
    x[1] = 0
    w = (torch.randn(NMAX, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    res = torch.randn(ROWS, NMAX, generator=g).to(torch.bfloat16)
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
    return _ops().decode_linear_wide_plan(ROWS, 4096, K, act)[0]


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
                out = ops.decode_linear_wide(g["x"][:M], g["w"][:N], residual=g["res"][:M, :N] if use_res else None,
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
                if not f32:                                                 # the zero row of x: exactly the residual, or 0
                    assert torch.equal(out[1], g["res"][1, :N]) if use_res else not out[1].any()


@pytest.mark.parametrize("N,K,rows", [(4100, 264, 16), (8200, 72, 32)])
def test_every_slab_size_with_a_ragged_last_workgroup(dev, N, K, rows):
    """The 16- and the 32-row slab (N >= 32 x CUs), the last workgroup ragged, M = 64 and 33 and a residual."""
    ops = _ops()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert ops.decode_linear_wide_plan(64, N, K) == ops.decode_linear_wide_plan(64, N, K, None, cus)
    if cus == 256:
        assert ops.decode_linear_wide_plan(64, N, K)[0] == rows
    g = torch.Generator().manual_seed(SEED + N)
    x = torch.randn(ROWS, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    r = torch.randn(ROWS, (N + 7) // 8 * 8, generator=g).to(torch.bfloat16)           # row stride: a multiple of 8
    ref = x.double() @ w.double().t() + r[:, :N].double()
    mag = x.double().abs() @ w.double().abs().t() + r[:, :N].double().abs()
    xg, wg, rg = x.to(dev), w.to(dev), r.to(dev)
    for M in (64, 33):
        out = ops.decode_linear_wide(xg[:M], wg, residual=rg[:M, :N])
        worst = float(((out.double().cpu() - ref[:M]).abs() / _bound(ref[:M], mag[:M], K, False)).max())
        print(f"N={N} K={K} M={M}: max err / bound {worst:.3g}")
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
        check(ops.decode_linear_wide(g["x"][:M], g["w"][:N], norm_weight=g["nw"], eps=EPS), ref, f"norm N={N}")
        out = ops.decode_linear_wide(g["x"][:M], g["w"][:N], norm_weight=g["nw"], eps=EPS, residual=g["res"][:M, :N])
        check(out, ref + d["res"][:M, :N].double(), f"norm + residual N={N}")
        assert torch.equal(out[1], g["res"][1, :N])                             # the zero row: finite, exactly the residual
    for inter in sorted({1, 15, slab // 2 - 1, slab // 2, slab // 2 + 1, 1024}):
        w = torch.cat([g["w"][:inter], g["w"][UP0:UP0 + inter]], 0)
        for norm in (False, True):
            y = d["yn"] if norm else d["y"]
            gate, up = y[:M, :inter], y[:M, UP0:UP0 + inter]
            ref = gate * torch.sigmoid(gate) * up
            out = ops.decode_linear_wide(g["x"][:M], w, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu")
            assert out.shape == (M, inter)
            check(out, ref, f"swiglu I={inter} norm={norm}")
            assert not out[1].any()                                             # the zero row gives silu(0) * 0 = 0
            f32 = ops.decode_linear_wide(g["x"][:M], w, norm_weight=g["nw"] if norm else None, eps=EPS, act="swiglu",
                                         out_dtype=torch.float32)
            assert torch.equal(f32.to(torch.bfloat16), out)                     # one rounding at the store


def test_swiglu_32_row_slab(dev):
    """I >= 16 x CUs: 16 gate and 16 up rows per workgroup, the last workgroup ragged; 64 and 49 rows, with the norm."""
    ops = _ops()
    inter, K = 4100, 72
    if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        assert ops.decode_linear_wide_plan(64, 2 * inter, K, "swiglu")[0] == 32
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(ROWS, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(2 * inter, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    xd = x.double()
    for norm in (False, True):
        xn = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double() if norm else xd
        y = xn @ w.double().t()
        ref = y[:, :inter] * torch.sigmoid(y[:, :inter]) * y[:, inter:]
        for M in (64, 49):
            out = ops.decode_linear_wide(x[:M].to(dev), w.to(dev), norm_weight=nw.to(dev) if norm else None, eps=EPS, act="swiglu")
            assert out.shape == (M, inter)
            assert rel_err(out, ref[:M]) < TOL["bf16"] and fit_err(out, ref[:M])[0] < 5e-3


def test_views_touch_nothing_around_them(dev):
    """x is a column slice of a wider buffer whose other rows and columns are NaN, W has NaN padding columns, residual and out
    are slices of wider buffers; out's surroundings hold a sentinel and keep their bits.  A misaligned pointer raises."""
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    K, N, M = 264, 30, 35
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
    want = ops.decode_linear_wide(d["x"][2:2 + M].to(dev), d["w"][:N].to(dev), residual=_dev_data(K, dev)["res"][:M, :N])
    assert torch.isfinite(want).all()
    for dt, sentinel in ((torch.bfloat16, -1.5), (torch.float32, -1.5)):
        obuf = torch.full((M + 2, N + 26), sentinel, dtype=dt, device=dev)
        out = obuf[1:1 + M, 8:8 + N]
        got = ops.decode_linear_wide(x, w, residual=r, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.to(torch.bfloat16), want)
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[1:1 + M, 8:8 + N] = False
        assert bool((obuf[mask] == sentinel).all())
    # the norm prologue reads x and the norm weights under the same rules
    a = ops.decode_linear_wide(x, w, norm_weight=_dev_data(K, dev)["nw"], eps=EPS)
    b = ops.decode_linear_wide(d["x"][2:2 + M].to(dev), d["w"][:N].to(dev), norm_weight=_dev_data(K, dev)["nw"], eps=EPS)
    assert torch.equal(a, b)
    with pytest.raises(CambrianAmdError):                                       # x starts 8 bytes off a 16-byte boundary
        ops.decode_linear_wide(xbuf[:M, 4:4 + K], w)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_wide(x, w, out=torch.empty(M, N + 6, dtype=torch.bfloat16, device=dev)[:, 4:4 + N])


@pytest.mark.parametrize("K,N", [(4096, 4096), (264, 30), (72, 8200)])
def test_same_call_same_bits_and_row_invariance(dev, K, N):
    """Two calls give the same bits; rows [:m] of the 64-row call are the m-row call's, for m in 1, 2 and 3 row blocks and on
    every epilogue kind; a row alone (M = 1) has the bits it has inside the batch.  (72, 8200) runs on 32-row slabs."""
    ops = _ops()
    if K == 72:
        gen = torch.Generator().manual_seed(SEED + N)
        g = dict(x=torch.randn(ROWS, K, generator=gen).to(torch.bfloat16).to(dev),
                 w=(torch.randn(N, K, generator=gen) * K ** -0.5).to(torch.bfloat16).to(dev),
                 nw=(1 + 0.1 * torch.randn(K, generator=gen)).to(torch.bfloat16).to(dev),
                 res=torch.randn(ROWS, N, generator=gen).to(torch.bfloat16).to(dev))
        w = wg = g["w"]
    else:
        g = _dev_data(K, dev)
        w, wg = g["w"][:N], torch.cat([g["w"][:N // 2], g["w"][UP0:UP0 + N // 2]], 0)
    variants = [dict(), dict(residual=True), dict(norm_weight=g["nw"], eps=EPS), dict(out_dtype=torch.float32),
                dict(act="swiglu"), dict(norm_weight=g["nw"], eps=EPS, act="swiglu")]
    for kw in variants:
        def run(rows):
            k2 = dict(kw)
            ww = wg if k2.get("act") else w
            if k2.pop("residual", False):
                k2["residual"] = g["res"][rows, :N]
            return ops.decode_linear_wide(g["x"][rows], ww, **k2)
        full = run(slice(0, ROWS))
        assert torch.equal(full, run(slice(0, ROWS))), f"{kw}: two runs differ"
        for m in (1, 16, 17, 33):
            assert torch.equal(run(slice(0, m)), full[:m]), f"{kw}: rows [:{m}] depend on M"
        for m in (0, 20, 63):                         # row m alone (M = 1) against row m of the 64-row call
            assert torch.equal(run(slice(m, m + 1))[0], full[m]), f"{kw}: row {m} depends on the batch"


def test_requires_grad_inputs_and_bad_shapes_raise(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    x = torch.zeros(40, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(32, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_linear_wide(x, w.clone().requires_grad_())
    with torch.no_grad():
        assert ops.decode_linear_wide(x, w.clone().requires_grad_()).shape == (40, 32)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_wide(x, w, act="swiglu", residual=torch.zeros(40, 16, dtype=torch.bfloat16, device=dev))
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_wide(torch.zeros(65, 64, dtype=torch.bfloat16, device=dev), w)
    with pytest.raises(CambrianAmdError):
        ops.decode_linear_wide(x.float(), w.float())


# ---- the decoder layer's decode() at 40 rows: five launches on the wide kernel against the stock sequence ----
def _spy(monkeypatch):
    ops = _ops()
    calls = {"wide": 0, "narrow": 0}

    def wrap(name, key):
        real = getattr(ops, name)

        def counted(*a, **kw):
            calls[key] += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)

    wrap("decode_linear_wide", "wide")
    wrap("decode_linear", "narrow")
    return calls


def _step_inputs(dev, hidden, nkv, hd, B):
    from test_decode_attn_gpu import TAIL, THETA, _masks
    ops = _ops()
    n = 37
    g = torch.Generator().manual_seed(4)
    dt = torch.bfloat16
    x = torch.randn(B, 1, hidden, generator=g).to(dt).to(dev)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    mask = _masks(B, n)[1][1].to(dev)
    cos, sin = ops.rope_table(torch.randint(20, 37, (B, 1), generator=g).to(dev), hd, THETA)
    return x, cos, sin, kc, vc, n - 1, mask


@pytest.mark.parametrize("lm,hidden,inter,nh,nkv", [("llama", 256, 512, 4, 2), ("phi3", 256, 512, 4, 2), ("llama", 512, 1024, 4, 1)])
def test_layer_decode_wide_vs_stock_sequence_and_row_invariance(dev, clean_env, lm, hidden, inter, nh, nkv):
    from test_decode_linear_gpu import _make_layer
    B, hd = 40, hidden // nh
    layer = _make_layer(dev, torch.bfloat16, lm, hidden, inter, nh, nkv, frozen=True)
    calls = _spy(clean_env)
    x, cos, sin, kc, vc, t, mask = _step_inputs(dev, hidden, nkv, hd, B)
    res = {}
    for env in ("1", "0"):
        clean_env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", env)
        k1, v1 = kc.clone(), vc.clone()
        before = calls["wide"]
        with torch.no_grad():
            y = layer.decode(x, cos, sin, k1, v1, t, mask)
        res[env] = (y, k1, v1, calls["wide"] - before)
    (y1, k1, v1, n1), (y0, k0, v0, n0) = res["1"], res["0"]
    assert (n1, n0) == (4, 0) and calls["narrow"] == 0, f"decode_linear_wide calls: {n1} with the switch at 1, {n0} at 0"
    assert y1.shape == y0.shape == (B, 1, hidden) and torch.isfinite(y1).all()
    e = rel_err(y1, y0)
    print(f"{lm} {hidden}/{inter} B={B}: layer out rel err {e:.3g}")
    assert e < TOL["bf16"]
    keep = torch.ones(k1.shape[2], dtype=torch.bool)
    keep[t] = False
    assert torch.equal(v1[:, :, keep], v0[:, :, keep]) and torch.equal(k1[:, :, keep], k0[:, :, keep])
    assert rel_err(v1[:, :, t], v0[:, :, t]) < TOL["bf16"] and rel_err(k1[:, :, t], k0[:, :, t]) < TOL["bf16"]
    # rows [:17] of the 40-row step are the 17-row step's, bit for bit
    clean_env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "1")
    with torch.no_grad():
        y17 = layer.decode(x[:17], cos[:17], sin[:17], kc[:17].clone(), vc[:17].clone(), t, mask[:17])
    assert calls["wide"] == 8 and torch.equal(y17, y1[:17])
    # the config flag switches it on as well; unset and without the flag it is off
    clean_env.delenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE")
    with torch.no_grad():
        assert torch.equal(layer.decode(x, cos, sin, kc.clone(), vc.clone(), t, mask), y0) and calls["wide"] == 8
        layer.__dict__["_decode_cfg"].decode_linear_wide = True
        assert torch.equal(layer.decode(x, cos, sin, kc.clone(), vc.clone(), t, mask), y1) and calls["wide"] == 12


def _lm(dev, dtype=torch.bfloat16):
    from cambrian_amd.model.language_model import cambrian_llama as CL
    cfg = CL.CambrianConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, rms_norm_eps=1e-5, max_position_embeddings=512, rope_theta=500000.0)
    torch.manual_seed(3)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=dtype)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model.requires_grad_(False)
    return model.eval()


def _prompt(dev, B, L=9):
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(1, 512, (B, L), generator=g).to(dev)
    att = torch.ones(B, L, dtype=torch.long)
    for b in range(1, B):
        att[b, :(2 * b) % (L - 2)] = 0              # left padding: rows of different lengths
    return ids, att.to(dev)


def _first_logits(monkeypatch):
    """Keeps the logits of the first decode step of a generate() call (``_decode_logits``' first result)."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    kept = []
    real = CL._decode_logits

    def wrapped(*a, **kw):
        r = real(*a, **kw)
        if not kept:
            kept.append(r.clone())
        return r

    monkeypatch.setattr(CL, "_decode_logits", wrapped)
    return kept


def test_generate_batch_20_on_the_wide_path(dev, clean_env):
    """Greedy, left padding, 20 sequences: every decode step is 4 wide calls per layer plus the logits with the switch on,
    none with it off; the first decode step's logits agree within the bf16 tolerance (tokens may flip on a near-tie)."""
    model = _lm(dev)
    layers = len(model.model.layers)
    calls = _spy(clean_env)
    kept = _first_logits(clean_env)
    ids, att = _prompt(dev, 20)
    new = 4
    out = {}
    for env in ("1", "0"):
        clean_env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", env)
        calls["wide"] = 0
        del kept[:]
        toks = model.generate(ids, attention_mask=att, max_new_tokens=new)
        assert toks.shape == (20, new)
        out[env] = (kept[0], calls["wide"])
    assert out["1"][1] == (new - 1) * (4 * layers + 1) and out["0"][1] == 0 and calls["narrow"] == 0
    assert out["1"][0].shape == out["0"][0].shape == (20, 512) and out["1"][0].dtype == torch.float32
    e = rel_err(out["1"][0], out["0"][0])
    print(f"first decode step, 20 rows: logits rel err {e:.3g}")
    assert e < TOL["bf16"]


def test_generate_fp32_model_keeps_the_stock_sequence(dev, clean_env):
    model = _lm(dev, torch.float32)
    calls = _spy(clean_env)
    ids, att = _prompt(dev, 20)
    toks = {}
    for env in ("1", "0"):
        clean_env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", env)
        toks[env] = model.generate(ids, attention_mask=att, max_new_tokens=4)
    assert calls == {"wide": 0, "narrow": 0}
    assert torch.equal(toks["1"], toks["0"])


def test_beam_search_of_20_rows_runs_through_the_wide_path(dev, clean_env):
    model = _lm(dev)
    clean_env.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    calls = _spy(clean_env)
    ids, att = _prompt(dev, 4)
    kw = dict(attention_mask=att, num_beams=5, max_new_tokens=4)
    clean_env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "0")
    off = model.generate(ids, **kw)
    assert calls == {"wide": 0, "narrow": 0}
    clean_env.setenv("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", "1")
    on = model.generate(ids, **kw)
    assert calls["wide"] > 0 and calls["wide"] % (4 * len(model.model.layers) + 1) == 0 and calls["narrow"] == 0
    assert on.shape == off.shape and on.dtype == off.dtype
