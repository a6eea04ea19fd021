"""GPU: sampled token selection on the device (``cmb_decode_sample``, decode_sample.hip) and ``generate()`` on top of it.

The reference is ``sample_reference`` of tests/test_decode_sample_host.py: the kernel's definition restated in numpy over the
exact integer Philox4x32-10, exact fp32 ``z`` and float64 masses and scores.

* threshold: with top-k alone ``thr`` and ``n_keep`` are the reference's exactly.  With top-p the device's cut must be the right
  one for some top_p within +-TOL_MASS: mass(z <= thr) / Z > (1 - top_p) - tol and mass(z < thr) / Z <= (1 - top_p) + tol in
  float64, tol = 1e-4 (a 2^-40 fixed-point sum of <= 2^17 positive terms after a 1-2 ulp expf is off by about 1e-5 of Z; ten
  times that); where the float64 margin of a case exceeds 1e-3, ``thr`` is the reference's exactly.
* choice: the id is in the kept set and its float64 score is within 1e-4 of the best (|z|, |g| <= 64: a few fp32 ulps of the sum
  are <= 1e-5; ten times that).
* distribution, non-finite rows, determinism and independence of B, the tail against torch, the argument rules, ``generate()``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_decode_sample_host import (DIST_ROWS, DIST_SEED, DIST_STEPS, DIST_V, check_distribution, distribution_logits,
                                     gumbel_noise, reference_draws, sample_filter, sample_reference)
from test_decode_step_gpu import SENT, THETA, _lm, _NextBufs, _prompt, clean_env  # noqa: F401  (clean_env is a fixture)

pytestmark = pytest.mark.gpu

TOL_MASS, TOL_SCORE, EXACT_MARGIN = 1e-4, 1e-4, 1e-3
H, HD = 72, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _ops():
    from cambrian_amd import ops
    return ops


def _inv(T):
    return float(np.float32(1.0 / T))


def _seed(dev, value):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _padded(rows_cpu: torch.Tensor, ld: int, dev):
    """fp32 [B, V] on the device as a view of [B, ld] whose columns past V hold +inf (a read past V would win)."""
    B, V = rows_cpu.shape
    full = torch.full((B, ld), float("inf"), dtype=torch.float32)
    full[:, :V] = rows_cpu
    return full.to(dev)[:, :V]


class _Call:
    """One ``decode_sample`` call with fresh outputs; ids, thr and n_keep come back as numpy."""

    def __init__(self, dev, logits, T, top_k, top_p, seed, step=0, eos=-1, embed=None, n_tok=None, steps=None, t=36, kv_ld=48):
        ops = _ops()
        B, V = logits.shape
        self.embed = torch.zeros(V, H, dtype=torch.bfloat16, device=dev) if embed is None else embed
        self.n_tok = torch.arange(1, B + 1, dtype=torch.int64, device=dev) if n_tok is None else n_tok
        self.bufs = _NextBufs(dev, B, H, HD, steps or step + 1, kv_ld, eos)
        self.thr = torch.full((B,), 123.0, dtype=torch.float32, device=dev)
        self.n_keep = torch.full((B,), -5, dtype=torch.int32, device=dev)
        self.args = (logits, _inv(T), top_k, top_p, _seed(dev, seed), eos, self.bufs.done if eos >= 0 else None, self.bufs.out,
                     step, self.n_tok, self.bufs.pos, self.bufs.kv, t, self.embed, self.bufs.x, HD, THETA, self.bufs.cos,
                     self.bufs.sin)
        self.step, self.t = step, t
        ops.decode_sample(*self.args, thr=self.thr, n_keep=self.n_keep)
        torch.cuda.synchronize()
        self.ids = self.bufs.out[:, step].cpu().numpy()
        self.thr_np, self.n_keep_np = self.thr.cpu().numpy(), self.n_keep.cpu().numpy()


def _check_row(l_row, T, top_k, top_p, seed, b, step, got_id, got_thr, got_n, what):
    """Every assertion on one row of one call (see the module docstring)."""
    inv = _inv(T)
    ref = sample_reference(l_row, inv, top_k, top_p, seed, b, step)
    if ref["argmax"] is not None:
        assert got_id == ref["argmax"] and np.isnan(got_thr) and got_n == 0, (what, b)
        return
    z = ref["z"]
    z64 = z.astype(np.float64)
    got_thr = np.float32(got_thr)
    if float(np.float32(top_p)) >= 1.0:
        assert got_thr == np.float32(ref["thr"]) and got_n == ref["n_keep"], (what, b, got_thr, ref["thr"], got_n, ref["n_keep"])
        keep = ref["keep"]
    else:
        in_k = sample_filter(l_row, inv, top_k, 1.0)["keep"]
        w = np.where(in_k, np.exp(z64 - z64.max()), 0.0)
        Z = w.sum()
        le, lt = w[z <= got_thr].sum() / Z, w[z < got_thr].sum() / Z
        cut = 1.0 - float(np.float32(top_p))
        print(f"{what} row {b}: mass(z <= thr) {le:.9f}, mass(z < thr) {lt:.9f}, 1 - top_p {cut:.9f}, margin {ref['margin']:.3g}")
        assert (in_k & (z == got_thr)).any(), (what, b, "thr is no value of the row", got_thr)
        assert le > cut - TOL_MASS and lt <= cut + TOL_MASS, (what, b, le, lt, cut)
        if ref["margin"] > EXACT_MARGIN:
            assert got_thr == np.float32(ref["thr"]), (what, b, got_thr, ref["thr"], ref["margin"])
        keep = in_k & (z >= got_thr)
        assert got_n == int(keep.sum()), (what, b, got_n, int(keep.sum()))
    assert keep[got_id], (what, b, "the id is outside the kept set", got_id)
    with np.errstate(invalid="ignore"):
        s = np.where(keep, z64 + gumbel_noise(seed, z.shape[0], [b], [step])[0, 0], -np.inf)
    print(f"{what} row {b}: s[id] {s[got_id]:.7f}, max s {s.max():.7f}")
    assert s[got_id] >= s.max() - TOL_SCORE, (what, b, got_id, int(np.argmax(s)), s[got_id], s.max())


KS = lambda V: (0, 1, 20, V + 7)          # noqa: E731
PS = (1.0, 0.9, 0.5, 1e-6)
TS = (0.5, 1.0, 1.3)


@pytest.mark.parametrize("V", [1, 5, 64, 1000, 4099, 32064])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_decode_sample_against_the_restatement(dev, B, V):
    """Every (top_k, top_p) pair, the temperature and the row stride cycling: contiguous rows, an odd stride (rows start at every
    alignment, so head and tail pieces are exercised), lm_head's padded stride.  Logits randn * 3 clamped so that |z| <= 64."""
    gen = torch.Generator().manual_seed(1000 * B + V)
    lds = (V, V + 5, (V + 7) // 8 * 8 + 8)
    n = 0
    for top_k in KS(V):
        for top_p in PS:
            T = TS[n % 3]
            rows = (torch.randn(B, V, generator=gen) * 3).clamp_(-64 * T, 64 * T)
            logits = _padded(rows, lds[n % 3], dev)
            seed, step = 77 + n, n % 5
            c = _Call(dev, logits, T, top_k, top_p, seed, step=step)
            for b in range(B):
                _check_row(rows[b].numpy(), T, top_k, top_p, seed, b, step, int(c.ids[b]), c.thr_np[b], int(c.n_keep_np[b]),
                           f"V={V} B={B} k={top_k} p={top_p} T={T}")
            n += 1


@pytest.mark.parametrize("T", [1.0, 0.5])
def test_ties_straddle_the_kth_place_and_the_nucleus_cut(dev, T):
    """Logits rounded to multiples of 0.25: many equal values, at the k-th place and at the cut.  Equal values are kept or
    dropped together, so n_keep counts whole groups; plus the 0.8 / 0.81 pair of test_top_p_keeps_smallest_sufficient_set."""
    gen = torch.Generator().manual_seed(5)
    B, V = 3, 1000
    rows = ((torch.randn(B, V, generator=gen) * 3).clamp_(-30, 30) * 4).round() / 4
    logits = _padded(rows, V + 5, dev)
    for top_k, top_p in ((20, 1.0), (20, 0.9), (0, 0.9), (0, 0.5), (50, 0.5), (V + 7, 0.9)):
        c = _Call(dev, logits, T, top_k, top_p, 11)
        for b in range(B):
            l = rows[b].numpy()
            _check_row(l, T, top_k, top_p, 11, b, 0, int(c.ids[b]), c.thr_np[b], int(c.n_keep_np[b]), f"ties k={top_k} p={top_p}")
            z = sample_filter(l, _inv(T), 0, 1.0)["z"]
            assert int(c.n_keep_np[b]) == int((z >= c.thr_np[b]).sum())
        if top_k == 20 and top_p == 1.0:
            assert int(c.n_keep_np.max()) > 20, "this case is here for ties at the k-th place"
    pair = torch.log(torch.tensor([[0.5, 0.3, 0.15, 0.05]]))
    for top_p, want in ((0.8, None), (0.81, 3)):          # at 0.8 the mass from below EQUALS 1 - top_p: either cut is in tolerance
        c = _Call(dev, _padded(pair, 9, dev), 1.0, 0, top_p, 3)
        _check_row(pair[0].numpy(), 1.0, 0, top_p, 3, 0, 0, int(c.ids[0]), c.thr_np[0], int(c.n_keep_np[0]), f"pair p={top_p}")
        assert want is None or int(c.n_keep_np[0]) == want


def test_rows_with_minus_infinity_entries(dev):
    gen = torch.Generator().manual_seed(6)
    B, V = 3, 4099
    rows = torch.randn(B, V, generator=gen) * 3
    rows[0, ::3] = float("-inf")
    rows[1, 5:] = float("-inf")                             # five finite entries: top_k = 20 reaches into the -inf
    rows[2, :V - 1] = float("-inf")
    logits = _padded(rows, V + 5, dev)
    for top_k, top_p in ((0, 1.0), (20, 1.0), (20, 0.9), (0, 0.5), (V + 7, 1e-6)):
        c = _Call(dev, logits, 1.3, top_k, top_p, 19, step=2)
        for b in range(B):
            _check_row(rows[b].numpy(), 1.3, top_k, top_p, 19, b, 2, int(c.ids[b]), c.thr_np[b], int(c.n_keep_np[b]),
                       f"-inf k={top_k} p={top_p}")
            assert np.isfinite(rows[b, int(c.ids[b])].item())
    assert int(c.ids[2]) == V - 1


def test_non_finite_rows_take_the_argmax(dev):
    B, V = 5, 1000
    gen = torch.Generator().manual_seed(7)
    rows = torch.randn(B, V, generator=gen) * 3
    rows[0, 700] = rows[0, 900] = float("nan")
    rows[0, 701] = float("inf")                             # the first NaN beats the +inf beside it
    rows[1, 400] = rows[1, 600] = float("inf")
    rows[2].fill_(float("-inf"))
    rows[3, 10] = 3.0e38                                    # finite, z = l * 2 overflows
    logits = _padded(rows, V + 5, dev)
    want = torch.argmax(logits, -1).cpu().numpy()
    assert want[:4].tolist() == [700, 400, 0, 10]
    for top_k, top_p in ((0, 1.0), (20, 0.9)):
        c = _Call(dev, logits, 0.5, top_k, top_p, 23)
        assert c.ids[:4].tolist() == want[:4].tolist()
        assert np.isnan(c.thr_np[:4]).all() and (c.n_keep_np[:4] == 0).all()
        _check_row(rows[4].numpy(), 0.5, top_k, top_p, 23, 4, 0, int(c.ids[4]), c.thr_np[4], int(c.n_keep_np[4]), "plain row")


def test_same_bits_twice_and_a_row_does_not_depend_on_the_batch(dev):
    gen = torch.Generator().manual_seed(8)
    B, V = 16, 4099
    rows = torch.randn(B, V, generator=gen) * 3
    logits = _padded(rows, V + 5, dev)
    for top_k, top_p in ((0, 1.0), (20, 0.9)):
        a = _Call(dev, logits, 1.3, top_k, top_p, 31, step=3)
        again = _Call(dev, logits, 1.3, top_k, top_p, 31, step=3)
        for x, y in zip(a.bufs.tensors() + [a.thr, a.n_keep], again.bufs.tensors() + [again.thr, again.n_keep]):
            assert torch.equal(x, y)
        for small in (1, 3):
            c = _Call(dev, logits[:small], 1.3, top_k, top_p, 31, step=3)
            assert c.ids.tolist() == a.ids[:small].tolist()
            assert c.thr_np.tolist() == a.thr_np[:small].tolist() and c.n_keep_np.tolist() == a.n_keep_np[:small].tolist()
        # the row index, the step and the seed all reach the counter: identical rows, other draws
        same = _padded(rows[:1].expand(B, V).contiguous(), V, dev)
        base = _Call(dev, same, 1.3, top_k, top_p, 31, step=3).ids
        assert len(set(base.tolist())) > 1
        assert _Call(dev, same, 1.3, top_k, top_p, 31, step=4).ids.tolist() != base.tolist()
        assert _Call(dev, same, 1.3, top_k, top_p, 32, step=3).ids.tolist() != base.tolist()
        assert _Call(dev, same, 1.3, top_k, top_p, 31 + (1 << 32), step=3).ids.tolist() != base.tolist()    # the seed's high word


@pytest.mark.parametrize("top_k", [0, 8])
def test_draws_follow_the_softmax(dev, top_k):
    """V = 64, 16 rows of identical logits, 256 draws: the 4096 pooled ids against the (renormalised) softmax by Pearson's
    chi-square with bins merged to an expectation >= 5, bound = the 99.9 % quantile by Wilson-Hilferty.  The restatement passes
    this for the seed used here and the next two (tests/test_decode_sample_host.py)."""
    ops = _ops()
    l = distribution_logits()
    f = sample_filter(l, 1.0, top_k, 1.0)
    logits = torch.from_numpy(l)[None].expand(DIST_ROWS, DIST_V).contiguous().to(dev)
    bufs = _NextBufs(dev, DIST_ROWS, H, HD, DIST_STEPS, 48, -1)
    embed = torch.zeros(DIST_V, H, dtype=torch.bfloat16, device=dev)
    n_tok = torch.ones(DIST_ROWS, dtype=torch.int64, device=dev)
    seed = _seed(dev, DIST_SEED)
    for step in range(DIST_STEPS):
        ops.decode_sample(logits, 1.0, top_k, 1.0, seed, -1, None, bufs.out, step, n_tok, bufs.pos, bufs.kv, 5, embed, bufs.x, HD,
                          THETA, bufs.cos, bufs.sin)
    torch.cuda.synchronize()
    ids = bufs.out.cpu().numpy()
    check_distribution(ids, f["z"], f["keep"])
    # and draw for draw it is the restatement's stream (fp32 scores: a near-tie may resolve the other way, so not all 4096)
    agree = float((ids == reference_draws(f["z"], f["keep"], DIST_SEED)).mean())
    print(f"draws equal to the restatement's: {agree:.4f}")
    assert agree >= 0.99


@pytest.mark.parametrize("B", [1, 3, 16])
def test_tail_against_torch(dev, B):
    """Outputs with sentinels around them, against torch expressions: the id (reference), pos, the key-mask byte, the embedding
    row, cos / sin; then the eos / done rule over three calls with top_k = 1, where the id is the argmax (the cases of
    test_decode_next_eos_and_done_over_three_calls)."""
    ops = _ops()
    V, steps, kv_ld, t0 = 1000, 4, 48, 40
    gen = torch.Generator(device=dev).manual_seed(50 + B)
    embed = torch.randn(V + 3, H + 8, generator=gen, device=dev).to(torch.bfloat16)[:, :H]
    n_tok = torch.randint(1, 30, (B,), generator=gen, device=dev)
    rows = (torch.randn(B, V, generator=gen, device=dev) * 3).cpu()
    logits = _padded(rows, V + 5, dev)
    probe = _NextBufs(dev, B, H, HD, steps, kv_ld, -1)
    before = probe.tensors()
    c = _Call(dev, logits, 1.3, 20, 0.9, 41, step=2, embed=embed, n_tok=n_tok, steps=steps, t=t0)
    want = torch.tensor([sample_reference(rows[b].numpy(), _inv(1.3), 20, 0.9, 41, b, 2)["id"] for b in range(B)], device=dev)
    bufs = c.bufs
    assert torch.equal(bufs.out[:, 2], want)
    assert torch.equal(bufs.pos, n_tok + 2) and bool((bufs.kv[:, t0] == 1).all())
    assert torch.equal(bufs.x, embed[want])
    cos, sin = ops.rope_table((n_tok + 2)[:, None], HD, THETA)
    assert torch.equal(bufs.cos, cos) and torch.equal(bufs.sin, sin)
    bufs.out[:, 2] = -SENT
    bufs.pos.fill_(-SENT)
    bufs.kv[:, t0] = SENT
    bufs.x.fill_(float(SENT))
    bufs.cos.fill_(float(SENT))
    bufs.sin.fill_(float(SENT))
    for name, a, b_ in zip(("out_ids", "pos", "key_valid", "x", "cos", "sin", "done"), before, bufs.tensors()):
        assert torch.equal(a, b_), f"{name}: bytes around the output changed"

    rounds = [torch.randn(B, V, generator=gen, device=dev) for _ in range(3)]
    eos = int(rounds[0][0].argmax())
    for r in rounds:
        r[1:B - 1 if B > 2 else B, eos] = -50.0
    rounds[1][B - 1, eos] = 50.0
    rounds[1][0, eos] = -50.0
    rounds[2][:, eos] = -50.0
    bufs = _NextBufs(dev, B, H, HD, steps, kv_ld, eos)
    seed = _seed(dev, 43)
    done_ref = torch.zeros(B, dtype=torch.bool, device=dev)
    for step, lg in enumerate(rounds):
        nxt = lg.argmax(-1)
        nxt = torch.where(done_ref, torch.full_like(nxt, eos), nxt)
        done_ref = done_ref | (nxt == eos)
        ops.decode_sample(lg, _inv(0.5), 1, 0.9, seed, eos, bufs.done, bufs.out, step, n_tok, bufs.pos, bufs.kv, t0 + step, embed,
                          bufs.x, HD, THETA, bufs.cos, bufs.sin)
        torch.cuda.synchronize()
        assert torch.equal(bufs.out[:, step], nxt), step
        assert torch.equal(bufs.done.bool(), done_ref) and bool((bufs.done <= 1).all()), step
        assert torch.equal(bufs.x, embed[nxt])
        assert torch.equal(bufs.pos, n_tok + step) and bool((bufs.kv[:, t0 + step] == 1).all())
    assert bool(done_ref[0]) and bool(done_ref[B - 1]) and int(done_ref.sum()) == min(B, 2)
    assert int(bufs.done_full[0]) == SENT and int(bufs.done_full[-1]) == SENT


def test_arguments_are_checked_before_any_launch(dev):
    """Host buffers: every case returns before anything is launched, the pointers are never dereferenced.  cmb_decode_next's
    rules in its order (NULL pointers, sizes and strides, alignment) and the new ones at their places."""
    from cambrian_amd import lib as L
    lib = L.load()
    bad_arg, alignment = -1, -2
    buf = (C.c_double * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16
    args = dict(logits=p, logits_ld=8, B=2, V=8, inv_temperature=1.0, top_k=0, top_p=1.0, seed=p, eos=-1, done=None, out_ids=p,
                out_ld=4, step=0, n_tok=p, pos=p, key_valid=p, kv_ld=4, t=0, embed=p, embed_ld=8, embed_rows=8, H=8, x=p, x_ld=8,
                hd=4, rope_base=1e4, cos_t=p, sin_t=p, thr=None, n_keep=None)

    def call(**over):
        assert not set(over) - set(args), over
        return lib.cmb_decode_sample(*[over.get(k, v) for k, v in args.items()], None)

    for name in ("logits", "seed", "out_ids", "n_tok", "pos", "key_valid", "embed", "x", "cos_t", "sin_t"):
        assert call(**{name: None}) == bad_arg, name
        assert call(**{name: None}, B=0, top_k=-1) == bad_arg, name             # the NULL test comes first
    for over in (dict(B=0), dict(B=17), dict(V=0), dict(V=1 << 31), dict(logits_ld=7), dict(embed_rows=7), dict(eos=-2), dict(eos=8),
                 dict(eos=3), dict(step=-1), dict(step=4), dict(t=-1), dict(t=4), dict(H=4), dict(H=12), dict(embed_ld=4),
                 dict(x_ld=12), dict(hd=0), dict(hd=3),
                 dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=float("inf")),
                 dict(inv_temperature=float("nan")), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan")),
                 dict(top_k=-1)):
        assert call(**over) == bad_arg, over
        assert call(**over, embed=p + 2, seed=p + 4) == bad_arg, over           # sizes come before alignment
    for over in (dict(logits=p + 2), dict(out_ids=p + 4), dict(n_tok=p + 4), dict(pos=p + 4), dict(embed=p + 8), dict(x=p + 8),
                 dict(seed=p + 4), dict(thr=p + 2), dict(n_keep=p + 2)):
        assert call(**over) == alignment, over


# ---------------------------------------------------------------------------------------------------------------------
# generate()
# ---------------------------------------------------------------------------------------------------------------------
def _spies(monkeypatch):
    ops = _ops()
    calls = {"sample": 0, "step": 0, "next": 0, "linear": 0, "linear_fp8": 0, "attention": 0, "multinomial": 0, "sort": 0,
             "topk": 0}
    for mod, key, name in ((ops, "sample", "decode_sample"), (ops, "step", "decode_step"), (ops, "next", "decode_next"),
                           (ops, "linear", "decode_linear"), (ops, "linear_fp8", "decode_linear_fp8"),
                           (ops, "attention", "decode_attention"), (torch, "multinomial", "multinomial"), (torch, "sort", "sort"),
                           (torch, "topk", "topk")):
        real = getattr(mod, name)

        def counted(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(mod, name, counted)
    return calls


def _run(model, monkeypatch, calls, step_switch, sample_switch, ids, att, seed=123, **kw):
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", step_switch)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_SAMPLE", sample_switch)
    for k in calls:
        calls[k] = 0
    torch.manual_seed(seed)
    toks = model.generate(ids, attention_mask=att, **kw)
    torch.cuda.synchronize()
    return toks, dict(calls)


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_samples_on_the_device(dev, clean_env, lm):
    clean_env.delenv("CAMBRIAN_AMD_DECODE_SAMPLE", raising=False)
    model = _lm(dev, lm)
    calls = _spies(clean_env)
    ids, att = _prompt(dev, 3)
    new = 12
    kw = dict(max_new_tokens=new, do_sample=True, temperature=0.8, top_k=20, top_p=0.9)
    on, n_on = _run(model, clean_env, calls, "1", "1", ids, att, **kw)
    assert on.shape == (3, new) and on.dtype == torch.int64
    assert n_on["sample"] == new and n_on["step"] == new - 1 and n_on["next"] == 0, n_on
    assert n_on["linear"] == 0 and n_on["linear_fp8"] == 0 and n_on["attention"] == 0, n_on
    assert n_on["multinomial"] == 0 and n_on["sort"] == 0 and n_on["topk"] == 0, n_on
    again, _ = _run(model, clean_env, calls, "1", "1", ids, att, **kw)
    assert torch.equal(again, on), "the same torch.manual_seed must give the same ids"
    other, _ = _run(model, clean_env, calls, "1", "1", ids, att, seed=124, **kw)
    assert not torch.equal(other, on), "the seed does not reach the sampler"
    # the switch from the config, and the environment over it
    clean_env.delenv("CAMBRIAN_AMD_DECODE_SAMPLE")
    model.config.decode_sample_device = True
    for k in calls:
        calls[k] = 0
    torch.manual_seed(123)
    assert torch.equal(model.generate(ids, attention_mask=att, **kw), on) and calls["sample"] == new
    assert _run(model, clean_env, calls, "1", "0", ids, att, **kw)[1]["sample"] == 0
    model.config.decode_sample_device = False
    # one kept token is greedy decoding
    greedy, n_g = _run(model, clean_env, calls, "1", "1", ids, att, max_new_tokens=new)
    assert n_g["sample"] == 0 and n_g["next"] == new
    for only_one in (dict(top_k=1), dict(top_p=1e-6)):
        got, n = _run(model, clean_env, calls, "1", "1", ids, att, max_new_tokens=new, do_sample=True, temperature=0.8, **only_one)
        assert n["sample"] == new and torch.equal(got, greedy), (only_one, got.tolist(), greedy.tolist())
    # top_p <= 0 raises the warper's error
    with pytest.raises(ValueError, match="`top_p` has to be a float > 0 and <= 1"):
        _run(model, clean_env, calls, "1", "1", ids, att, max_new_tokens=new, do_sample=True, temperature=0.8, top_p=0.0)
    assert calls["sample"] == 0


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_with_eos_on_the_device(dev, clean_env, lm):
    """The rows are independent and the draws are counted by (row, step), so the run with an eos id is the free run up to each
    row's first eos, eos from there on, cut at the first column where every row is done."""
    model = _lm(dev, lm)
    calls = _spies(clean_env)
    ids, att = _prompt(dev, 3)
    new = 20
    kw = dict(max_new_tokens=new, do_sample=True, temperature=1.3, top_k=40)
    free, _ = _run(model, clean_env, calls, "1", "1", ids, att, **kw)
    rows = free.tolist()
    eos = rows[1][2]
    want, stop = [], 0
    for r in rows:
        first = r.index(eos) if eos in r else new
        want.append(r[:first] + [eos] * (new - first))
        stop = max(stop, first)
    stop = min(stop + 1, new)
    got, n = _run(model, clean_env, calls, "1", "1", ids, att, eos_token_id=eos, **kw)
    assert got.tolist() == [w[:stop] for w in want], (got.tolist(), want, stop)
    assert bool((got[1, 2:] == eos).all())
    assert n["sample"] == min(new, -(-stop // 8) * 8) and n["step"] == n["sample"] - 1, n      # on to the next poll, no further
    assert n["multinomial"] == 0 and n["linear"] == 0


@pytest.mark.parametrize("why", ["fp32", "batch17", "step_off"])
def test_outside_the_conditions_the_sample_switch_changes_nothing(dev, clean_env, why):
    model = _lm(dev, "llama", dt=torch.float32 if why == "fp32" else torch.bfloat16)
    calls = _spies(clean_env)
    ids, att = _prompt(dev, 17 if why == "batch17" else 3)
    step_switch = "0" if why == "step_off" else "1"
    kw = dict(max_new_tokens=6, do_sample=True, temperature=0.7, top_k=20, top_p=0.9)
    off, n_off = _run(model, clean_env, calls, step_switch, "0", ids, att, seed=9, **kw)
    on, n_on = _run(model, clean_env, calls, step_switch, "1", ids, att, seed=9, **kw)
    assert torch.equal(on, off)
    assert n_on == n_off and n_on["sample"] == 0 and n_on["step"] == 0 and n_on["multinomial"] == 6, (why, n_on, n_off)
