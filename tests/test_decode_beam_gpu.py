"""GPU: beam search on the device (``cmb_decode_beam``, decode_beam.hip) and ``generate(num_beams > 1)`` on top of it.

The reference is the torch restatement, cambrian_amd/model/language_model/beam.py (itself checked against HF on the CPU,
tests/test_decode_beam_host.py): a call starts from a state the restatement reached and must leave the restatement's next state.

* selection: tokens, parents, sequences, hypotheses, flags, ``pos``, the key-mask byte and the embedding rows are equal.  A prompt
  is excused only where the fp64 gap among its top K + 1 scores is below GAP = 1e-4 (the kernel's log-sum-exp is not torch's, so a
  nearer pair may resolve the other way); at most EXCUSED = 10 % of the prompts of a test may be.
* scores: against an fp64 restatement on the same inputs.  The yardstick is the error of torch's fp32 ``log_softmax`` against
  fp64 on those inputs; the kernel gets twice that plus one ulp of the score.
* exact ties, rows with -inf, non-finite rows, determinism and independence of the other prompts, the cache reorder, the
  argument rules, ``generate()``.
"""
import ctypes as C

import pytest
import torch

from cambrian_amd.model.language_model import beam as BM
from test_decode_beam_host import decision_gap, load_beam_fixture
from test_decode_step_gpu import THETA, _lm, _prompt, clean_env as _step_clean_env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

GAP, EXCUSED = 1e-4, 0.10
H, HD, KV_LD, T0 = 72, 64, 48, 40
CONFIGS = [(1, 2), (1, 3), (2, 4), (1, 8), (1, 16), (4, 4), (8, 2)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture()
def clean_env(_step_clean_env):
    for name in ("CAMBRIAN_AMD_DECODE_BEAM", "CAMBRIAN_AMD_DECODE_SAMPLE"):
        _step_clean_env.delenv(name, raising=False)
    return _step_clean_env


def _ops():
    from cambrian_amd import ops
    return ops


def _padded(rows_cpu: torch.Tensor, ld: int, dev):
    """fp32 [R, V] on the device as a view of [R, ld] whose columns past V hold a large FINITE value (a read past V would win)."""
    R, V = rows_cpu.shape
    full = torch.full((R, ld), 1.0e30, dtype=torch.float32)
    full[:, :V] = rows_cpu
    return full.to(dev)[:, :V]


def _load(state, st: BM.BeamState, step: int):
    """The restatement's state before ``step`` into a device state block."""
    B, nb, M = st.run_ids.shape
    state.buf.zero_()
    state.run_score.copy_(st.run_score.reshape(-1))
    state.fin_score.copy_(st.fin_score.reshape(-1))
    state.fin_len.copy_(st.fin_len.reshape(-1))
    state.fin_ok.copy_(st.fin_ok.reshape(-1).to(torch.uint8))
    state.unsat.copy_(st.unsat.to(torch.uint8))
    state.run_ids2[step & 1].copy_(st.run_ids.reshape(B * nb, M))
    state.fin_ids.copy_(st.fin_ids.reshape(B * nb, M))


class _Call:
    """One ``decode_beam`` call from the restatement's state ``st`` (left untouched), everything read back to the host."""

    def __init__(self, dev, logits, st, step, eos, embed, n_tok):
        ops = _ops()
        B, nb, M = st.run_ids.shape
        R = B * nb
        self.state = ops.DecodeBeamState(B, nb, M, dev)
        if step:                                                  # step 0 reads nothing: the block stays zeroed
            _load(self.state, st, step)
        self.pos = torch.full((R,), -7, dtype=torch.int64, device=dev)
        self.kv = torch.zeros(R, KV_LD, dtype=torch.uint8, device=dev)
        self.x = torch.zeros(R, H + 8, dtype=torch.bfloat16, device=dev)[:, :H]
        self.cos = torch.zeros(R, HD // 2, dtype=torch.float32, device=dev)
        self.sin = torch.zeros_like(self.cos)
        ops.decode_beam(logits, nb, -1 if eos is None else eos, self.state, step, n_tok, self.pos, self.kv, T0 + step, embed,
                        self.x, HD, THETA, self.cos, self.sin)
        torch.cuda.synchronize()
        self.after = self.state.view(step + 1)
        self.parent = self.state.parent.view(B, nb).cpu()
        self.tok = self.state.tok.view(B, nb).cpu()
        self.unfinished = int(self.state.unfinished.item())


def _ulp(x: torch.Tensor) -> torch.Tensor:
    x = x.abs().double().clamp_min(1e-30)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


def _check_step(c: _Call, rows_cpu, st_before, st_after, parent, tok, step, eos, last, embed, n_tok, what):
    """Everything one call must have left, against the restatement's step from the same state; returns (prompts excused,
    the yardstick, the largest score error)."""
    B, nb, M = st_before.run_ids.shape
    V = rows_cpu.shape[1]
    K = 2 * nb
    lp64 = torch.log_softmax(rows_cpu.double(), -1).view(B, nb, V)
    lp32 = torch.log_softmax(rows_cpu, -1).view(B, nb, V)
    finite = torch.isfinite(lp64)
    yard = float((lp32.double() - lp64)[finite].abs().max())
    s64 = lp64 + st_before.run_score.double()[:, :, None]
    top = torch.sort(s64.reshape(B, nb * V), dim=1, descending=True, stable=True).values[:, :K + 1]
    gaps = top[:, :-1] - top[:, 1:]
    gaps[~torch.isfinite(gaps)] = float("inf")                     # -inf beside -inf: the order is the index, exactly
    excused = gaps.min(dim=1).values < GAP
    got = c.after
    worst = 0.0
    for b in range(B):
        if bool(excused[b]):
            continue
        w = (what, "prompt", b)
        assert c.parent[b].tolist() == parent[b].tolist() and c.tok[b].tolist() == tok[b].tolist(), w
        assert torch.equal(got.run_ids[b, :, :step + 1].cpu(), st_after.run_ids[b, :, :step + 1]), w
        assert torch.equal(got.fin_len[b].cpu(), st_after.fin_len[b]) and torch.equal(got.fin_ok[b].cpu(), st_after.fin_ok[b]), w
        for i in range(nb):
            n = int(st_after.fin_len[b, i])
            assert torch.equal(got.fin_ids[b, i, :n].cpu(), st_after.fin_ids[b, i, :n]), w
        assert bool(got.unsat[b]) == bool(st_after.unsat[b]) and bool(got.all_hit[b]) == bool(st_after.all_hit[b]), w
        rows = slice(b * nb, (b + 1) * nb)
        assert torch.equal(c.pos[rows].cpu(), n_tok[rows].cpu() + step), w
        assert bool((c.kv[rows, T0 + step] == 1).all()) and int(c.kv[rows].sum()) == nb, w
        assert torch.equal(c.x[rows].cpu(), embed[tok[b]].cpu()), w
        # the running scores in fp64: run_score[parent] + lp[parent, tok], 1e9 lower where the candidate hit
        hit = torch.ones(nb, dtype=torch.bool) if last else (tok[b] == eos if eos is not None else torch.zeros(nb, dtype=torch.bool))
        want = s64[b, parent[b], tok[b]] + hit.double() * BM.NEG
        have = got.run_score[b].cpu().double()
        ok = torch.isfinite(want)
        err = (have - want)[ok].abs()
        tol = 2 * yard + _ulp(want[ok])
        assert bool((err <= tol).all()), (w, "run_score", err.max().item(), tol.min().item(), yard)
        assert torch.equal(have[~ok], want[~ok]), w
        real = want[ok] > -5e8                                     # beside a -1e9 marker an ulp is 64: not a figure to report
        worst = max(worst, float(err[real].max()) if bool(real.any()) else 0.0)
        # hypotheses added in this step, where the sequence names its parent: score / (step + 1)
        for i in range(nb):
            if not bool(st_after.fin_ok[b, i]) or int(st_after.fin_len[b, i]) != step + 1 or step == 0:
                continue
            seq = st_after.fin_ids[b, i, :step + 1]
            par = [j for j in range(nb) if torch.equal(st_before.run_ids[b, j, :step], seq[:step])]
            if len(par) != 1:
                continue
            want_h = s64[b, par[0], seq[step]] / (step + 1) + (0.0 if bool(st_before.unsat[b]) else BM.NEG)
            err_h = abs(float(got.fin_score[b, i].cpu().double() - want_h))
            assert err_h <= 2 * yard + float(_ulp(want_h)), (w, "fin_score", i, err_h, yard)
            worst = max(worst, err_h if float(s64[b, par[0], seq[step]]) > -5e8 and bool(st_before.unsat[b]) else 0.0)
    assert c.unfinished == int(not BM.beam_done(st_after)) or bool(excused.any()), what
    return int(excused.sum()), yard, worst


def _drive(dev, B, nb, V, seed, max_new=4, check=True):
    """max_new steps (0, 1, ..., the last) of one (B, num_beams, V) configuration in lockstep with the restatement."""
    gen = torch.Generator().manual_seed(seed)
    R = B * nb
    eos = int(torch.randint(0, V, (1,), generator=gen))
    lds = (V, V + 5, (V + 7) // 8 * 8 + 8)
    st = BM.BeamState(B, nb, max_new)
    embed = n_tok = None
    if check:
        embed = torch.randn(V + 3, H + 8, generator=gen).to(torch.bfloat16).to(dev)[:, :H]
        n_tok = torch.randint(1, 30, (B,), generator=gen).repeat_interleave(nb).to(dev)
    excused, prompts, yard, worst = 0, 0, 0.0, 0.0
    for step in range(max_new):
        rows = torch.randn(R, V, generator=gen) * 3
        rows[:, eos] += 2.0                                        # a frequent eos: hypotheses form early
        last = step + 1 == max_new
        before = BM.BeamState.__new__(BM.BeamState)
        before.__dict__.update({k: v.clone() for k, v in st.__dict__.items()})
        parent, tok = BM.beam_update(st, rows, step, eos, last)
        prompts += B
        if not check:                                              # the CPU rehearsal: how many prompts the rule excuses
            s64 = torch.log_softmax(rows.double(), -1).view(B, nb, V) + before.run_score.double()[:, :, None]
            top = torch.sort(s64.reshape(B, nb * V), dim=1, descending=True).values[:, :2 * nb + 1]
            excused += int(((top[:, :-1] - top[:, 1:]).min(dim=1).values < GAP).sum())
            continue
        c = _Call(dev, _padded(rows, lds[step % 3], dev), before, step, eos, embed, n_tok)
        e, y, w = _check_step(c, rows, before, st, parent, tok, step, eos, last, embed, n_tok, (B, nb, V, step))
        excused, yard, worst = excused + e, max(yard, y), max(worst, w)
    return excused, prompts, yard, worst


@pytest.mark.parametrize("V", [2, 5, 64, 1000, 4099, 32064])
def test_decode_beam_against_the_restatement(dev, V):
    """Every (prompts, num_beams) configuration, four steps each (0, 1, 2 and the last), the row stride cycling: contiguous, odd
    (rows start at every alignment), lm_head's padded stride.  V = 5 with 16 beams is a row with fewer than K entries."""
    excused = prompts = 0
    yard = worst = 0.0
    for n, (B, nb) in enumerate(CONFIGS):
        e, p, y, w = _drive(dev, B, nb, V, 1000 * V + n)
        excused, prompts, yard, worst = excused + e, prompts + p, max(yard, y), max(worst, w)
    print(f"V={V}: {excused} of {prompts} prompts excused; log_softmax fp32 against fp64 {yard:.3e}, "
          f"largest score error of the kernel {worst:.3e}")
    assert excused <= EXCUSED * prompts, (excused, prompts)


def _tie_case(nb, V, seed, kind):
    """Quantised logits (many equal values inside a row), identical rows with equal running scores; a state after step 1."""
    gen = torch.Generator().manual_seed(seed)
    row = (torch.randn(1, V, generator=gen) * 2).round()
    rows = row.expand(nb, V).clone()
    st = BM.BeamState(1, nb, 6)
    st.run_score[:] = -1.5
    st.run_ids[0, :, 0] = torch.arange(nb)
    eos = int(row[0].argmax())
    if kind == "minus_inf":
        rows[0, 3:] = float("-inf")                               # nb + 2 finite entries in all: K reaches into the -inf,
        rows[1:, 1:] = float("-inf")                              # which the rows resolve by the lowest index
    return rows, st, eos


@pytest.mark.parametrize("kind", ["ties", "minus_inf"])
@pytest.mark.parametrize("nb", [2, 3, 4])
def test_exact_ties_resolve_as_the_restatement(dev, nb, kind):
    """Equal logits inside a row and identical rows with equal running scores: ties at the K-th place, at the num_beams-th place
    and in the merge of the hypotheses (equal new hypotheses; the -1e9 entries behind them).  Nothing is excused."""
    seen = dict(kth=0, nbth=0, merge=0)
    V, step = 64, 1
    embed = torch.zeros(V, H, dtype=torch.bfloat16, device=dev)
    n_tok = torch.ones(nb, dtype=torch.int64, device=dev)
    for seed in range(6):
        rows, st, eos = _tie_case(nb, V, 50 + seed, kind)
        before = BM.BeamState.__new__(BM.BeamState)
        before.__dict__.update({k: v.clone() for k, v in st.__dict__.items()})
        trace = {}
        parent, tok = BM.beam_update(st, rows, step, eos, False, trace)
        K = 2 * nb
        if kind == "minus_inf" and nb > 2:
            assert bool(torch.isinf(trace["cand"][0, K - 1])), "this case is here for a K that reaches into the -inf"
        seen["kth"] += int(trace["cand"][0, K - 1] == trace["cand"][0, K])
        seen["nbth"] += int(trace["run"][0, nb - 1] == trace["run"][0, nb])
        seen["merge"] += int(trace["merged"][0, 0] == trace["merged"][0, 1] or trace["merged"][0, nb - 1] == trace["merged"][0, nb])
        c = _Call(dev, _padded(rows, V + 5, dev), before, step, eos, embed, n_tok)
        w = (kind, nb, seed)
        assert c.parent.tolist() == parent.tolist() and c.tok.tolist() == tok.tolist(), w
        assert torch.equal(c.after.run_ids[:, :, :2].cpu(), st.run_ids[:, :, :2]), w
        assert torch.equal(c.after.fin_ok.cpu(), st.fin_ok) and torch.equal(c.after.fin_len.cpu(), st.fin_len), w
        for i in range(nb):
            n = int(st.fin_len[0, i])
            assert torch.equal(c.after.fin_ids[0, i, :n].cpu(), st.fin_ids[0, i, :n]), w
        assert bool(c.after.unsat[0]) == bool(st.unsat[0])
        assert torch.allclose(c.after.run_score.cpu(), st.run_score, atol=1e-5, rtol=0, equal_nan=True), w
    if kind == "ties":
        assert all(seen.values()), seen


def test_non_finite_logits_stay_in_range(dev):
    """A NaN or +inf logit is outside the contract: the call returns CMB_OK and every index it wrote is in range."""
    B, nb, V = 2, 4, 1000
    gen = torch.Generator().manual_seed(3)
    rows = torch.randn(B * nb, V, generator=gen) * 3
    rows[0, 10] = float("nan")
    rows[1, 20] = float("inf")
    rows[2].fill_(float("-inf"))
    rows[5, ::2] = float("nan")
    embed = torch.zeros(V, H, dtype=torch.bfloat16, device=dev)
    n_tok = torch.ones(B * nb, dtype=torch.int64, device=dev)
    st = BM.BeamState(B, nb, 4)
    st.run_score[:] = -1.0
    for step in (0, 1, 3):
        c = _Call(dev, _padded(rows, V + 5, dev), st, step, 7, embed, n_tok)
        assert bool(((c.parent >= 0) & (c.parent < nb)).all()) and bool(((c.tok >= 0) & (c.tok < V)).all())
        ids = c.after.run_ids[:, :, step].cpu()
        assert bool(((ids >= 0) & (ids < V)).all())


def test_same_bits_twice_and_a_prompt_does_not_depend_on_the_batch(dev):
    B, nb, V, M = 4, 4, 4099, 4
    gen = torch.Generator().manual_seed(8)
    embed = torch.randn(V, H, generator=gen).to(torch.bfloat16).to(dev)
    n_tok = torch.randint(1, 30, (B,), generator=gen).repeat_interleave(nb).to(dev)
    st = BM.BeamState(B, nb, M)
    BM.beam_update(st, torch.randn(B * nb, V, generator=gen) * 3, 0, 5, False)
    rows = torch.randn(B * nb, V, generator=gen) * 3
    logits = _padded(rows, V + 5, dev)
    a = _Call(dev, logits, st, 1, 5, embed, n_tok)
    again = _Call(dev, logits, st, 1, 5, embed, n_tok)
    assert torch.equal(a.state.buf, again.state.buf), "the state block differs between two runs"
    for x, y in ((a.pos, again.pos), (a.kv, again.kv), (a.x, again.x), (a.cos, again.cos), (a.sin, again.sin)):
        assert torch.equal(x, y)
    for b in (0, 2, 3):
        one = BM.BeamState.__new__(BM.BeamState)
        one.__dict__.update({k: v[b:b + 1].clone() for k, v in st.__dict__.items()})
        rs = slice(b * nb, (b + 1) * nb)
        c = _Call(dev, _padded(rows[rs], V + 5, dev), one, 1, 5, embed, n_tok[rs].contiguous())
        assert c.parent[0].tolist() == a.parent[b].tolist() and c.tok[0].tolist() == a.tok[b].tolist()
        for name in ("run_score", "fin_score", "fin_len", "fin_ok", "unsat", "run_ids", "fin_ids"):
            assert torch.equal(getattr(c.after, name)[0], getattr(a.after, name)[b]), (b, name)
        assert torch.equal(c.state.cand_lp, a.state.cand_lp[rs]) and torch.equal(c.x, a.x[rs])


# ---------------------------------------------------------------------------------------------------------------------
# the cache reorder
# ---------------------------------------------------------------------------------------------------------------------
def _cache_plan(dev, layers, R, nkv, Lmax, hd):
    """(desc, table, caches): bf16 caches [R, nkv, Lmax, hd] of random values inside larger allocations (guard elements
    before and after), described the way DecodeStepPlan describes them."""
    from cambrian_amd import lib as L
    n = R * nkv * Lmax * hd
    caches, rows = [], []
    gen = torch.Generator().manual_seed(layers * 100 + R)
    for l in range(layers):
        pair = []
        for kv in range(2):
            # random bf16 bit patterns below the infinities: two rows agree nowhere for long, and no NaN spoils an equality
            full = torch.randint(0, 0x7F00, (n + 128,), dtype=torch.int16, generator=gen).to(dev).view(torch.bfloat16)
            pair.append((full, full[64:64 + n].view(R, nkv, Lmax, hd)))
        row = L.DecodeLayer()
        row.kcache, row.vcache = pair[0][1].data_ptr(), pair[1][1].data_ptr()
        rows.append(row)
        caches.append(pair)
    kc = caches[0][0][1]
    desc = L.DecodeStepDesc(B=R, layers=layers, H=0, I=0, nh=0, nkv=nkv, hd=hd, fp8=0, V=0, eps=0.0, scale=1.0, c_sb=kc.stride(0),
                            c_sh=kc.stride(1), c_st=kc.stride(2))
    return desc, (L.DecodeLayer * layers)(*rows), caches


def test_cache_reorder_moves_the_generated_columns_only(dev):
    ops = _ops()
    layers, nb, nkv, hd, Lmax, L0, t = 3, 4, 2, 64, 40, 9, 14
    R = 2 * nb
    cases = {"swap, one parent three times": [1, 0, 3, 3, 2, 2, 2, 0], "3-cycle and the identity": [1, 2, 0, 3, 0, 1, 2, 3],
             "out of range stays": [0, 7, -1, 2, 3, 2, 1, 0]}
    for name, parent in cases.items():
        desc, table, caches = _cache_plan(dev, layers, R, nkv, Lmax, hd)
        before = [[(full.clone(), view.clone()) for full, view in pair] for pair in caches]
        par = torch.tensor(parent, dtype=torch.int32, device=dev)
        ops.decode_beam_reorder(desc, table, par, nb, L0, t)
        torch.cuda.synchronize()
        src = torch.tensor([(r // nb) * nb + (p if 0 <= p < nb else r % nb) for r, p in enumerate(parent)], device=dev)
        for l in range(layers):
            for kv in range(2):
                full, view = caches[l][kv]
                full0, view0 = before[l][kv]
                want = view0.clone()
                want[:, :, L0:t] = view0[:, :, L0:t].index_select(0, src)
                assert torch.equal(view, want), (name, l, kv)
                assert torch.equal(full[:64], full0[:64]) and torch.equal(full[-64:], full0[-64:]), (name, l, kv, "guards")
        assert not torch.equal(caches[0][0][1], before[0][0][1])
    # nothing to move: t == L0
    desc, table, caches = _cache_plan(dev, layers, R, nkv, Lmax, hd)
    before = [[view.clone() for _, view in pair] for pair in caches]
    ops.decode_beam_reorder(desc, table, torch.tensor(cases["swap, one parent three times"], dtype=torch.int32, device=dev), nb, L0, L0)
    torch.cuda.synchronize()
    assert all(torch.equal(caches[l][kv][1], before[l][kv]) for l in range(layers) for kv in range(2))


def test_decode_beam_reorders_the_caches_by_its_own_parents(dev):
    """The whole call with a cache description: the generated columns follow the parents the call chose."""
    ops = _ops()
    B, nb, V, M, nkv, hd, Lmax, L0 = 2, 4, 1000, 8, 2, 64, 24, 9
    R = B * nb
    gen = torch.Generator().manual_seed(21)
    embed = torch.randn(V, H, generator=gen).to(torch.bfloat16).to(dev)
    n_tok = torch.full((R,), L0, dtype=torch.int64, device=dev)
    st = BM.BeamState(B, nb, M)
    for s in range(3):
        BM.beam_update(st, torch.randn(R, V, generator=gen) * 3, s, None, False)
    step = 3
    rows = torch.randn(R, V, generator=gen) * 3
    desc, table, caches = _cache_plan(dev, 2, R, nkv, Lmax, hd)
    before = [[view.clone() for _, view in pair] for pair in caches]
    state = ops.DecodeBeamState(B, nb, M, dev)
    _load(state, st, step)
    pos = torch.empty(R, dtype=torch.int64, device=dev)
    kv = torch.zeros(R, Lmax, dtype=torch.uint8, device=dev)
    x = torch.empty(R, H, dtype=torch.bfloat16, device=dev)
    cos = torch.empty(R, HD // 2, dtype=torch.float32, device=dev)
    sin = torch.empty_like(cos)
    ops.decode_beam(_padded(rows, V + 5, dev), nb, -1, state, step, n_tok, pos, kv, L0 + step, embed, x, HD, THETA, cos, sin, desc,
                    table, L0)
    torch.cuda.synchronize()
    parent, _ = BM.beam_update(st, rows, step, None, False)
    assert state.parent.view(B, nb).cpu().tolist() == parent.tolist()
    assert not torch.equal(parent, torch.arange(nb)[None].expand(B, nb)), "this seed is here for a reorder"
    src = (parent + torch.arange(B)[:, None] * nb).reshape(-1).to(dev)
    for l in range(2):
        for k in range(2):
            want = before[l][k].clone()
            want[:, :, L0:L0 + step] = before[l][k][:, :, L0:L0 + step].index_select(0, src)
            assert torch.equal(caches[l][k][1], want), (l, k)
    assert int(state.unfinished.item()) == 1


def test_arguments_are_checked_before_any_launch(dev):
    """Host buffers: every case returns before anything is launched, the pointers are never dereferenced.  The documented
    order: state / unfinished / the descriptor pair, cmb_decode_next's rules, the beam rules, the state's size, the caches,
    then alignment."""
    from cambrian_amd import lib as L
    lib = L.load()
    bad_arg, alignment, workspace = -1, -2, -4
    buf = (C.c_double * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    need = lib.cmb_decode_beam_state_bytes(1, 2, 4)
    assert need > 0 and need % 16 == 0 and need <= 8 * 4000
    assert lib.cmb_decode_beam_state_bytes(1, 1, 4) == bad_arg and lib.cmb_decode_beam_state_bytes(2, 9, 4) == bad_arg
    assert lib.cmb_decode_beam_state_bytes(1, 17, 4) == bad_arg and lib.cmb_decode_beam_state_bytes(1, 2, 0) == bad_arg
    assert lib.cmb_decode_beam_state_bytes(8, 2, 4) > lib.cmb_decode_beam_state_bytes(4, 2, 4) > need
    layer = L.DecodeLayer()
    layer.kcache = layer.vcache = p
    table = (L.DecodeLayer * 1)(layer)
    desc = L.DecodeStepDesc(B=2, layers=1, nkv=1, hd=8, c_sb=64, c_sh=64, c_st=8)
    args = dict(logits=p, logits_ld=8, rows=2, num_beams=2, V=8, eos=-1, state=p, state_bytes=need, step=0, max_new=4, n_tok=p, pos=p,
                key_valid=p, kv_ld=4, t=0, embed=p, embed_ld=8, embed_rows=8, H=8, x=p, x_ld=8, hd=4, rope_base=1e4, cos_t=p,
                sin_t=p, d=None, layers=None, L0=0, unfinished=p)

    def call(**over):
        assert not set(over) - set(args), over
        return lib.cmb_decode_beam(*[over.get(k, v) for k, v in args.items()], None)

    for name in ("state", "unfinished", "logits", "n_tok", "pos", "key_valid", "embed", "x", "cos_t", "sin_t"):
        assert call(**{name: None}) == bad_arg, name
        assert call(**{name: None}, rows=0, num_beams=1) == bad_arg, name
    assert call(d=C.byref(desc)) == bad_arg and call(layers=table) == bad_arg            # one of the pair
    for over in (dict(rows=0), dict(rows=17), dict(V=0), dict(V=1 << 31), dict(logits_ld=7), dict(embed_rows=7), dict(eos=-2),
                 dict(eos=8), dict(step=-1), dict(step=4), dict(max_new=0), dict(t=-1), dict(t=4), dict(H=4), dict(H=12),
                 dict(embed_ld=4), dict(x_ld=12), dict(hd=0), dict(hd=3),
                 dict(num_beams=1), dict(num_beams=0), dict(num_beams=17), dict(rows=3), dict(V=1, embed_rows=8),
                 dict(V=1 << 30, logits_ld=1 << 30, embed_rows=1 << 30)):
        assert call(**over) == bad_arg, over
        assert call(**over, embed=p + 2, state_bytes=0) == bad_arg, over                   # sizes before the block and alignment
    assert call(state_bytes=need - 1) == workspace and call(state_bytes=0, embed=p + 8) == workspace
    for field, value in (("B", 4), ("layers", 0), ("nkv", 0), ("hd", 4), ("hd", 12), ("c_sb", -8), ("c_st", 4)):
        d2 = L.DecodeStepDesc(B=2, layers=1, nkv=1, hd=8, c_sb=64, c_sh=64, c_st=8)
        setattr(d2, field, value)
        assert call(d=C.byref(d2), layers=table, t=3, L0=1) == bad_arg, (field, value)
    for over in (dict(L0=-1), dict(L0=4)):
        assert call(d=C.byref(desc), layers=table, t=3, **over) == bad_arg, over
    none = L.DecodeLayer()
    assert call(d=C.byref(desc), layers=(L.DecodeLayer * 1)(none), t=3, L0=1) == bad_arg
    for over in (dict(logits=p + 2), dict(n_tok=p + 4), dict(pos=p + 4), dict(embed=p + 8), dict(x=p + 8), dict(state=p + 8)):
        assert call(**over) == alignment, over
    d3 = L.DecodeStepDesc(B=2, layers=1, nkv=1, hd=8, c_sb=68, c_sh=64, c_st=8)
    assert call(d=C.byref(d3), layers=table, t=3, L0=1) == alignment
    odd = L.DecodeLayer()
    odd.kcache, odd.vcache = p, p + 8
    assert call(d=C.byref(desc), layers=(L.DecodeLayer * 1)(odd), t=3, L0=1) == alignment
    # the reorder entry on its own
    assert lib.cmb_decode_beam_reorder(None, table, p, 2, 1, 3, None) == bad_arg
    assert lib.cmb_decode_beam_reorder(C.byref(desc), table, None, 2, 1, 3, None) == bad_arg
    assert lib.cmb_decode_beam_reorder(C.byref(desc), table, p, 3, 1, 3, None) == bad_arg
    assert lib.cmb_decode_beam_reorder(C.byref(desc), table, p, 2, 4, 3, None) == bad_arg
    assert lib.cmb_decode_beam_reorder(C.byref(desc), table, p + 2, 2, 1, 3, None) == alignment


# ---------------------------------------------------------------------------------------------------------------------
# generate()
# ---------------------------------------------------------------------------------------------------------------------
def _spies(monkeypatch):
    ops = _ops()
    calls = {"beam": 0, "step": 0, "next": 0, "linear": 0, "attention": 0, "index_select": 0, "update": 0}
    from cambrian_amd.model.language_model import cambrian_llama as CL
    for mod, key, name in ((ops, "beam", "decode_beam"), (ops, "step", "decode_step"), (ops, "next", "decode_next"),
                           (ops, "linear", "decode_linear"), (ops, "attention", "decode_attention"),
                           (torch.Tensor, "index_select", "index_select"), (CL, "update", "beam_update")):
        real = getattr(mod, name)

        def counted(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(mod, name, counted)
    return calls


def _run(model, monkeypatch, calls, step_switch, ids, att, **kw):
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", step_switch)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    for k in calls:
        calls[k] = 0
    toks = model.generate(ids, attention_mask=att, **kw)
    torch.cuda.synchronize()
    return toks, dict(calls)


def _host_gap(model, monkeypatch, calls, ids, att, nb, **kw):
    """The per-launch path with the restatement, and the smallest decision gap it met."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    gaps = []
    real = CL.beam_update

    def traced(state, logits, step, eos, last):
        trace = {}
        out = real(state, logits, step, eos, last, trace)
        gaps.append(decision_gap(trace, nb))
        return out

    monkeypatch.setattr(CL, "beam_update", traced)
    try:
        toks, n = _run(model, monkeypatch, calls, "0", ids, att, num_beams=nb, **kw)
    finally:
        monkeypatch.setattr(CL, "beam_update", real)
    return toks, n, min(gaps)


@pytest.mark.parametrize("with_eos", [False, True], ids=["free", "eos"])
@pytest.mark.parametrize("B,nb", [(1, 4), (2, 3)])
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_beam_search_fused_equals_the_per_launch_path(dev, clean_env, lm, B, nb, with_eos):
    """Both paths see the same logits bits (test_generate_greedy_equals_the_per_token_loop), so where no decision of the host
    path was closer than 1e-3 the tokens are equal.  The prompt is the first of eight seeded ones whose gap is that wide."""
    model = _lm(dev, lm)
    calls = _spies(clean_env)
    new = 10
    found = None
    for seed in range(8):
        g = torch.Generator().manual_seed(100 * B + seed)
        ids = torch.randint(1, 64, (B, 9), generator=g).to(dev)
        att = torch.ones(B, 9, dtype=torch.long, device=dev)
        if B > 1:
            att[1, 6:] = 0
        kw = dict(max_new_tokens=new)
        if with_eos:
            free, _, _ = _host_gap(model, clean_env, calls, ids, att, nb, **kw)
            kw["eos_token_id"] = int(free[0, 2])                   # a token the best free hypothesis emits early
            kw["pad_token_id"] = 0
        host, n_host, gap = _host_gap(model, clean_env, calls, ids, att, nb, **kw)
        print(f"{lm} B={B} nb={nb} eos={kw.get('eos_token_id')} seed {seed}: decision gap of the host path {gap:.3e}")
        if gap >= 1e-3:
            found = (ids, att, kw, host, n_host)
            break
    assert found is not None, "no seed of eight leaves every decision of the host path 1e-3 wide"
    ids, att, kw, host, n_host = found
    assert n_host["beam"] == 0 and n_host["step"] == 0 and n_host["update"] >= 1 and n_host["next"] == 0, n_host
    fused, n = _run(model, clean_env, calls, "1", ids, att, num_beams=nb, **kw)
    assert fused.dtype == torch.int64 and fused.shape[0] == B and 1 <= fused.shape[1] <= new
    assert fused.tolist() == host.tolist(), (fused.tolist(), host.tolist())
    assert n["update"] == 0 and n["index_select"] == 0 and n["next"] == 0 and n["linear"] == 0 and n["attention"] == 0, n
    assert n["step"] == n["beam"] - 1 and 1 <= n["beam"] <= new, n
    if not with_eos:
        assert n["beam"] == new and fused.shape[1] == new, n
    else:
        assert n["beam"] == new or n["beam"] % _ops().DECODE_STEP_POLL == 0, n
        assert n["beam"] <= min(new, -(-n_host["update"] // 8) * 8), (n, n_host)      # on to the next poll, no further
    # the switch from the config, and the environment over it
    clean_env.delenv("CAMBRIAN_AMD_DECODE_BEAM")
    model.config.decode_beam_search = True
    try:
        assert torch.equal(model.generate(ids, attention_mask=att, num_beams=nb, **kw), fused)
        clean_env.setenv("CAMBRIAN_AMD_DECODE_BEAM", "0")
        with pytest.raises(NotImplementedError, match="num_beams"):
            model.generate(ids, attention_mask=att, num_beams=nb, **kw)
    finally:
        model.config.decode_beam_search = False


def test_generate_equals_the_recorded_hf_beam_search(dev, clean_env):
    """The fixture model (tests/golden/beam_cases.pt) in fp32 through ``generate()``: HF's recorded tokens, on cases whose
    every decision is at least 1e-3 wide (fp32 logits of two implementations differ by about 1e-5)."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    fx = load_beam_fixture()
    cfg = CL.CambrianConfig(**fx["config"])
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.float32)
    missing, unexpected = model.load_state_dict({k: v.float() for k, v in fx["state"].items()}, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(("model.layers", "model.embed", "model.norm", "lm_head"))]
    model.requires_grad_(False)
    model.eval()
    clean_env.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    for c in fx["cases"]:
        got = model.generate(c["prompts"].to(dev), num_beams=c["num_beams"], max_new_tokens=c["max_new"], eos_token_id=c["eos"],
                             pad_token_id=0)
        assert got.cpu().tolist() == c["tokens"].tolist(), (c["num_beams"], c["eos"], got.tolist(), c["tokens"].tolist())


def _by_hand(model, ids, att, nb, new, eos):
    """The host loop restated for the test: prefill, then beam.py around ``layer.decode`` and an ``index_select`` of the WHOLE
    caches per step."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    ops = _ops()
    m = model.model
    dev = ids.device
    B, L = ids.shape
    with torch.no_grad():
        valid = att.bool()
        pos = (valid.long().cumsum(1) - 1).clamp_min(0)
        kv_out = []
        hidden = m(m.embed_tokens(ids).to(m.llm_dtype), pos, att, None, kv_out=kv_out)
        last = valid.long().sum(1) - 1
        logits = model.lm_head(hidden[torch.arange(B, device=dev), last]).float().repeat_interleave(nb, 0)
        a0 = m.layers[0].self_attn
        Lmax = L + new
        caches = []
        for k, v in kv_out:
            kc = torch.zeros(B * nb, a0.nkv, Lmax, a0.hd, dtype=k.dtype, device=dev)
            vc = torch.zeros_like(kc)
            kc[:, :, :L], vc[:, :, :L] = k.repeat_interleave(nb, 0), v.repeat_interleave(nb, 0)
            caches.append([kc, vc])
        mask = torch.zeros(B * nb, Lmax, dtype=torch.bool, device=dev)
        mask[:, :L] = valid.repeat_interleave(nb, 0)
        n_tok = valid.long().sum(1).repeat_interleave(nb)
        st = BM.BeamState(B, nb, new, dev)
        for step in range(new):
            parent, tok = BM.beam_update(st, logits, step, eos, step + 1 == new)
            if step + 1 == new or BM.beam_done(st):
                break
            src = (parent + torch.arange(B, device=dev)[:, None] * nb).reshape(-1)
            for pair in caches:
                pair[0], pair[1] = pair[0].index_select(0, src), pair[1].index_select(0, src)
            t = L + step
            mask[:, t] = True
            cos, sin = ops.rope_table((n_tok + step)[:, None], a0.hd, float(model.config.rope_theta))
            x = m.embed_tokens(tok.reshape(-1))[:, None, :].to(m.llm_dtype)
            for layer, (kc, vc) in zip(m.layers, caches):
                x = layer.decode(x, cos, sin, kc, vc, t, mask)
            logits = CL._decode_logits(model, x)
        return BM.beam_result(st, BM.beam_fill(0, eos))


@pytest.mark.parametrize("why", ["fp32", "rows17", "step_off"])
def test_outside_the_conditions_beam_search_runs_on_the_host_path(dev, clean_env, why):
    model = _lm(dev, "llama", dt=torch.float32 if why == "fp32" else torch.bfloat16)
    calls = _spies(clean_env)
    B, nb = (1, 17) if why == "rows17" else (2, 3)
    ids, att = _prompt(dev, B)
    want = _by_hand(model, ids, att, nb, 6, 11)
    got, n = _run(model, clean_env, calls, "0" if why == "step_off" else "1", ids, att, num_beams=nb, max_new_tokens=6,
                  eos_token_id=11, pad_token_id=0)
    assert got.tolist() == want.tolist(), why
    assert n["beam"] == 0 and n["step"] == 0 and n["update"] >= 1, (why, n)


def test_with_the_switch_off_beam_search_still_raises(dev, clean_env):
    model = _lm(dev, "llama")
    ids, att = _prompt(dev, 1)
    for value in (None, "0"):
        if value is not None:
            clean_env.setenv("CAMBRIAN_AMD_DECODE_BEAM", value)
        with pytest.raises(NotImplementedError, match="num_beams"):
            model.generate(ids, attention_mask=att, num_beams=4, max_new_tokens=3)
    clean_env.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    with pytest.raises(NotImplementedError, match="do_sample"):
        model.generate(ids, attention_mask=att, num_beams=4, max_new_tokens=3, do_sample=True)
    assert model.generate(ids, attention_mask=att, num_beams=4, max_new_tokens=3).shape == (1, 3)
