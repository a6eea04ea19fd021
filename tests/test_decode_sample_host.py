"""CPU: the host side of device sampling (``cmb_decode_sample``) and its restatement in numpy.

* ``ops.decode_sample_enabled``: environment over config, off by default.
* ``_sample_fused`` raises ``filter_logits_top_k_top_p``'s ValueError for ``top_p <= 0`` before anything is launched.
* ``sample_reference``: steps 1-5 of the kernel's definition (include/cambrian_amd.h) over the exact integer Philox4x32-10,
  exact fp32 ``z`` and float64 masses and scores.  tests/test_decode_sample_gpu.py imports it.
* the distribution of the restatement's draws (Pearson chi-square against the softmax), for the seed the GPU test uses AND the
  next two, so that the seed is not hand-picked.
"""
import math

import numpy as np
import pytest
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable integer arrays; returns the four output words as uint64 arrays (values < 2^32)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def gumbel_noise(seed: int, V: int, rows, steps):
    """float64 g [len(rows), len(steps), V]: element i takes word i & 3 of the counter (i >> 2, row, step, 0) under the key
    (seed low, seed high); u = ((word >> 8) + 0.5) * 2^-24, g = -log(-log u)."""
    seed &= (1 << 64) - 1
    groups = np.arange((V + 3) // 4, dtype=np.uint64)
    r = np.asarray(rows, dtype=np.uint64)[:, None, None]
    s = np.asarray(steps, dtype=np.uint64)[None, :, None]
    words = np.stack(philox4x32_10(groups[None, None, :], r, s, 0, seed & 0xFFFFFFFF, seed >> 32), axis=-1)
    words = words.reshape(words.shape[0], words.shape[1], -1)[:, :, :V]
    u = ((words >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def sample_filter(logits_row, inv_temperature, top_k: int, top_p: float):
    """Steps 1-4 for one row: dict(z fp32, argmax (int) when the maximum is not finite else None, keep (bool [V]), thr, n_keep,
    margin).  ``margin``: how far 1 - top_p is, in units of Z, from the nearest cumulative mass at which the cut would move
    (inf without top-p)."""
    l = np.asarray(logits_row, dtype=np.float32)
    V = l.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        z = l * np.float32(inv_temperature)                          # one fp32 multiply
    out = dict(z=z, argmax=None, keep=None, thr=float("nan"), n_keep=0, margin=float("inf"))
    nan = np.isnan(l)
    if nan.any():
        out["argmax"] = int(np.argmax(nan))                          # the first NaN (torch.argmax's rule)
        return out
    if not np.isfinite(l.max()) or not np.isfinite(z.max()):
        out["argmax"] = int(np.argmax(l))                            # the lowest index among equals
        return out
    keep = np.ones(V, dtype=bool)
    thr = float("-inf")
    if top_k > 0:
        thr = float(np.sort(z)[V - min(top_k, V)])                   # the k-th largest; ties at it are kept
        keep = z >= np.float32(thr)
    p = float(np.float32(top_p))                                     # the kernel is handed an fp32
    if p < 1.0:
        z64 = z.astype(np.float64)
        w = np.where(keep, np.exp(z64 - z64.max()), 0.0)
        Z = w.sum()
        order = np.argsort(z, kind="stable")
        csum = np.cumsum(w[order])                                   # dropped elements weigh nothing
        vals = np.unique(z[keep])                                    # ascending
        cum = csum[np.searchsorted(z[order], vals, side="right") - 1] / Z      # mass of the kept elements with z <= v
        cum[-1] = 1.0
        j = int(np.argmax(cum > 1.0 - p))                            # the smallest value whose mass from below exceeds
        thr = float(vals[j])
        keep = keep & (z >= vals[j])
        below = cum[j - 1] if j > 0 else 0.0
        out["margin"] = float(min(cum[j] - (1.0 - p), (1.0 - p) - below))
    out.update(keep=keep, thr=thr, n_keep=int(keep.sum()))
    return out


def sample_reference(logits_row, inv_temperature, top_k: int, top_p: float, seed: int, b: int, step: int):
    """Steps 1-5 for row ``b`` at draw ``step``: ``sample_filter``'s dict plus id and the float64 scores s (-inf outside the
    kept set)."""
    out = sample_filter(logits_row, inv_temperature, top_k, top_p)
    if out["argmax"] is not None:
        out.update(id=out["argmax"], s=None)
        return out
    g = gumbel_noise(seed, out["z"].shape[0], [b], [step])[0, 0]
    with np.errstate(invalid="ignore"):
        s = np.where(out["keep"], out["z"].astype(np.float64) + g, -np.inf)
    out.update(id=int(np.argmax(s)), s=s)
    return out


def chi_square_bound(df: int, zq: float = 3.0902) -> float:
    """The 99.9 % quantile of chi-square with ``df`` degrees of freedom by Wilson-Hilferty."""
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + zq * math.sqrt(a)) ** 3


def chi_square(ids, probs, n: int):
    """(Pearson chi-square of the counts of ``ids`` against ``n * probs``, degrees of freedom): bins in ascending order of
    expectation are merged until each expects at least 5."""
    counts = np.bincount(np.asarray(ids).ravel(), minlength=len(probs)).astype(np.float64)
    order = np.argsort(probs, kind="stable")
    exp_bins, obs_bins, e, o = [], [], 0.0, 0.0
    for i in order:
        e += n * probs[i]
        o += counts[i]
        if e >= 5.0:
            exp_bins.append(e)
            obs_bins.append(o)
            e = o = 0.0
    if e > 0.0 or o > 0.0:                                           # what is left joins the last bin
        exp_bins[-1] += e
        obs_bins[-1] += o
    ex, ob = np.array(exp_bins), np.array(obs_bins)
    return float(((ob - ex) ** 2 / ex).sum()), len(ex) - 1


DIST_V, DIST_ROWS, DIST_STEPS, DIST_SEED = 64, 16, 256, 1


def distribution_logits():
    """fp32 [64]: the row every distribution check uses (a fixed numpy stream; flat enough that most bins expect >= 5)."""
    return (np.random.default_rng(2024).standard_normal(DIST_V) * 1.5).astype(np.float32)


def reference_draws(z_row, keep, seed: int):
    """ids [DIST_ROWS, DIST_STEPS] of the restatement for identical rows ``z_row`` with the kept set ``keep``."""
    g = gumbel_noise(seed, DIST_V, range(DIST_ROWS), range(DIST_STEPS))
    s = np.where(keep[None, None, :], z_row.astype(np.float64)[None, None, :] + g, -np.inf)
    return np.argmax(s, axis=-1)


def check_distribution(ids, z_row, keep):
    """The assertions of the distribution check on ids [rows, steps]; returns (chi-square, degrees of freedom, bound)."""
    ids = np.asarray(ids)
    assert keep[ids].all(), "an id outside the kept set was drawn"
    w = np.where(keep, np.exp(z_row.astype(np.float64) - float(z_row.max())), 0.0)
    chi, df = chi_square(ids, w / w.sum(), ids.size)
    bound = chi_square_bound(df)
    print(f"chi-square {chi:.1f} at {df} degrees of freedom, bound {bound:.1f}")
    assert chi <= bound, (chi, df, bound)
    assert len({tuple(r) for r in ids.tolist()}) > 1, "every row drew the same sequence: the row index does not reach the counter"
    return chi, df, bound


@pytest.mark.parametrize("seed", [DIST_SEED, DIST_SEED + 1, DIST_SEED + 2])
@pytest.mark.parametrize("top_k", [0, 8])
def test_restatement_draws_follow_the_softmax(seed, top_k):
    l = distribution_logits()
    f = sample_filter(l, 1.0, top_k, 1.0)
    assert f["n_keep"] == (top_k or DIST_V)
    _, df, _ = check_distribution(reference_draws(f["z"], f["keep"], seed), f["z"], f["keep"])
    assert df >= (5 if top_k else 30), "too few bins left for the check to mean anything"


def test_philox_known_answers():
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == want


def test_filter_rules_of_the_restatement():
    """The rules that differ from, or pin down, HF's warpers: ties at the k-th value are kept; equal values at the nucleus cut
    stay together; top_p keeps the smallest sufficient set (0.8 / 0.81 around a mass of exactly 0.8); non-finite maxima."""
    l = np.log(np.array([0.5, 0.3, 0.1, 0.1], dtype=np.float64)).astype(np.float32)
    assert sample_filter(l, 1.0, 3, 1.0)["n_keep"] == 4                       # two tied at third place
    assert sample_filter(l, 1.0, 2, 1.0)["n_keep"] == 2 and sample_filter(l, 1.0, 9, 1.0)["n_keep"] == 4
    assert sample_filter(l, 1.0, 0, 0.79)["n_keep"] == 2                      # {0.5, 0.3} reaches 0.8 > 0.79
    assert sample_filter(l, 1.0, 0, 0.81)["n_keep"] == 4                      # the two 0.1 come or go together
    assert sample_filter(l, 1.0, 0, 1e-6)["n_keep"] == 1 and sample_filter(l, 1.0, 0, 1.0)["n_keep"] == 4
    assert sample_filter(l, 1.0, 1, 0.99)["n_keep"] == 1
    f = sample_filter(l, 1.0, 0, 1.0)
    assert f["thr"] == float("-inf") and f["margin"] == float("inf")
    nan = np.array([0.0, float("inf"), float("nan"), float("nan")], dtype=np.float32)
    assert sample_reference(nan, 1.0, 0, 1.0, 1, 0, 0)["id"] == 2
    assert sample_reference(np.array([0, np.inf, np.inf], dtype=np.float32), 1.0, 0, 1.0, 1, 0, 0)["id"] == 1
    assert sample_reference(np.full(5, -np.inf, dtype=np.float32), 1.0, 0, 1.0, 1, 0, 0)["id"] == 0
    assert sample_reference(np.array([1e38, 2e38], dtype=np.float32), 2.0, 0, 1.0, 1, 0, 0)["id"] == 1     # z_max overflows
    # against the torch warpers where no tie sits on a cut
    from cambrian_amd.model.language_model.cambrian_llama import filter_logits_top_k_top_p
    g = torch.Generator().manual_seed(0)
    for k, p in ((0, 0.9), (20, 1.0), (20, 0.5), (50, 0.9)):
        row = torch.randn(1, 1000, generator=g) * 3
        want = torch.isfinite(filter_logits_top_k_top_p(row / 0.7, k, p))[0].numpy()
        got = sample_filter(row[0].numpy(), np.float32(1 / 0.7), k, p)
        assert got["margin"] > 1e-6 and (got["keep"] == want).all(), (k, p)


def test_switch_resolution(monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_SAMPLE", raising=False)
    assert ops.decode_sample_enabled() is False and ops.decode_sample_enabled(False) is False
    assert ops.decode_sample_enabled(True) is True
    for value, flag, want in (("1", False, True), ("0", True, False), ("", True, True), ("", False, False)):
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_SAMPLE", value)
        assert ops.decode_sample_enabled(flag) is want, (value, flag)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_SAMPLE", "1")
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_STEP", raising=False)
    assert ops.decode_step_enabled() is False, "the sample switch must not turn the step switch on"


@pytest.mark.parametrize("top_p", [0.0, -0.5])
def test_top_p_out_of_range_raises_before_any_launch(monkeypatch, top_p):
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL

    def launched(*a, **kw):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(ops, "decode_sample", launched)
    monkeypatch.setattr(torch, "randint", launched)
    logits = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="`top_p` has to be a float > 0 and <= 1"):
        CL._sample_fused(None, None, logits, None, None, 4, 3, None, 64, 1e4, 0.7, 5, top_p)
    with pytest.raises(ValueError, match="`top_p` has to be a float > 0 and <= 1"):     # the message of the torch warper
        CL.filter_logits_top_k_top_p(logits, 5, top_p)
