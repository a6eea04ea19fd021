"""No GPU: the per-tile attention checker (tests/attn_check.py) has teeth.  For every input family and output, the block error
of the bf16 twin (legal rounding) and of the mutants (a)-(g) (wrong results) against the fp64 reference, at S = 512, B = 1,
H = 2, HKV = 1, D = 128 — mutant (e), the wrong KV head, at H = 4, HKV = 2: with one KV head h % HKV and h // group agree.
TOL[family][output] has to sit at 3 x the twin's error or above and at half the error of the mutants in CATCHES or below.

Measured here (block_err; lse: lse_err), twin = the larger of the causal and the key-padded run:
            o        lse      dq      dk      dv
gauss  twin 0.0024   3.6e-8   0.0033  0.0028  0.0026    fp32 logsumexp 8.0e-8   TOL 0.009 6.4e-7 0.015 0.015 0.010
       a    0.13     1.6e-2   0.15    0.097   0.11
       b    0.060    8.3e-3   0.19    0.16    0.072
       c    0.59     5.4e-2   0.58    0.44    0.46
       d    0        0        0       1       1
       e    1.5      0.47     1.6     1.2     1.3
       f    0.58     5.7e-2   0.57    0.66    0.70
       g    0.79     0.38     0.27    0.58    0.63
peaked twin 0.0018   3.5e-8   0.033   0.020   0.0029    fp32 logsumexp 1.6e-7   TOL 0.009 1.3e-6 -     -     0.012
       a    0.096    3.6e-2   0.088   0.019   0.10
       b    0.0017   4.5e-4   0.0074  0.0020  0.0022    (lse only)
       c    0.25     0.23     0.93    0.58    0.56
       d    0        0        0       1       1
       e    0.57     0.72     2.0     2.8     65
       f    0.27     0.36     1.1     0.89    0.86
       g    0.58     0.55     0.63    0.94    0.74
diag   twin 0.0017   4.9e-8   1.4     0.20    0.0023    fp32 logsumexp 3.2e-7   TOL 0.008 2.6e-6 -     -     0.010
       a    0.11     0.50     1.4     1.2     0.28
       b    0.0007   4.9e-4   0.092   0.021   0.0010    (lse only)
       c    0.014    7.3e-3   0.23    0.25    0.032
       d    0        0        0       1       1
       e    0.53     1.0      129     18      0.83
       f    0.0059   2.8e-3   0.18    0.23    0.012     (lse only)
       g    0.61     0.96     74      14      0.81
"""
import functools

import pytest
import torch

import attn_check as A

S, D = 512, 128


@functools.lru_cache(maxsize=None)
def _measure(family):
    """{'twin': {output: err}, 'lse32': err, mutant: {output: err}} for one family."""
    def errs(got, ref):
        return {n: (A.lse_err(x, r) if n == "lse" else A.block_err(x, r)) for n, x, r in zip(A.OUTPUTS, got, ref)}

    q, k, v, w = A.inputs(family, 1, 2, 1, S, D, seed=1)
    out = {"twin": dict.fromkeys(A.OUTPUTS, 0.0), "lse32": 0.0}
    for allow, muts in ((A.causal_allow(S), "abcd"), (A.causal_allow(S, A.mutant_key_valid(1, S)), "fg")):
        ref = A.reference(q, k, v, w, allow)
        tw = errs(A.twin(q, k, v, w, allow), ref)
        out["twin"] = {n: max(out["twin"][n], tw[n]) for n in A.OUTPUTS}
        out["lse32"] = max(out["lse32"], A.lse_fp32_err(q, k, allow))
        for m in muts:
            out[m] = errs(A.mutant(m, q, k, v, w), ref)
    q, k, v, w = A.inputs(family, 1, 4, 2, S, D, seed=2)
    ref = A.reference(q, k, v, w, A.causal_allow(S))
    tw = errs(A.twin(q, k, v, w, A.causal_allow(S)), ref)
    out["twin"] = {n: max(out["twin"][n], tw[n]) for n in A.OUTPUTS}
    out["e"] = errs(A.mutant("e", q, k, v, w), ref)
    for row in ("twin",) + A.MUTANTS:
        print(f"{family:6s} {row:4s} " + " ".join(f"{n}={out[row][n]:.3g}" for n in A.OUTPUTS)
              + (f"  fp32-logsumexp={out['lse32']:.3g}" if row == "twin" else ""))
    return out


@pytest.mark.parametrize("family", A.FAMILIES)
def test_tolerances_sit_between_twin_and_mutants(family):
    m = _measure(family)
    for name in A.OUTPUTS:
        tol = A.TOL[family][name]
        if name == "lse":
            # 8 x the error of an fp32 logsumexp of fp32 scores (within the spread of one measurement: [6, 12] x)
            assert tol is not None and 6.0 * m["lse32"] <= tol <= 12.0 * m["lse32"], (family, tol, m["lse32"])
            assert m["twin"]["lse"] <= tol
        elif name in ("dq", "dk") and m["twin"][name] > 1e-2:
            assert tol is None and family != "gauss", (family, name, m["twin"][name])   # ill-conditioned: not checked
            continue
        else:
            assert tol is not None and 3.0 * m["twin"][name] <= tol, (family, name, tol, m["twin"][name])
        caught = A.CATCHES[(family, name)]
        assert caught, (family, name)
        for mut in caught:
            assert tol <= 0.5 * m[mut][name], (family, name, mut, tol, m[mut][name])
    assert all(A.TOL["gauss"][n] is not None for n in A.OUTPUTS)
    assert all(A.TOL[family][n] is None or (family, n) in A.CATCHES for n in A.OUTPUTS)


def test_every_mutant_is_rejected():
    for mut in A.MUTANTS:
        pairs = [fo for fo, muts in A.CATCHES.items() if mut in muts]
        assert pairs, f"mutant {mut}: no (family, output) pair is meant to catch it"
        # and by a BLOCK error, not only by the log-sum-exp (d has no forward error at all)
        assert any(o != "lse" and _measure(f)[mut][o] > A.TOL[f][o] for f, o in pairs), mut
        for f, o in pairs:
            assert _measure(f)[mut][o] > A.TOL[f][o], (mut, f, o)


def _twin_ok(family, q, k, v, w, allow, scale, label, zero_ok=False, skip=()):
    ref = A.reference(q, k, v, w, allow, scale)
    tw = A.twin(q, k, v, w, allow, scale)
    for name, x, r in zip(A.OUTPUTS, tw, ref):
        tol = A.TOL[family][name]
        if tol is None or name in skip:
            continue
        err = A.lse_err(x, r) if name == "lse" else A.block_err(x, r, zero_ok=zero_ok)
        assert 3.0 * err <= tol if name != "lse" else err <= tol, f"{label} {family} {name}: twin {err:.3g}, TOL {tol}"


@pytest.mark.parametrize("family", A.FAMILIES)
def test_twin_passes_at_every_gpu_case(family):
    """3 x twin <= TOL at the shapes, head groupings and masks test_flash_tiles_gpu.py runs, not only at S = 512."""
    for H, HKV in A.CAUSAL_HEADS:
        for s_ in A.CAUSAL_S:
            q, k, v, w = A.inputs(family, 1, H, HKV, s_, D, seed=s_ + H)
            _twin_ok(family, q, k, v, w, A.causal_allow(s_), None, f"causal S={s_} H={H}/{HKV}")
    for name in A.MASK_NAMES:
        q, k, v, w = A.inputs(family, 2, 4, 1, A.MASK_S, D, seed=7)
        allow = A.causal_allow(A.MASK_S, A.key_valid_mask(name, 2, A.MASK_S))
        _twin_ok(family, q, k, v, w, allow, None, f"mask {name}", zero_ok=True)
    if family == "gauss":
        for hd in A.VIT_HD:
            for n in A.VIT_N:
                q, k, v, w = A.inputs(family, 1, 2, 2, n, hd, seed=n + hd, scale=hd ** -0.5)
                allow = torch.ones(1, 1, n, n, dtype=torch.bool)
                # one token: o = v, dq = dk = 0 exactly (dS = P (dP - D) = 0): nothing for a relative error to divide by
                _twin_ok(family, q, k, v, w, allow, hd ** -0.5, f"vit N={n} hd={hd}", skip=("dq", "dk") if n == 1 else ())


def test_global_max_metric_accepts_tile_mutants():
    """The record of why attn_check exists: at S = 1024 on Gaussian data the metric of test_flash_bwd_gpu.py (one maximum per
    tensor, < 2e-2 forward, < 3e-2 gradients) accepts mutant (a) in the forward and mutant (d) in dk and dv, which the block
    error rejects at twice its tolerance and more."""
    s_ = 1024
    q, k, v, w = A.inputs("gauss", 1, 2, 1, s_, D, seed=3)
    ref = A.reference(q, k, v, w, A.causal_allow(s_))
    ma, md = A.mutant("a", q, k, v, w), A.mutant("d", q, k, v, w)
    old_a, old_dk, old_dv = A.global_max_err(ma[0], ref[0]), A.global_max_err(md[3], ref[3]), A.global_max_err(md[4], ref[4])
    new_a, new_dk, new_dv = A.block_err(ma[0], ref[0]), A.block_err(md[3], ref[3]), A.block_err(md[4], ref[4])
    print(f"S=1024 global-max metric: (a) o {old_a:.3g}, (d) dk {old_dk:.3g} dv {old_dv:.3g};"
          f" block error: (a) o {new_a:.3g}, (d) dk {new_dk:.3g} dv {new_dv:.3g}")
    assert old_a < 2e-2 and old_dk < 3e-2 and old_dv < 3e-2
    assert new_a > 2 * A.TOL["gauss"]["o"] and new_dk > 2 * A.TOL["gauss"]["dk"] and new_dv > 2 * A.TOL["gauss"]["dv"]


def test_block_err_edges():
    ref = torch.ones(1, 1, 40, 4)
    a = ref.clone()
    a[0, 0, 39] = 0                                     # the 8-row remainder joins the last block: rows 16..39
    assert A.block_errs(a, ref).shape == (1, 1, 2)
    assert abs(A.block_err(a, ref) - (4 / 96) ** 0.5) < 1e-12
    assert A.block_errs(ref[:, :, :5], ref[:, :, :5]).shape == (1, 1, 1)      # fewer than 16 rows: one block
    z = ref.clone()
    z[0, 0, :16] = 0
    with pytest.raises(AssertionError):
        A.block_err(z, z)
    assert A.block_err(z, z, zero_ok=True) == 0.0
    a = z.clone()
    a[0, 0, 0, 0] = float("nan")
    assert A.block_err(a, z, zero_ok=True) == float("inf")
