"""Per-tile checks for the attention kernels (flash_bwd.hip, flash2.hip; ops.causal_attention, ops.vit_attention).

Plain device-agnostic torch, no pytest in here: the host test (test_attn_check_host.py) runs it on the CPU to show that the
metric and the tolerances below separate a legitimately rounded result from a wrong one, the GPU tests
(test_flash_tiles_gpu.py, test_flash_bwd_gpu.py) run it on the device against the kernels.

Why: `max|a - ref| / max|ref|` over a whole tensor of causal attention on Gaussian data is set by the first rows (|o| ~ 3
where a row averages a few keys, ~ 1/sqrt(row) later on), so a wrong LATE tile is divided by a maximum it has no part in.
Measured in fp64 at D = 128: dK or dV of the last 64 keys all zero, or row r blind to key r whenever r % 64 == 0, pass the
2e-2 / 3e-2 bounds at S = 1024 (test_attn_check_host.py::test_global_max_metric_accepts_tile_mutants keeps the figures).

Pieces:
  reference()   fp64 softmax(Q K^T scale + mask) V with grouped KV heads and its analytic backward, dense boolean mask
  twin()        the same formula with the kernels' bf16 roundings: ONE model of legal rounding, the only thing TOL comes from
  block_err()   max over (batch, head, block of 16 rows) of ||a - ref||_F / ||ref||_F: finer than any kernel tile (64 / 128)
  lse_err()     max |a - ref| / max(1, max |ref|) for the fp32 log-sum-exp
  inputs()      the families gauss / peaked / diag, rounded to bf16
  mutant()      wrong results (a)-(g) made from the reference, to show what the metric rejects
  TOL, CATCHES  tolerance per (family, output) and the mutants each pair is meant to reject

Teeth check by hand (scratch copy of the library, not part of the suite): in flash2.hip apply_mask, line 121, replace
`key <= qi` by `key <= qi - (!MASKED && qi >= 512 && (qi & 63) == 0)` (the default forward; the same line in
flash_bwd.hip:161 for the knob values without bit 0).  In the causal kernels without a key-padding mask a row r >= 512 then
misses key r at every 64-key tile edge.  Tried on an MI355X: every assertion test_flash_bwd_gpu.py had before the block checks
still passes (global-maximum metric of o 0.005 at S = 2048, 0.009-0.018 at S = 1024 against 2e-2 in the fp64 simulation of the
edit, simulate_forward_edit(); S = 256 and 384 are not touched), while test_causal_tiles fails at S = 640 for every head
grouping — block_err of o 0.027 / 0.033 on `gauss` (TOL 0.009), 0.10-0.11 on `diag` (TOL 0.008), dv on `diag` 1.3-2.0 (TOL
0.010), lse_err 6e-5 to 0.25 against 6.4e-7 to 2.6e-6 — and so do the block checks of the S = 2048 and the every-variant test
(o 0.077 at S = 1024).  The simulation gives the same figures to three digits.  Without `!MASKED &&` the old key-padding test
notices too, just (0.0201 against 2e-2 at S = 1024): padding leaves a row fewer keys to share its weight with.
"""
import math

import torch

ROWS = 16


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _same(x):
    return x


def _core(q, k, v, w, allow, scale, kv_of_head, rnd, allow_fwd=None):
    """q, w [B,H,S,D], k, v [B,HKV,S,D], allow bool broadcastable to [B,H,S,S] -> fp64 (o, lse, dq, dk, dv).  ``rnd`` is the
    identity (reference) or a bf16 round trip (twin) applied where the kernels round; a row with no visible key gives o = 0,
    lse = 0 and no gradient (mutants only).  ``allow_fwd``: the mask of the forward alone, for simulate_forward_edit()."""
    B, H, S, D = q.shape
    HKV = k.shape[1]
    scale = D ** -0.5 if scale is None else float(scale)
    if kv_of_head is None:
        kv_of_head = [h // (H // HKV) for h in range(H)]
    idx = torch.as_tensor(kv_of_head, device=q.device)
    allow = allow.to(q.device).expand(B, H, S, S)
    allow_fwd = allow if allow_fwd is None else allow_fwd.to(q.device).expand(B, H, S, S)
    f64 = dict(dtype=torch.float64, device=q.device)
    o, lse = torch.empty(B, H, S, D, **f64), torch.empty(B, H, S, **f64)
    dq, dk, dv = torch.empty(B, H, S, D, **f64), torch.empty(B, HKV, S, D, **f64), torch.empty(B, HKV, S, D, **f64)
    for b in range(B):   # one sample at a time: [H,S,S] fp64 temporaries, not [B,H,S,S]
        qd, ke, ve = q[b].double(), k[b].double()[idx], v[b].double()[idx]
        # dO: the upstream gradient arrives as bf16 (autograd casts it to the dtype of the bf16 output, ops.py:2096)
        do = rnd(w[b].double())
        s0 = qd @ ke.transpose(-1, -2) * scale
        s = s0.masked_fill(~allow_fwd[b], float("-inf"))
        m = s.amax(-1, keepdim=True)
        empty = torch.isinf(m)
        m = torch.where(empty, torch.zeros_like(m), m)
        e = torch.exp(s - m)
        # the row sum takes the UNROUNDED exponentials (flash_bwd.hip:194 `l += pv` before the conversion; flash2.hip:165)
        ell = torch.where(empty, torch.ones_like(m), e.sum(-1, keepdim=True))
        # exp(s - m) -> bf16 as the operand of the PV product (flash_bwd.hip:200 cvt8; flash2.hip:186, 202 cvt2_bf16);
        # O -> bf16 on the store (flash_bwd.hip:223; flash2.hip:251)
        ob = rnd(rnd(e) @ ve / ell)
        lb = (m + torch.log(ell)).squeeze(-1)
        if rnd is not _same:
            lb = lb.float().double()          # lse is an fp32 output (flash_bwd.hip:226; flash2.hip:254)
        # backward: P recomputed from the stored lse (flash_bwd.hip:335, 537-539; flash2.hip:395)
        sb = s0.masked_fill(~allow[b], float("-inf"))
        p = torch.exp(sb - lb[..., None])
        dp = do @ ve.transpose(-1, -2)
        dd = (do * ob).sum(-1, keepdim=True)  # D = rowsum(dO * O) from the bf16 O in fp32 (flash_bwd.hip:270)
        ds = p * (dp - dd)                    # without the 1/sqrt(d) factor, as the kernels hold it (flash_bwd.hip:336, 556)
        # dS -> bf16 before dQ += K^T dS (flash_bwd.hip:340; flash2.hip:397); dQ * scale -> bf16 (flash_bwd.hip:369; flash2.hip:434)
        dq[b] = rnd(rnd(ds) @ ke * scale)
        # P, dS -> bf16 before dV += dO^T P and dK += Q^T dS (flash_bwd.hip:560, 561 and 636, 637, 666, 667 of the four-phase
        # body); the query heads of a group add up in the fp32 accumulators (loop over hq, :487), dK * scale and dV -> bf16 (:708, :709)
        dv_e = rnd(p).transpose(-1, -2) @ do
        dk_e = rnd(ds).transpose(-1, -2) @ qd * scale
        dv[b] = rnd(torch.zeros(HKV, S, D, **f64).index_add_(0, idx, dv_e))
        dk[b] = rnd(torch.zeros(HKV, S, D, **f64).index_add_(0, idx, dk_e))
        o[b], lse[b] = ob, lb
    return o, lse, dq, dk, dv


def reference(q, k, v, w, allow, scale=None, kv_of_head=None):
    """fp64 attention and its analytic backward for the upstream gradient ``w``: (o, lse, dq, dk, dv)."""
    return _core(q, k, v, w, allow, scale, kv_of_head, _same)


def twin(q, k, v, w, allow, scale=None):
    """reference() with a bf16 rounding at every point where the kernels round (cited in _core)."""
    return _core(q, k, v, w, allow, scale, None, _bf)


def simulate_forward_edit(q, k, v, w, allow, allow_fwd, scale=None):
    """What a forward kernel with the mask ``allow_fwd`` followed by correct backward kernels returns, in fp64."""
    return _core(q, k, v, w, allow, scale, None, _same, allow_fwd=allow_fwd)


def _segments(x, rows):
    """[B,H,S] -> [B,H,nblocks]: sums over blocks of ``rows`` consecutive rows; a remainder joins the last block, and a
    tensor shorter than ``rows`` is one block."""
    S = x.shape[-1]
    nb = S // rows
    if nb == 0:
        return x.sum(-1, keepdim=True)
    out = x[..., :nb * rows].reshape(*x.shape[:-1], nb, rows).sum(-1)
    if S > nb * rows:
        out[..., -1] += x[..., nb * rows:].sum(-1)
    return out


def block_errs(a, ref, rows=ROWS, zero_ok=False):
    """[B,H,nblocks] of ||a - ref||_F / ||ref||_F over blocks of ``rows`` rows x D.  Every reference block must be non-zero,
    unless ``zero_ok``: a block whose reference is exactly zero (dq and dk of rows that see only themselves: dS = P (dP - D)
    = 0) is then given the error budget of a typical block, ||a||_F / median of the non-zero reference block norms."""
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape and a.dim() == 4, (a.shape, ref.shape)
    r2 = _segments((ref * ref).sum(-1), rows)
    if zero_ok:   # "zero": below 1e-10 of the largest block norm (dP - D cancels to fp64 rounding, not always to 0.0)
        live = r2 > 1e-20 * r2.max()
        assert bool(live.any())
        r2 = torch.where(live, r2, r2[live].median())
    assert bool((r2 > 0).all()), "a reference block is all zero: block_err has nothing to divide by"
    return torch.sqrt(_segments(((a - ref) ** 2).sum(-1), rows) / r2)


def block_err(a, ref, rows=ROWS, zero_ok=False):
    """Maximum of block_errs; NaN / inf anywhere in ``a`` gives inf."""
    e = block_errs(a, ref, rows, zero_ok)
    return float("inf") if not bool(torch.isfinite(e).all()) else e.max().item()


def lse_err(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape
    d = (a - ref).abs().max().item()
    return float("inf") if not math.isfinite(d) else d / max(1.0, ref.abs().max().item())


def global_max_err(a, ref):
    """The metric the older tests use: one number per tensor, normalised by its largest element."""
    a, ref = a.detach().double(), ref.detach().double()
    return ((a - ref).abs().max() / ref.abs().max()).item()


def lse_fp32_err(q, k, allow, scale=None):
    """lse_err of an fp32 logsumexp over fp32 scores of the same inputs against fp64: the scale TOL[...]['lse'] is 8 x of."""
    B, H, S, D = q.shape
    g = H // k.shape[1]
    scale = D ** -0.5 if scale is None else float(scale)
    allow = allow.to(q.device).expand(B, H, S, S)
    s32 = (q.float() @ k.float().repeat_interleave(g, 1).transpose(-1, -2)) * scale
    s64 = (q.double() @ k.double().repeat_interleave(g, 1).transpose(-1, -2)) * scale
    l32 = torch.logsumexp(s32.masked_fill(~allow, float("-inf")), -1)
    l64 = torch.logsumexp(s64.masked_fill(~allow, float("-inf")), -1)
    return lse_err(l32, l64)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("gauss", "peaked", "diag")
OUTPUTS = ("o", "lse", "dq", "dk", "dv")


def inputs(family, B, H, HKV, S, D, seed, scale=None, device="cpu"):
    """bf16 q, w [B,H,S,D] and k, v [B,HKV,S,D] as transposed views of token-major ([B,S,heads,D]) storage.
    gauss:  randn.
    peaked: q, k = sqrt(6 / (scale sqrt(D))) randn: logits of standard deviation ~6, a near one-hot softmax whose winning key
            falls in a random tile; v = randn + 2 so that no output row is near zero.
    diag:   q_i = 0.5 randn + c k_i / |k_i|^2 with c = 8 / scale (s_ii ~ 8, the other logits of unit scale): the diagonal key
            carries most of the weight; v = randn + 2."""
    scale = D ** -0.5 if scale is None else float(scale)
    g_ = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, H, D, generator=g_)
    k = torch.randn(B, S, HKV, D, generator=g_)
    v = torch.randn(B, S, HKV, D, generator=g_)
    w = torch.randn(B, S, H, D, generator=g_)
    if family == "peaked":
        a = math.sqrt(6.0 / (scale * math.sqrt(D)))
        q, k, v = q * a, k * a, v + 2.0
    elif family == "diag":
        kb = k.to(torch.bfloat16).float()
        ke = kb.repeat_interleave(H // HKV, 2)
        q = 0.5 * q + (8.0 / scale) * ke / (ke * ke).sum(-1, keepdim=True)
        v = v + 2.0
    elif family != "gauss":
        raise ValueError(family)
    return tuple(t.to(torch.bfloat16).to(device).transpose(1, 2) for t in (q, k, v, w))


def causal_allow(S, key_valid=None, device="cpu"):
    """tril, or (tril & key_valid) | eye for a bool key_valid [B,S]: [1 or B, 1, S, S]."""
    tri = torch.ones(S, S, dtype=torch.bool, device=device).tril_()[None, None]
    if key_valid is None:
        return tri
    return (tri & key_valid.to(device)[:, None, None, :]) | torch.eye(S, dtype=torch.bool, device=device)[None, None]


def mutant_key_valid(B, S):
    """The key-padding mask mutants (f) and (g) start from: a padded prefix of 5 keys (rows that see only themselves, yet no
    16-row block of dq or dk that is all zero) and every third key after it."""
    kv = torch.ones(B, S, dtype=torch.bool)
    kv[:, :5] = False
    kv[:, 7::3] = False
    return kv


# ---- mutants --------------------------------------------------------------------------------------------------------------
MUTANTS = ("a", "b", "c", "d", "e", "f", "g")


def mutant(name, q, k, v, w, scale=None):
    """(o, lse, dq, dk, dv) of a wrong attention, fp64:
    a  row r loses key r when r % 64 == 0 (r > 0: row 0 has no other key)
    b  row r gains key r + 1 when r % 64 == 63
    c  the 64-key tile [64, 128) dropped for the rows of the last but one 128-row block
    d  dk and dv of the last 64 keys zeroed
    e  KV head h % HKV instead of h // group (differs from the truth only when 1 < HKV < H)
    f  key_valid ignored inside the 64-key tile [128, 192)
    g  the diagonal not reopened for a row whose own key is padded (a row that then sees nothing: output and gradients zero)"""
    B, H, S, D = q.shape
    HKV = k.shape[1]
    tri = causal_allow(S).clone()
    r = torch.arange(S)
    if name == "a":
        e = r[(r % 64 == 0) & (r > 0)]
        tri[0, 0, e, e] = False
        return reference(q, k, v, w, tri, scale)
    if name == "b":
        e = r[(r % 64 == 63) & (r + 1 < S)]
        tri[0, 0, e, e + 1] = True
        return reference(q, k, v, w, tri, scale)
    if name == "c":
        assert S >= 384
        tri[0, 0, S - 256:S - 128, 64:128] = False
        return reference(q, k, v, w, tri, scale)
    if name == "d":
        o, lse, dq, dk, dv = reference(q, k, v, w, tri, scale)
        dk[:, :, S - 64:] = 0
        dv[:, :, S - 64:] = 0
        return o, lse, dq, dk, dv
    if name == "e":
        return reference(q, k, v, w, tri, scale, kv_of_head=[h % HKV for h in range(H)])
    kv = mutant_key_valid(B, S)
    if name == "f":
        kv[:, 128:192] = True
        return reference(q, k, v, w, causal_allow(S, kv), scale)
    if name == "g":
        return reference(q, k, v, w, tri & kv[:, None, None, :], scale)
    raise ValueError(name)


# ---- tolerances -----------------------------------------------------------------------------------------------------------
# From test_attn_check_host.py's measurements on the CPU (S = 512, B = 1, H = 2, HKV = 1, D = 128; the figures are in that
# test's docstring), never from a kernel's output:  3 x twin error <= TOL <= 0.5 x error of every mutant in CATCHES for the pair.
# None: the pair is not checked.  dq and dk on `peaked` and `diag` are ill-conditioned (dS = P (dP - D) cancels: the twin's
# own block error is 0.012-1.4, above the 1e-2 the rule admits), so those families check o, lse and dv only.
# lse: 8 x lse_fp32_err (an fp32 logsumexp of fp32 scores against fp64: 8.0e-8 / 1.6e-7 / 3.2e-7), in lse_err's units.
TOL = {
    "gauss": {"o": 9e-3, "lse": 6.4e-7, "dq": 1.5e-2, "dk": 1.5e-2, "dv": 1.0e-2},
    "peaked": {"o": 9e-3, "lse": 1.3e-6, "dq": None, "dk": None, "dv": 1.2e-2},
    "diag": {"o": 8e-3, "lse": 2.6e-6, "dq": None, "dk": None, "dv": 1.0e-2},
}

# mutants each (family, output) pair is meant to reject: block error (lse: lse_err) at least 2 x TOL
CATCHES = {
    ("gauss", "o"): "abcefg", ("gauss", "lse"): "abcefg", ("gauss", "dq"): "abcefg", ("gauss", "dk"): "abcdefg",
    ("gauss", "dv"): "abcdefg",
    ("peaked", "o"): "acefg", ("peaked", "lse"): "abcefg", ("peaked", "dv"): "acdefg",
    ("diag", "o"): "aeg", ("diag", "lse"): "abcefg", ("diag", "dv"): "acdeg",
}


def check(family, name, a, ref, zero_ok=False):
    """(error, tolerance) of output ``name``; tolerance None: the pair is not checked (the error is still measured)."""
    err = lse_err(a, ref) if name == "lse" else block_err(a, ref, zero_ok=zero_ok)
    return err, TOL[family][name]


# ---- the cases of test_flash_tiles_gpu.py (test_attn_check_host.py runs the twin over the same list) ---------------------------
CAUSAL_HEADS = ((4, 2), (2, 2), (4, 1))
CAUSAL_S = (128, 256, 384, 640)        # one block; an even count; 3 and 5 blocks: odd counts through flash_items' pairing
MASK_S = 384
MASK_NAMES = ("tile", "prefix70", "tail", "k63_k64", "alternate", "all")
VIT_HD = (64, 72, 128)
VIT_N = (1, 63, 64, 65, 128, 129, 192, 193)
FLASH_KNOBS = (0, 4, 7, 23, 1, 2, 16, 20)


def key_valid_mask(name, B, S):
    """bool [B,S]: sample 0 carries the named padding, the other samples are all valid (a mask read under the wrong batch
    index shows)."""
    kv = torch.ones(B, S, dtype=torch.bool)
    if name == "tile":
        kv[0, 128:192] = False          # one whole 64-key tile
    elif name == "prefix70":
        kv[0, :70] = False              # rows 0..69 see only themselves
    elif name == "tail":
        kv[0, S - 100:] = False
    elif name == "k63_k64":
        kv[0, 63:65] = False            # either side of a tile edge
    elif name == "alternate":
        kv[0, 1::2] = False
    elif name != "all":
        raise ValueError(name)
    return kv
