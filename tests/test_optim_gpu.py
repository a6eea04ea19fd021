"""`-m gpu`: cmb_grad_sqnorm / cmb_adamw_step (csrc/optim.hip) through ops.grad_sqnorm / ops.adamw_step and FusedAdamW, against
references computed on the CPU from the same inputs: float64 is the truth, torch's CPU fp32 AdamW the yardstick for what an
fp32 evaluation may lose — err_hip <= 2 * err_torch_fp32 + 1 ulp (max-abs over every element; the ulp is that of the largest
parameter), both being fp32 evaluations of the same formulas.

Tensor list: numels 1, 7, 8, 9, 4095, 4096, 4097, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3 and an empty tensor; fp32 and
bf16 gradients, with and without the bf16 copy; every tensor is a view into a flat buffer with 16 guard elements on both sides,
half of them at element offset 8 (16-byte aligned: the vector path), half at offset 7 (the element-wise path; for every other
one of those only the gradient is displaced, as for a parameter whose gradient is a view into a flat bucket).

Clip tests follow the design note of the feature: Adam's update is nearly invariant to the gradient's scale, so the steps'
norms are 100, 1 and 0.01 times the threshold in turn and eps is 1e-3, and each test first requires the UNCLIPPED reference
to differ from the clipped one by far more than the tolerance."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 16, -77.0   # -77 is exact in bf16
LR, BETAS = 1e-2, (0.9, 0.999)


def _chunk():
    from cambrian_amd import ops
    return ops.OPTIM_CHUNK


def _numels():
    c = _chunk()
    return [1, 7, 8, 9, 4095, 4096, 4097, c - 1, c, c + 1, 2 * c + 3, 0]


def _layout(i):
    """(every pointer displaced, only the gradient displaced, gradient dtype, has a bf16 copy) of tensor i"""
    return i % 4 == 1, i % 4 == 3, torch.bfloat16 if i % 4 >= 2 else torch.float32, i % 3 != 1


def _view(values, dtype, dev, off):
    """``values`` (CPU) as a view at element offset ``off`` of a fresh device buffer with sentinel guard bands"""
    n = values.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    v = buf[off:off + n]
    v.copy_(values)
    return buf, v


def _guards_intact(buf, off, n):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


def _ulp(x):
    x = float(x)
    return float(torch.nextafter(torch.tensor(x, dtype=torch.float32), torch.tensor(float("inf"))) - x)


def _grads(numels, steps, seed, scales=(1.0,)):
    """per step, per tensor: fp32 CPU gradients whose GLOBAL norm is about scales[t % len(scales)], already rounded to bf16
    where the tensor's gradient is bf16 (so every reference sees the values the kernel sees)"""
    gen = torch.Generator().manual_seed(seed)
    total = max(sum(numels), 1)
    out = []
    for t in range(steps):
        s = scales[t % len(scales)] / total ** 0.5
        out.append([(torch.randn(n, generator=gen) * s).to(_layout(i)[2]).float() for i, n in enumerate(numels)])
    return out


def _torch_adamw(dtype, params0, grads, lr, wd, eps, max_norm=None, lr_lambda=None, groups=None):
    """torch's CPU AdamW in ``dtype`` (float64: the truth; float32: the yardstick) over the per-step gradients, optionally
    under clip_grad_norm_ and a LambdaLR; ``groups``: [(indices, lr, wd)].  Returns the parameters after every step and the
    pre-clip norms."""
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params0]
    if groups is None:
        groups = [(list(range(len(ps))), lr, wd)]
    opt = torch.optim.AdamW([{"params": [ps[i] for i in idx], "lr": l, "weight_decay": w} for idx, l, w in groups],
                            lr=lr, betas=BETAS, eps=eps, weight_decay=wd)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda) if lr_lambda else None
    snaps, norms = [], []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(dtype).clone()
        live = [p for p in ps if p.grad is not None]
        norms.append(float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in live))))
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(live, max_norm)
        opt.step()
        if sched:
            sched.step()
        snaps.append([p.detach().clone() for p in ps])
    return snaps, norms


def _max_err(got, ref64):
    return max([float((g.detach().double().cpu() - r).abs().max()) for g, r in zip(got, ref64) if r.numel()] or [0.0])


def _assert_error_rule(got, ref64, ref32, what):
    err_hip, err_t = _max_err(got, ref64), _max_err(ref32, ref64)
    ulp = _ulp(max(float(r.abs().max()) for r in ref64 if r.numel()))
    print(f"{what}: err_hip {err_hip:.3e} err_torch_fp32 {err_t:.3e} ulp {ulp:.3e}")
    assert err_hip <= 2 * err_t + ulp, f"{what}: err_hip {err_hip:.3e} > 2 * {err_t:.3e} + {ulp:.3e}"


# ---- cmb_grad_sqnorm --------------------------------------------------------------------------------------------------------------
def test_grad_sqnorm(dev):
    from cambrian_amd import ops
    numels = _numels()
    gs = _grads(numels, 1, seed=1, scales=(30.0,))[0]
    want = float(sum(g.double().pow(2).sum() for g in gs))
    aligned = [g.to(_layout(i)[2]).to(dev) for i, g in enumerate(gs)]                       # fresh allocations
    held = [_view(g, _layout(i)[2], dev, 7) for i, g in enumerate(gs)]                       # views at an odd element offset
    views = [v for _, v in held]
    assert all(v.data_ptr() % 16 for v in views if v.numel()) and not any(a.data_ptr() % 16 for a in aligned)
    a1 = ops.grad_sqnorm(aligned)
    assert a1.dtype == torch.float32 and a1.dim() == 0 and a1.is_cuda
    a2 = ops.grad_sqnorm(aligned)
    u1 = ops.grad_sqnorm(views)
    print("sqnorm", float(a1), want)
    assert abs(float(a1) - want) <= 1e-5 * want
    assert torch.equal(a1, a2), "two runs differ"
    assert torch.equal(a1, u1), "aligned copies and unaligned views differ"
    assert all(_guards_intact(b, 7, v.numel()) for b, v in held)                              # (the norm writes nothing)
    # the order of the tensors is part of the fixed order; one tensor alone, and none
    one = ops.grad_sqnorm([aligned[9]])
    assert abs(float(one) - float(gs[9].double().pow(2).sum())) <= 1e-5 * float(one)
    assert float(ops.grad_sqnorm([torch.empty(0, device=dev)])) == 0.0
    assert float(ops.grad_sqnorm([torch.empty(0, device=dev, dtype=torch.bfloat16), torch.empty(0, device=dev)])) == 0.0
    nc = torch.randn(6, 10, device=dev).t()                                                   # a non-contiguous gradient
    assert abs(float(ops.grad_sqnorm([nc])) - float(nc.double().pow(2).sum())) <= 1e-5 * float(nc.double().pow(2).sum())


# ---- cmb_adamw_step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_step_against_float64(dev, wd):
    from cambrian_amd import ops
    numels, steps, eps = _numels(), 10, 1e-8
    gen = torch.Generator().manual_seed(2)
    p0 = [torch.randn(n, generator=gen) for n in numels]
    grads = _grads(numels, steps, seed=3, scales=(float(sum(numels)) ** 0.5,))             # element-wise ~ N(0, 1)
    ref64, _ = _torch_adamw(torch.float64, p0, grads, LR, wd, eps)
    ref32, _ = _torch_adamw(torch.float32, p0, grads, LR, wd, eps)
    T = []
    for i, n in enumerate(numels):
        every, grad_only, gdt, has_low = _layout(i)
        off = 7 if every else 8
        t = {"off": off, "goff": 7 if (every or grad_only) else 8, "n": n}
        t["pbuf"], t["p"] = _view(p0[i], torch.float32, dev, off)
        t["mbuf"], t["m"] = _view(torch.zeros(n), torch.float32, dev, off)
        t["vbuf"], t["v"] = _view(torch.zeros(n), torch.float32, dev, off)
        t["gbuf"], t["g"] = _view(torch.zeros(n), gdt, dev, t["goff"])
        t["lbuf"], t["low"] = _view(torch.zeros(n), torch.bfloat16, dev, off) if has_low else (None, None)
        T.append(t)
    vec = [t for t in T if t["n"] and all(x is None or x.data_ptr() % 16 == 0 for x in (t["p"], t["m"], t["v"], t["g"], t["low"]))]
    assert len(vec) == 6 and sum(1 for t in T if t["n"]) == 11, "of the non-empty tensors, 6 take the vector path and 5 the other"
    for step in range(steps):
        for t, g in zip(T, grads[step]):
            t["g"].copy_(g)
        ops.adamw_step([t["g"] for t in T], [t["p"] for t in T], [t["m"] for t in T], [t["v"] for t in T],
                       [t["low"] for t in T], lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=eps, weight_decay=wd, step=step + 1)
        for t in T:
            if t["low"] is not None:
                assert torch.equal(t["low"], t["p"].to(torch.bfloat16)), f"bf16 copy of a tensor of {t['n']} after step {step}"
    _assert_error_rule([t["p"] for t in T], ref64[-1], ref32[-1], f"adamw wd={wd}")
    for t in T:
        for buf, off in ((t["pbuf"], t["off"]), (t["mbuf"], t["off"]), (t["vbuf"], t["off"]), (t["gbuf"], t["goff"]),
                         (t["lbuf"], t["off"])):
            assert buf is None or _guards_intact(buf, off, t["n"]), f"guard band of a tensor of {t['n']} elements was written"
        assert bool(torch.isfinite(t["m"]).all()) and bool((t["v"] >= 0).all())


# ---- FusedAdamW ---------------------------------------------------------------------------------------------------------------------
def _param_set(dev, seed=5):
    """fp32 and bf16 Parameters (one of them a view at an odd offset of a flat buffer, as under flat buckets) and their
    starting values as fp32 CPU tensors (a bf16 parameter's master starts at its own value)"""
    c = _chunk()
    spec = [(9, torch.float32), (4097, torch.bfloat16), (c + 1, torch.float32), (1, torch.bfloat16), (2 * c + 3, torch.bfloat16),
            (333, torch.float32)]
    gen = torch.Generator().manual_seed(seed)
    params, p0 = [], []
    for i, (n, dt) in enumerate(spec):
        v = torch.randn(n, generator=gen).to(dt)
        if i == 5:
            flat = torch.zeros(n + 16, dtype=dt, device=dev)
            flat[7:7 + n].copy_(v)
            params.append(torch.nn.Parameter(flat[7:7 + n]))
        else:
            params.append(torch.nn.Parameter(v.to(dev)))
        p0.append(v.float())
    return params, p0


def _set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad = None if g is None else g.to(p.dtype).to(p.device)


def _stepped(opt, params):
    """the fp32 tensors the optimizer steps, in the order of ``params``: the master of a bf16 parameter, else the parameter"""
    master_of = {id(low): m for m, low in zip(opt.masters, opt.low)}
    return [master_of.get(id(p), p) for p in params]


def _pgrads(params, steps, seed, scales):
    gen = torch.Generator().manual_seed(seed)
    total = sum(p.numel() for p in params)
    return [[(torch.randn(p.numel(), generator=gen) * (scales[t % len(scales)] / total ** 0.5)).to(p.dtype).float()
             for p in params] for t in range(steps)]


def _no_sync_step(opt):
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_fused_adamw_clipping(dev):
    from cambrian_amd.train.fused_adamw import FusedAdamW
    eps, wd, steps, scales = 1e-3, 0.1, 6, (100.0, 1.0, 0.01)
    params, p0 = _param_set(dev)
    grads = _pgrads(params, steps, seed=6, scales=scales)
    ref64, norms64 = _torch_adamw(torch.float64, p0, grads, LR, wd, eps, max_norm=1.0)
    ref32, _ = _torch_adamw(torch.float32, p0, grads, LR, wd, eps, max_norm=1.0)
    free64, _ = _torch_adamw(torch.float64, p0, grads, LR, wd, eps)
    tol = 2 * _max_err(ref32[-1], ref64[-1]) + _ulp(max(float(r.abs().max()) for r in ref64[-1]))
    assert _max_err(free64[-1], ref64[-1]) > 1000 * tol, "clipping changes nothing here: the test could not see a missing clip"
    assert norms64[0] > 50 and norms64[2] < 0.02
    opt = FusedAdamW(params, lr=LR, betas=BETAS, eps=eps, weight_decay=wd, max_grad_norm=1.0)
    assert opt.last_grad_norm is None
    for t in range(steps):
        _set_grads(params, grads[t])
        _no_sync_step(opt)                       # raises on any host synchronisation inside step()
        n = opt.last_grad_norm
        assert n.is_cuda and n.dtype == torch.float32 and n.dim() == 0
        assert abs(float(n) - norms64[t]) <= 1e-5 * norms64[t], (t, float(n), norms64[t])
        opt.zero_grad()
    _assert_error_rule(_stepped(opt, params), ref64[-1], ref32[-1], "clipped")
    for m, low in zip(opt.masters, opt.low):
        assert torch.equal(low.detach(), m.detach().to(torch.bfloat16))


def test_fused_adamw_huge_threshold_equals_no_clipping(dev):
    from cambrian_amd.train.fused_adamw import FusedAdamW
    steps = 3
    pa, _ = _param_set(dev)
    pb, _ = _param_set(dev)
    grads = _pgrads(pa, steps, seed=7, scales=(100.0, 1.0, 0.01))
    a = FusedAdamW(pa, lr=LR, eps=1e-3, weight_decay=0.1, max_grad_norm=1e30)
    b = FusedAdamW(pb, lr=LR, eps=1e-3, weight_decay=0.1)
    for t in range(steps):
        for opt, ps in ((a, pa), (b, pb)):
            _set_grads(ps, grads[t])
            opt.step()
            opt.zero_grad()
    assert b.last_grad_norm is None and a.last_grad_norm is not None
    for x, y in zip(_stepped(a, pa) + pa, _stepped(b, pb) + pb):
        assert torch.equal(x.detach(), y.detach())
    for opt_a, opt_b in zip(_stepped(a, pa), _stepped(b, pb)):
        assert torch.equal(a.state[opt_a]["exp_avg_sq"], b.state[opt_b]["exp_avg_sq"])


def test_fused_adamw_groups_scheduler_and_missing_gradients(dev):
    """two groups with their own lr / weight decay, a LambdaLR stepping both, and a parameter that never gets a gradient:
    its value and its (absent) state stay untouched, while the others match the references"""
    from cambrian_amd.train.fused_adamw import FusedAdamW
    eps, steps = 1e-8, 5
    params, p0 = _param_set(dev)
    idle = 3
    groups = [([0, 1, 2], 1e-2, 0.1), ([3, 4, 5], 3e-3, 0.0)]
    lam = lambda k: 1.0 / (1.0 + k)
    grads = _pgrads(params, steps, seed=8, scales=(float(sum(p.numel() for p in params)) ** 0.5,))
    for gs in grads:
        gs[idle] = None
    ref64, _ = _torch_adamw(torch.float64, p0, grads, LR, 0.0, eps, lr_lambda=lam, groups=groups)
    ref32, _ = _torch_adamw(torch.float32, p0, grads, LR, 0.0, eps, lr_lambda=lam, groups=groups)
    opt = FusedAdamW([{"params": [params[i] for i in idx], "lr": l, "weight_decay": w} for idx, l, w in groups],
                     lr=LR, betas=BETAS, eps=eps)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    idle_before = params[idle].detach().clone()
    for t in range(steps):
        _set_grads(params, grads[t])
        _no_sync_step(opt)
        sched.step()
        opt.zero_grad()
    assert abs(opt.param_groups[0]["lr"] - 1e-2 / (1 + steps)) < 1e-12 and abs(opt.param_groups[1]["lr"] - 3e-3 / (1 + steps)) < 1e-12
    st = _stepped(opt, params)
    assert torch.equal(params[idle].detach(), idle_before) and torch.equal(st[idle].detach(), idle_before.float())
    assert len(opt.state[st[idle]]) == 0, "a parameter without a gradient must not get optimizer state"
    _assert_error_rule(st, ref64[-1], ref32[-1], "groups + LambdaLR")
    assert opt.state_bytes() == sum(p.numel() * (12 if p.dtype == torch.bfloat16 else 8) for p in params)


def test_state_dict_round_trip_through_master_adamw(dev):
    """FusedAdamW (3 steps) -> MasterAdamW (2 steps) -> FusedAdamW (3 steps), each built over the same parameters and loaded
    from the previous one's state_dict(), against one uninterrupted reference run of 8 steps."""
    from cambrian_amd.train.fused_adamw import FusedAdamW
    from cambrian_amd.train.master import MasterAdamW
    eps, wd, legs = 1e-8, 0.1, (3, 2, 3)
    params, p0 = _param_set(dev)
    grads = _pgrads(params, sum(legs), seed=9, scales=(float(sum(p.numel() for p in params)) ** 0.5,))
    ref64, _ = _torch_adamw(torch.float64, p0, grads, LR, wd, eps)
    ref32, _ = _torch_adamw(torch.float32, p0, grads, LR, wd, eps)
    make = [lambda: FusedAdamW(params, lr=LR, betas=BETAS, eps=eps, weight_decay=wd),
            lambda: MasterAdamW(params, lr=LR, betas=BETAS, eps=eps, weight_decay=wd),
            lambda: FusedAdamW(params, lr=LR, betas=BETAS, eps=eps, weight_decay=wd)]
    sd, t = None, 0
    for leg, build in zip(legs, make):
        opt = build()
        if sd is not None:
            with torch.no_grad():                       # loading must restore the parameters too: scramble them first
                for p in opt.low:
                    p.mul_(0.5)
            opt.load_state_dict(copy.deepcopy(sd))
        for _ in range(leg):
            _set_grads(params, grads[t])
            opt.step()
            opt.zero_grad()
            t += 1
        sd = opt.state_dict()
        assert set(sd) == {"state", "param_groups", "masters"} and len(sd["masters"]) == 3
        assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
        assert all(float(s["step"]) == t for s in sd["state"].values())
        _assert_error_rule(_stepped(opt, params), ref64[t - 1], ref32[t - 1], f"after leg ending at step {t}")
    for m, low in zip(opt.masters, opt.low):
        assert torch.equal(low.detach(), m.detach().to(torch.bfloat16))


def test_end_to_end_train_step(dev, monkeypatch):
    """the smallest model configuration of tests/test_model_gpu.py: forward, backward, GradSync.finish(),
    FusedAdamW(max_grad_norm=1.0).step(); then the next forward's weight_step_begin() must prepare its bf16 weight copies
    from the UPDATED fp32 parameters."""
    from test_model_gpu import P0, S, SIDE, _build
    from cambrian_amd import ops
    from cambrian_amd.train.data_layout import synthetic_batch
    from cambrian_amd.train.dp import GradSync
    from cambrian_amd.train.fused_adamw import FusedAdamW
    dt = torch.bfloat16
    model, cfg, towers = _build(dev, dt, monkeypatch, kinds=("vit",))
    train = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert len(train) > 30
    sync = GradSync([p for _, p in train])
    opt = FusedAdamW([p for _, p in train], lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    batch = synthetic_batch(2, seq_len=S, image_position=P0, image_token_len=SIDE * SIDE, aux_token_lens=[16],
                            image_res=[56], image_sizes=[(336, 336), (336, 150)], vocab_lo=1, vocab_hi=300)

    def forward():
        att = batch["attention_mask"]
        return model(input_ids=batch["input_ids"].to(dev), attention_mask=None if att is None else att.to(dev),
                     position_ids=batch["position_ids"].to(dev), labels=batch["labels"].to(dev),
                     images=[i.to(dev, dt) for i in batch["images"]],
                     image_aux_attention_masks_list=[m.to(dev) for m in batch["image_aux_attention_masks_list"]],
                     image_sizes=batch["image_sizes"])

    before = [p.detach().clone() for _, p in train]
    forward().loss.backward()
    sync.finish()
    assert all(p.grad is not None for _, p in train)
    want_norm = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for _, p in train)))
    _no_sync_step(opt)
    assert abs(float(opt.last_grad_norm) - want_norm) <= 1e-5 * want_norm
    for (n, p), b in zip(train, before):
        assert bool(torch.isfinite(p).all()), n
        assert not torch.equal(p.detach(), b), f"{n} did not change"
    opt.zero_grad()
    loss2 = forward().loss                       # opens the next prepared-weight window: one cmb_weight_prep over the table
    assert bool(torch.isfinite(loss2))
    trained = {id(p) for _, p in train}
    checked = 0
    for e in ops._PREP.values():
        base = e.ref()
        if base is None or id(base) not in trained:
            continue
        w = torch.as_strided(base.detach(), e.shape, e.stride, e.off)
        assert torch.equal(e.w_c, w.to(torch.bfloat16)), "a prepared bf16 copy is not the updated parameter's cast"
        checked += 1
    assert checked > 5, checked
