"""CPU, world_size 2, gloo: ``Zero2AdamW(max_grad_norm=...)`` (cambrian_amd/train/zero.py) — the global L2 clip of the
rank-averaged gradient, formed from the owned shards' sums of squares and one all-reduced scalar — against an unsharded
``torch.optim.AdamW`` with ``torch.nn.utils.clip_grad_norm_`` on the rank-averaged gradients.

Adam's update is nearly invariant to the gradient's scale, so a clip shows only where different coefficients enter the
moments or eps matters: the three steps scale the loss by 300, 1 and 0.003 (norms far above, near and far below the
threshold) and eps is 1e-3.  The test first requires the UNCLIPPED reference to differ from the clipped one by far more than
the tolerance, so that it cannot pass without a clip."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

# lr: the bound below is 1e-5 * lr whatever lr is; at 3e-2 it is 3e-7, above the 1.19e-7 spacing of the fp32 LayerNorm weights
# (which sit at 1): a bound below one spacing could not tell a last-place rounding difference from an error
LR, WD, EPS, STEPS = 3e-2, 0.1, 1e-3, 3
LOSS_SCALE = (300.0, 1.0, 0.003)
# a delta-relative change of the coefficient moves an update by O(delta * lr); the coefficients here agree to fp32 rounding
ATOL = 1e-5 * LR


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(16, 33), torch.nn.GELU(), torch.nn.Linear(33, 32), torch.nn.LayerNorm(32),
                               torch.nn.Linear(32, 5))


def _data(world, step):
    return [torch.randn(8, 16, generator=torch.Generator().manual_seed(100 * step + k)) for k in range(world)]


def _loss(m, x, step):
    return m(x).pow(2).mean() * LOSS_SCALE[step]


def _reference(world, max_norm):
    """unsharded AdamW on the rank-averaged gradients; (parameters, float64 norms of the averaged gradient per step)"""
    m = _model()
    unused = torch.nn.Parameter(torch.ones(7))
    params = list(m.parameters()) + [unused]
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, eps=EPS)
    norms = []
    for step in range(STEPS):
        grads = None
        for k in range(world):
            for p in params:
                p.grad = None
            _loss(m, _data(world, step)[k], step).backward()
            g = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params]
            grads = g if grads is None else [a + b for a, b in zip(grads, g)]
        for p, g in zip(params, grads):
            p.grad = g / world
        norms.append(float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in params))))
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
    return [p.detach().clone() for p in params], norms


def _run_zero(rank, world, max_norm):
    from cambrian_amd.train.zero import Zero2AdamW
    m = _model()
    unused = torch.nn.Parameter(torch.ones(7))
    params = list(m.parameters()) + [unused]
    kw = {} if max_norm is None else {"max_grad_norm": max_norm}
    opt = Zero2AdamW(params, lr=LR, weight_decay=WD, eps=EPS, bucket_mb=0.002, **kw)   # tiny buckets: several shards per rank
    assert len(opt.buckets) > 2
    norms = []
    for step in range(STEPS):
        _loss(m, _data(world, step)[rank], step).backward()
        opt.step()
        opt.zero_grad()
        norms.append(None if opt.last_grad_norm is None else float(opt.last_grad_norm))
    opt.remove()
    return [p.detach().clone() for p in params], norms


def _maxdiff(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from cambrian_amd.train.dp import init_distributed
    init_distributed("gloo")
    out = {}
    ref_clip, norms64 = _reference(world, 1.0)
    ref_free, norms64_free = _reference(world, None)
    out["norms64"] = norms64
    out["clip_matters"] = _maxdiff(ref_clip, ref_free)
    got_clip, norms = _run_zero(rank, world, 1.0)
    out["norm_rel"] = max(abs(a - b) / b for a, b in zip(norms, norms64))
    out["clip_err"] = _maxdiff(got_clip, ref_clip)
    got_free, norms_free = _run_zero(rank, world, None)
    out["free_norms"] = norms_free
    out["free_ok"] = all(torch.allclose(p, w, atol=1e-6, rtol=1e-5) for p, w in zip(got_free, ref_free))   # test_zero.py's
    got_loose, norms_loose = _run_zero(rank, world, 1e6)       # far above every norm: the coefficient is exactly 1
    out["loose_equal"] = all(torch.equal(a, b) for a, b in zip(got_loose, got_free))
    out["loose_norm_rel"] = max(abs(a - b) / b for a, b in zip(norms_loose, norms64_free))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_zero2_clip_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [0, 1]
    for rank, out in res.items():
        print(rank, out)
        n = out["norms64"]
        assert n[0] > 10.0 and n[2] < 0.1, f"the steps do not straddle the threshold: {n}"
        assert out["clip_matters"] > 1000 * ATOL, "clipping changes nothing here: the test could not see a missing clip"
        assert out["norm_rel"] <= 1e-6, out
        assert out["clip_err"] <= ATOL, out
        assert out["free_norms"] == [None] * STEPS and out["free_ok"], out
        assert out["loose_equal"], "a norm below the threshold must leave the unclipped run's bits"
        assert out["loose_norm_rel"] <= 1e-6, out


def test_zero2_clip_single_process():
    """world 1 (no process group): the clip is one extra pass over the shard, against clip_grad_norm_ + AdamW."""
    from cambrian_amd.train.zero import Zero2AdamW
    m = _model()
    opt = Zero2AdamW(list(m.parameters()), lr=LR, weight_decay=WD, eps=EPS, max_grad_norm=1.0)
    m2 = _model()
    o2 = torch.optim.AdamW(m2.parameters(), lr=LR, weight_decay=WD, eps=EPS)
    for step in range(STEPS):
        _loss(m, _data(1, step)[0], step).backward()
        opt.step()
        opt.zero_grad()
        o2.zero_grad()
        _loss(m2, _data(1, step)[0], step).backward()
        want = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in m2.parameters())))
        torch.nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
        o2.step()
        assert abs(float(opt.last_grad_norm) - want) <= 1e-6 * want
    assert _maxdiff([p.detach() for p in m.parameters()], [p.detach() for p in m2.parameters()]) <= ATOL
