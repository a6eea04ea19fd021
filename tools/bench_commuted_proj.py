"""The ConvNeXt aux projector's first linear at the release shape, resize commuted behind the projection
(``ops.linear_stage_maps``: the stages with fewer positions than the output grid projected at their own resolution, the
products resized and summed by ``cmb_resample_accum``) against the unfused composition (``resample`` every stage to 96 x 96,
concatenate, one 5760-wide GEMM), same process, same run.

    python tools/bench_commuted_proj.py [--out FILE] [--iters 10] [--images 24] [--quick]

Shape: 24 images; ConvNeXt-XXL@1024 stage maps 256^2 x 384, 128^2 x 768, 64^2 x 1536, 32^2 x 3072 (frozen tower: the maps
carry no gradient); output side 96; N = 1024; GELU; bf16 activations, fp32 master weight inside a prepared-weight window (as
in a training step).  Arms: ``unfused``; ``fused`` with fp32 partial products (the default) and with bf16 ones
(``CAMBRIAN_AMD_COMMUTED_PROJ_F32=0``).  The arms alternate; each timing is the median (min - max) of ``WINDOWS`` windows of
``--iters`` calls between HIP events, in microseconds per call: forward alone (under ``no_grad``) and forward + backward
(weight and bias gradients).  ``accumulate alone`` times the ``cmb_resample_accum`` launch of the fused arm on its own and
gives its achieved bytes/s against what the launch must move — base and every source read once, ``pre`` and ``out`` written
once — next to the ~6.3 TB/s an MI355X achieves from HBM.  A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = [(256, 384), (128, 768), (64, 1536), (32, 3072)]       # (side, channels) of the ConvNeXt-XXL@1024 stage maps
SIDE, N_OUT = 96, 1024
HBM_TBPS = 6.3
WINDOWS = 3
ARMS = [("unfused", None), ("fused, fp32 partials", "1"), ("fused, bf16 partials", "0")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--quick", action="store_true", help="maps and output 8 x smaller per side, 2 images (rehearsal)")
    a = ap.parse_args()
    import torch
    from cambrian_amd import lib as L, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_commuted_proj: no GPU visible")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(0)
    B = 2 if a.quick else a.images
    stages = [(s // 8, c) for s, c in STAGES] if a.quick else STAGES
    side = SIDE // 8 if a.quick else SIDE
    ctot = sum(c for _, c in stages)
    maps = [torch.randn(B, s, s, c, device=dev, dtype=dt) for s, c in stages]
    w = torch.nn.Parameter(torch.randn(N_OUT, ctot, device=dev) / ctot ** 0.5)
    b = torch.nn.Parameter(torch.randn(N_OUT, device=dev) * 0.1)
    go = torch.randn(B * side * side, N_OUT, device=dev, dtype=dt)
    assert ops.stage_maps_fusable(maps, side, w, b, L.ACT_GELU_ERF)

    def timed(fn):
        res = []
        for _ in range(WINDOWS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        return res

    def make(arm_env):
        def forward():
            if arm_env is not None:
                os.environ["CAMBRIAN_AMD_COMMUTED_PROJ_F32"] = arm_env
            return ops.linear_stage_maps(maps, side, w, b, L.ACT_GELU_ERF, enabled=arm_env is not None)

        def fwd():
            with torch.no_grad():
                forward()

        def step():
            w.grad = b.grad = None
            ops.weight_step_begin()
            y = forward()
            ops.weight_step_end()
            y.backward(go)
        return fwd, step

    res = {name: dict(fwd=[], step=[]) for name, _ in ARMS}
    outs = {}
    for name, env in ARMS:                                        # warm-up, and the arms against each other
        fwd, step = make(env)
        for _ in range(a.warmup):
            step()
        with torch.no_grad():
            outs[name] = ops.linear_stage_maps(maps, side, w, b, L.ACT_GELU_ERF, enabled=env is not None).float()
    torch.cuda.synchronize()
    for _round in range(2):                                       # the arms alternate
        for name, env in ARMS:
            fwd, step = make(env)
            res[name]["fwd"] += timed(fwd)
            res[name]["step"] += timed(step)

    # the accumulate launch alone, as the fused arm issues it (two dense stages -> base, two commuted -> sources)
    accum = {}
    P = side * side
    for name, pdt in (("fused, fp32 partials", torch.float32), ("fused, bf16 partials", dt)):
        plan = ops.stage_maps_plan([s for s, _ in stages], side)
        base = torch.randn(B, P, N_OUT, device=dev).to(pdt)
        srcs = [(torch.randn(B, s * s, N_OUT, device=dev).to(pdt), s, s) for (s, _), c in zip(stages, plan) if c]
        out = torch.empty(B, P, N_OUT, device=dev, dtype=dt)
        pre = torch.empty_like(out)

        def launch():
            ops.k_resample_accum(out, side, side, base=base, bias=b.detach(), srcs=srcs, pre_out=pre, act=L.ACT_GELU_ERF)
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        nbytes = base.numel() * base.element_size() + sum(x.numel() * x.element_size() for x, _, _ in srcs) + 2 * out.numel() * 2
        accum[name] = (timed(launch), nbytes)
        del base, srcs, out, pre

    def f(ts):
        return f"{statistics.median(ts):.0f} ({min(ts):.0f} - {max(ts):.0f})"

    ref = outs["unfused"]
    scale = ref.abs().max().item()
    lines = ["# Aux projector linear over ConvNeXt stage maps: resize commuted behind the projection against the unfused composition", "",
             f"Command: `python tools/bench_commuted_proj.py --iters {a.iters} --warmup {a.warmup} --images {a.images}`"
             + (" `--quick`" if a.quick else ""),
             f"on `{socket.gethostname()}` (MI355X), bf16, {B} images, maps " + " / ".join(f"{s}^2 x {c}" for s, c in stages)
             + f" -> {side}^2, N = {N_OUT}, GELU; HIP events, {2 * WINDOWS} windows of {a.iters} calls per arm (arms alternating): "
             "median (min - max), microseconds per call.  `max diff` = largest difference of the arm's output from the unfused "
             "arm's, relative to the largest output.", "",
             "| arm | forward us | forward + backward us | x fwd | x fwd+bwd | max diff |", "|---|---|---|---|---|---|"]
    u = res["unfused"]
    for name, _ in ARMS:
        r = res[name]
        lines.append(f"| {name} | {f(r['fwd'])} | {f(r['step'])} | {statistics.median(u['fwd']) / statistics.median(r['fwd']):.2f} | "
                     f"{statistics.median(u['step']) / statistics.median(r['step']):.2f} | "
                     f"{(outs[name] - ref).abs().max().item() / scale:.2e} |")
    lines += ["", "| `cmb_resample_accum` alone | us | MB moved | GB/s | of HBM |", "|---|---|---|---|---|"]
    for name, (ts, nbytes) in accum.items():
        gbs = nbytes / (statistics.median(ts) * 1e-6) / 1e9
        lines.append(f"| {name} | {f(ts)} | {nbytes / 1e6:.0f} | {gbs:.0f} | {gbs / (HBM_TBPS * 1e3) * 100:.0f} % |")
    slower = [name for name, _ in ARMS[1:] if statistics.median(res[name]["step"]) >= statistics.median(u["step"])]
    lines += ["", "Every fused arm's median forward + backward is below the unfused arm's." if not slower else
              "NOT faster than the unfused arm (forward + backward, median): " + "; ".join(slower) + "."]
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
