"""Forward + backward of the bilinear token-grid resize alone: the resample kernel and its adjoint (``ops.resample_bilinear`` /
``ops.resample_concat``) against the ATen body (``CAMBRIAN_AMD_RESAMPLE_BWD=0``: permute, fp32 up-cast, ``F.interpolate``,
cast, permute, ``torch.cat``), same box, same run.

    python tools/bench_resample.py [--out profiles/resample_bwd.md] [--iters 50] [--quick]

Shapes, bf16, batch 8 (the reference's batch with the towers unfrozen):
  * ``convnext-xxl``  the four ConvNeXt-XXL@1024 stage maps 256^2 x 384, 128^2 x 768, 64^2 x 1536, 32^2 x 3072 -> 96^2 as ONE
                      ``resample_concat`` ([8, 9216, 5760]);
  * ``vit-1152`` / ``vit-1536``  27^2 -> 24^2 at C = 1152 (SigLIP) and 1536 (DINOv2-g), the tokens behind a CLS row.
Each arm runs in a fresh child process, the arms alternating (``--rounds`` children per arm); a child warms every shape up,
then times windows of ``--iters`` forward + backward calls with HIP events.  The table pools the windows of an arm's
children: median (min - max).  The kernel arm also times the adjoint launches alone (``k_resample_bwd``) and gives their
achieved bytes/s against what one pass must move, B * (Ho*Wo + Hi*Wi) * C * 2 B, next to the ~6.3 TB/s an MI355X achieves
from HBM.  ``peak MB`` is ``torch.cuda.max_memory_allocated`` over the timed calls, inputs and incoming gradient included.
The kernel arm counts as faster at a shape only when its slowest window beats the ATen arm's fastest.
A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH = 8
CONVNEXT = [(256, 384), (128, 768), (64, 1536), (32, 3072)]       # (side, channels) of the ConvNeXt-XXL@1024 stage maps
SHAPES = ["convnext-xxl", "vit-1152", "vit-1536"]
HBM_TBPS = 6.3
WINDOWS = 3


def pass_bytes(shape: str) -> int:
    """what one pass (forward, or backward) must move: every input cell and every output cell once, bf16"""
    if shape == "convnext-xxl":
        return sum(BATCH * (96 * 96 + s * s) * c * 2 for s, c in CONVNEXT)
    return BATCH * (24 * 24 + 27 * 27) * int(shape.split("-")[1]) * 2


def child(arm: str, iters: int, warmup: int, quick: bool) -> None:
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.multimodal_encoder import vit_ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: no GPU visible")
    assert ops.resample_enabled() == (arm == "kernel")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(0)

    def timed(fn, n):
        """WINDOWS windows of n calls, microseconds per call"""
        res = []
        for _ in range(WINDOWS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(n):
                fn()
            b.record()
            b.synchronize()
            res.append(a.elapsed_time(b) * 1e3 / n)
        return res

    for shape in (SHAPES[1:2] if quick else SHAPES):
        if shape == "convnext-xxl":
            leaves = [torch.randn(BATCH, s, s, c, device=dev, dtype=dt).requires_grad_() for s, c in CONVNEXT]
            g = torch.randn(BATCH, 96 * 96, sum(c for _, c in CONVNEXT), device=dev, dtype=dt)

            def fwd():
                return ops.resample_concat(leaves, 96)

            def bwd_alone():
                off = 0
                for (s, c), dx in zip(CONVNEXT, scratch):
                    vit_ops.k_resample_bwd(g, 96, 96, dx, s, s, col_offset=off)
                    off += c
            scratch_shapes = [(BATCH, s * s, c) for s, c in CONVNEXT]
        else:
            C = int(shape.split("-")[1])
            seq = torch.randn(BATCH, 27 * 27 + 1, C, device=dev, dtype=dt).requires_grad_()      # CLS row + 27 x 27 tokens
            leaves = [seq]
            g = torch.randn(BATCH, 24 * 24, C, device=dev, dtype=dt)

            def fwd():
                return ops.resample_bilinear(seq[:, 1:], 27, 27, 24, 24)

            def bwd_alone():
                vit_ops.k_resample_bwd(g, 24, 24, scratch[0], 27, 27)
            scratch_shapes = [(BATCH, 27 * 27, C)]

        def step():
            for t in leaves:
                t.grad = None
            fwd().backward(g)

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        us = timed(step, iters)
        peak = torch.cuda.max_memory_allocated()
        rec = dict(shape=shape, arm=arm, iters=iters, step_us=us, peak_bytes=peak, pass_bytes=pass_bytes(shape))
        if arm == "kernel":
            scratch = [torch.empty(sh, device=dev, dtype=dt) for sh in scratch_shapes]
            for _ in range(warmup):
                bwd_alone()
            torch.cuda.synchronize()
            rec["bwd_us"] = timed(bwd_alone, iters)
            del scratch
        print("BENCH_RESAMPLE " + json.dumps(rec), flush=True)
        for t in leaves:
            t.grad = None
        del leaves, g
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bwd.md"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="child processes per arm (the arms alternate)")
    ap.add_argument("--quick", action="store_true", help="one small shape only (rehearsal)")
    ap.add_argument("--child", metavar="ARM")
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: at least 20")
    if a.child:
        child(a.child, a.iters, a.warmup, a.quick)
        return
    recs: dict = {}
    for _round in range(a.rounds):
        for arm in ("kernel", "aten"):
            env = dict(os.environ, CAMBRIAN_AMD_RESAMPLE_BWD="1" if arm == "kernel" else "0")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--iters", str(a.iters),
                   "--warmup", str(a.warmup)] + (["--quick"] if a.quick else [])
            # the GPU step runs under its own time limit (SIGTERM, then SIGKILL 10 s later)
            p = subprocess.run(["timeout", "-k", "10", "240"] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_resample: child {arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if ln.startswith("BENCH_RESAMPLE "):
                    r = json.loads(ln[len("BENCH_RESAMPLE "):])
                    acc = recs.setdefault((r["shape"], r["arm"]), dict(step_us=[], bwd_us=[], peak_bytes=0, pass_bytes=r["pass_bytes"]))
                    acc["step_us"] += r["step_us"]
                    acc["bwd_us"] += r.get("bwd_us", [])
                    acc["peak_bytes"] = max(acc["peak_bytes"], r["peak_bytes"])
                    print(ln, flush=True)

    def f(ts):
        return f"{statistics.median(ts):.1f} ({min(ts):.1f} - {max(ts):.1f})"

    lines = ["# Bilinear resize, forward + backward: the resample kernels against the ATen body", "",
             f"Command: `python tools/bench_resample.py --iters {a.iters} --warmup {a.warmup} --rounds {a.rounds}`"
             + (" `--quick`" if a.quick else ""),
             f"on `{socket.gethostname()}` (MI355X), bf16, batch {BATCH}; HIP events, windows of {a.iters} forward + backward calls, "
             f"{WINDOWS} windows per child process, {a.rounds} alternating child processes per arm: median (min - max) over an arm's "
             "windows, microseconds per call.  `adjoint alone` = the `k_resample_bwd` launches of the shape without autograd; its "
             "GB/s is against B * (Ho*Wo + Hi*Wi) * C * 2 B, what one pass must move, and the share is of the "
             f"~{HBM_TBPS} TB/s an MI355X achieves from HBM.  `peak MB` = `torch.cuda.max_memory_allocated` over the timed calls.", "",
             "| shape | fwd+bwd kernel us | fwd+bwd ATen us | x | peak MB kernel | peak MB ATen | adjoint alone us | pass MB | GB/s | of HBM |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for shape in SHAPES:
        kr, ar = recs.get((shape, "kernel")), recs.get((shape, "aten"))
        if kr is None or ar is None:
            continue
        gbs = kr["pass_bytes"] / (statistics.median(kr["bwd_us"]) * 1e-6) / 1e9
        lines.append(f"| {shape} | {f(kr['step_us'])} | {f(ar['step_us'])} | "
                     f"{statistics.median(ar['step_us']) / statistics.median(kr['step_us']):.2f} | {kr['peak_bytes'] / 1e6:.0f} | "
                     f"{ar['peak_bytes'] / 1e6:.0f} | {f(kr['bwd_us'])} | {kr['pass_bytes'] / 1e6:.1f} | {gbs:.0f} | "
                     f"{gbs / (HBM_TBPS * 1e3) * 100:.0f} % |")
        if max(kr["step_us"]) >= min(ar["step_us"]):
            slower.append(shape)
    lines += ["", "The kernel arm's slowest window beats the ATen arm's fastest at every listed shape." if not slower else
              "The kernel arm is NOT faster by more than the spread at: " + "; ".join(slower) + "."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
