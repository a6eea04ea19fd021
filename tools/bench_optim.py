"""Optimizer step: ``FusedAdamW`` (cmb_grad_sqnorm + cmb_adamw_step) against ``MasterAdamW`` (+ ``clip_grad_norm_``), same box,
same run.

    python tools/bench_optim.py [--out profiles/fused_adamw.md] [--iters 30] [--quick]

Parameter lists (shapes taken from the release 8B model built on the meta device; values random):
  * ``pretrain``  the pre-training stage's trainable set (SVA layers, connector, projector, newline): fp32 parameters, fp32
                  gradients, stepped in place;
  * ``decoder4``  four Llama-3-8B decoder layers as the finetune stage holds them: bf16 parameters and gradients, fp32 masters.
Arms, each in a fresh child process under its own time limit (the run stops at the first child that fails):
  * ``master``       MasterAdamW.step()                                   (the path before this change)
  * ``master_clip``  torch.nn.utils.clip_grad_norm_(params, 1.0), then MasterAdamW.step()
  * ``fused``        FusedAdamW.step()
  * ``fused_clip``   FusedAdamW(max_grad_norm=1.0).step()
A step is timed with HIP events around the whole call (every launch it makes); the figure is the median over ``--iters``
steps after a warm-up, min - max in brackets.  The gradients stay in place between steps (no backward runs here).
``bytes`` is the HBM traffic the arm's algorithm needs per element, summed over the list:
  fp32 parameter   master 28 (g 4, p / m / v read 12 + written 12), + clip 12 (norm 4, scale 4 + 4); fused 28, + clip 4
  bf16 parameter   master 40 (up-cast 2 + 4, AdamW 28, cast back 4 + 2), + clip 6 (norm 2, scale 2 + 2); fused 28 (g 2,
                   p / m / v 24, bf16 copy 2), + clip 2
GB/s = bytes / time, shown against the ~6.3 TB/s an MI355X achieves from HBM.  A run without a GPU fails; nothing is
estimated."""
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

LISTS = ("pretrain", "decoder4")
ARMS = ("master", "master_clip", "fused", "fused_clip")
HBM_TBPS = 6.3
TRAIN_KEYS = ("mm_projector", "pos_emb", "vision_sampler", "vision_sampler_layers", "vision_query", "image_newline")
BYTES = {   # (parameter is bf16, arm) -> bytes per element
    (False, "master"): 28, (False, "master_clip"): 40, (False, "fused"): 28, (False, "fused_clip"): 32,
    (True, "master"): 40, (True, "master_clip"): 46, (True, "fused"): 28, (True, "fused_clip"): 30,
}


def shapes(which: str, quick: bool):
    """[(shape, is_bf16)] of a parameter list, from the release model's modules (decoder on the meta device: shapes only)"""
    import torch
    os.environ.setdefault("CAMBRIAN_AMD_RANDOM_INIT", "1")
    from cambrian_amd.model.language_model.cambrian_llama import (CambrianLlamaForCausalLM, apply_release_8b_vision_config,
                                                                llama3_8b_config)
    cfg = apply_release_8b_vision_config(llama3_8b_config())
    model = CambrianLlamaForCausalLM(cfg, device=torch.device("meta"), llm_dtype=torch.bfloat16)
    if which == "pretrain":
        out = [(tuple(p.shape), False) for n, p in model.named_parameters() if any(k in n for k in TRAIN_KEYS)]
    else:
        layers = 1 if quick else 4
        out = [(tuple(p.shape), True) for n, p in model.named_parameters()
               if any(n.startswith(f"model.layers.{i}.") for i in range(layers)) and "vision" not in n]
    return out[:40] if quick and which == "pretrain" else out


def child(which: str, arm: str, iters: int, warmup: int, quick: bool) -> None:
    import torch
    from cambrian_amd.train.fused_adamw import FusedAdamW
    from cambrian_amd.train.master import MasterAdamW
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: no GPU visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    params = []
    for shape, low in shapes(which, quick):
        dt = torch.bfloat16 if low else torch.float32
        p = torch.nn.Parameter((torch.randn(shape, device=dev) * 0.02).to(dt))
        p.grad = (torch.randn(shape, device=dev) * 1e-3).to(dt)
        params.append(p)
    n_elem = sum(p.numel() for p in params)
    model_bytes = sum(p.numel() * BYTES[p.dtype == torch.bfloat16, arm] for p in params)
    kw = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    if arm.startswith("master"):
        opt = MasterAdamW(params, **kw)
    else:
        opt = FusedAdamW(params, max_grad_norm=1.0 if arm == "fused_clip" else None, **kw)

    def step():
        if arm == "master_clip":
            torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    rec = dict(list=which, arm=arm, tensors=len(params), elements=n_elem, bytes=model_bytes, iters=iters,
               us=[statistics.median(times), min(times), max(times)])
    print("BENCH_OPTIM " + json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_adamw.md"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a fraction of each list (rehearsal): the table is marked as such")
    ap.add_argument("--child", nargs=2, metavar=("LIST", "ARM"))
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters: at least 10")
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup, a.quick)
        return
    recs = {}
    for which in LISTS:
        for arm in ARMS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, arm, "--iters", str(a.iters),
                   "--warmup", str(a.warmup)] + (["--quick"] if a.quick else [])
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_optim: child {which}/{arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if ln.startswith("BENCH_OPTIM "):
                    r = json.loads(ln[len("BENCH_OPTIM "):])
                    recs[r["list"], r["arm"]] = r
                    print(ln, flush=True)
    lines = ["# Optimizer step: `FusedAdamW` against `MasterAdamW` (+ `clip_grad_norm_`)", "",
             f"Command: `python tools/bench_optim.py --iters {a.iters} --warmup {a.warmup}`" + (" `--quick`" if a.quick else ""),
             f"on `{socket.gethostname()}` (MI355X).  One optimizer step over a parameter list with resident gradients; HIP events "
             f"around the whole step, median of {a.iters} steps (min - max in brackets), each arm in its own process, all arms "
             "in one run.  `pretrain` = the pre-training stage's trainable set (fp32, stepped in place), `decoder4` = four "
             "Llama-3-8B decoder layers (bf16 parameters and gradients, fp32 masters).  `master` / `master_clip` are the path "
             "before this change (`MasterAdamW`, and `torch.nn.utils.clip_grad_norm_` in front of it).  `model MB` is the HBM "
             "traffic the arm's algorithm needs (byte model in the tool's docstring), GB/s = model bytes / time, the share is "
             f"of the ~{HBM_TBPS} TB/s an MI355X achieves from HBM." + ("  REHEARSAL RUN (`--quick`): a fraction of each "
                                                                       "list, not the figures to quote." if a.quick else ""), "",
             "| list | tensors | M elements | arm | step us | model MB | GB/s | of HBM | x vs counterpart |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdict = []
    for which in LISTS:
        for arm in ARMS:
            r = recs[which, arm]
            other = recs[which, arm.replace("fused", "master")]
            gbs = r["bytes"] / (r["us"][0] * 1e-6) / 1e9
            ratio = "" if arm.startswith("master") else f"{other['us'][0] / r['us'][0]:.2f}"
            lines.append(f"| {which} | {r['tensors']} | {r['elements'] / 1e6:.1f} | {arm} | {r['us'][0]:.0f} ({r['us'][1]:.0f} - "
                         f"{r['us'][2]:.0f}) | {r['bytes'] / 1e6:.0f} | {gbs:.0f} | {gbs / (HBM_TBPS * 1e3) * 100:.0f} % | {ratio} |")
            if arm.startswith("fused"):
                verdict.append((which, arm, r["us"][0] < other["us"][0]))
    slower = [f"{w} / {arm}" for w, arm, ok in verdict if not ok]
    lines += ["", "`FusedAdamW` is faster than its `MasterAdamW` counterpart in every row." if not slower else
              "`FusedAdamW` is NOT faster than its `MasterAdamW` counterpart at: " + "; ".join(slower) +
              ".  There the class is clipping without a host synchronisation, not a speed-up."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
