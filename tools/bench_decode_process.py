#!/usr/bin/env python
"""Measures the logits processors of ``generate()`` on the device (``cmb_decode_process``, CAMBRIAN_AMD_DECODE_PROCESS=1) and
writes profiles/decode_process.md:

(a) the kernel alone on device events at V = 128256, B = 1 and 16, histories of 16, 256 and 2048 ids, three arms (penalty
    only, n-gram 3 only, everything on), each beside ``processors.apply_torch`` on the same tensors;
(b) ms per decoded token through ``generate()`` on the Llama-3-8B geometry at full depth, context 2048, batch 1, 4 and 16, bf16
    and e4m3 weights, ``repetition_penalty=1.2, no_repeat_ngram_size=3``: the one-call step plus the kernel, the one-call step
    plus ``apply_torch`` in the kernel's place, and the one-call step without processors (``--parent-tree``: on a checkout of the
    parent commit with its library built; without it that arm is this tree with the switch off and the table says so);
(c) the kernel's registers, LDS and spills from hipcc's remarks (no GPU needed: ``--dump-resources FILE`` where hipcc is).

Every arm of (b) runs in its own process; a window is (wall clock of ``generate()`` for 1 + NEW tokens - that for 1 token,
device synchronised) / NEW; median of 3 windows (min - max) after one warm-up call of every shape.  **faster** = the median is
below the other arm's fastest window, anything else is NOT faster.  ``--parts a``, ``--parts b`` or ``--parts ab``; ``--from-log``
writes the note again from a run's output.  A run without a GPU fails; nothing is made up for a part that did not run: the note
calls it unmeasured."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_decode_step import resource_usage  # noqa: E402

V = 128256
CTX = 2048
BATCHES = [1, 4, 16]
KTAG = "BENCH_DECODE_PROCESS_KERNEL "
GTAG = "BENCH_DECODE_PROCESS_GENERATE "
GEN_KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)
KERNEL_REPS, TORCH_REPS = 2000, 200          # calls per timed window of part (a)


def kernel_child() -> None:
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import processors as P
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_process: no GPU visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    arms = (("penalty 1.2", lambda w: P.ProcessSpec(penalty=float(torch.tensor(1.2, dtype=torch.float32)))),
            ("ngram 3", lambda w: P.ProcessSpec(ngram=3)),
            ("everything", lambda w: P.ProcessSpec(penalty=float(torch.tensor(1.2, dtype=torch.float32)), ngram=3, min_new=4096,
                                                   eos=[128001, 128009], bans=[5, 6, 7], words=w)))

    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    def timed(fk, ft, windows=5):
        """us per call of both arms: warm-up, then windows of KERNEL_REPS / TORCH_REPS calls, the arms alternating"""
        for _ in range(20):
            fk()
            ft()
        torch.cuda.synchronize()
        k, t = [], []
        for _ in range(windows):
            k.append(window(fk, KERNEL_REPS))
            t.append(window(ft, TORCH_REPS))
        return (statistics.median(k), min(k), max(k)), (statistics.median(t), min(t), max(t))

    for B in (1, 16):
        for n in (16, 256, 2048):
            hist = torch.randint(0, 4000, (B, n), generator=g).to(dev)          # a few thousand symbols: ids repeat, n-grams rarely
            words = [[int(i) for i in torch.randint(0, 4000, (k,), generator=g)] for k in (2, 3, 4, 2)]
            for name, make in arms:
                spec = make(words)
                proc = ops.DecodeProcess(spec, dev)
                logits = (torch.randn(B, V, generator=g) * 3).to(dev)
                done = torch.zeros(B, dtype=torch.bool, device=dev)
                ref = P.apply_torch(logits.clone(), hist, n, spec)
                got = ops.decode_process(logits.clone(), hist, n, proc)
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (B, n, name)
                k, t = timed(lambda: ops.decode_process(logits, hist, n, proc, done),
                             lambda: P.apply_torch(logits, hist, n, spec, done))
                print(KTAG + json.dumps(dict(B=B, n=n, arm=name, kernel_us=k, torch_us=t)), flush=True)


def generate_child(tree: str, arm: str, new: int, quick: bool) -> None:
    sys.path.insert(0, tree)
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_process: no GPU visible")
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == os.path.abspath(tree)
    prec, mode = arm.split("-")                          # bf16 | fp8, kernel | torch | none | parent
    assert ops.decode_step_enabled() and ops.decode_fp8_enabled() == (prec == "fp8")
    kw = dict(GEN_KW) if mode in ("kernel", "torch") else {}
    calls = {"process": 0}
    if mode in ("kernel", "torch"):
        from cambrian_amd.model.language_model import processors as P
        assert ops.decode_process_enabled()
        real = ops.decode_process

        def counted(logits, hist, n, proc, done=None):
            calls["process"] += 1
            return real(logits, hist, n, proc, done) if mode == "kernel" else P.apply_torch(logits, hist, n, proc.spec, done)

        ops.decode_process = counted
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=dt)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()

    def gen(ids, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B in (BATCHES[:1] if quick else BATCHES):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, cfg.vocab_size, (B, CTX), generator=g).to(dev)
        calls["process"] = 0
        _, first = gen(ids, 1 + new)                    # warm-up of every shape
        assert calls["process"] == (1 + new if kw else 0), calls
        base = statistics.median(gen(ids, 1)[0] for _ in range(3))
        win = []
        for _ in range(3):
            ms, out = gen(ids, 1 + new)
            assert torch.equal(out, first)
            win.append((ms - base) / new)
        print(GTAG + json.dumps(dict(arm=arm, B=B, new=new, ms=(statistics.median(win), min(win), max(win)),
                                     tokens=first[0, :8].tolist())), flush=True)
        del ids


def f3(t, unit=""):
    return f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f}){unit}"


def write_note(path: str, log: str, resources, parent: bool) -> None:
    krecs, grecs = [], {}
    if log and os.path.exists(log):
        with open(log) as fh:
            for ln in fh:
                if ln.startswith(KTAG):
                    krecs.append(json.loads(ln[len(KTAG):]))
                elif ln.startswith(GTAG):
                    r = json.loads(ln[len(GTAG):])
                    grecs[r["arm"], r["B"]] = r
    L = ["# Logits processors on the device: `cmb_decode_process`", "",
         "Written by `tools/bench_decode_process.py`.  The feature is opt-in (`CAMBRIAN_AMD_DECODE_PROCESS=1` / "
         "`config.decode_logits_processors`) whatever these tables say; no threshold is derived from them.  A figure that is "
         "not in this note is unmeasured.", "",
         "## (a) The kernel alone, V = 128256", ""]
    if krecs:
        L += [f"Device events around {KERNEL_REPS} launches ({TORCH_REPS} calls for `apply_torch`), 5 windows per arm, the arms "
              "alternating, after 20 warm-up calls of each; us per call, median (min - max).  Back-to-back launches: the figure is the "
              "launch rate plus the kernel, not the kernel's device time alone.  Both arms edit the same fp32 logits in place from the same history (ids drawn from 4000 symbols) and "
              "were checked equal bit for bit on a copy first.  `apply_torch` is the plain restatement in torch (full-row "
              "`where` / `scatter_` / `unfold`), not a tuned host implementation.  **faster** = the kernel's median is below "
              "`apply_torch`'s fastest window.", "",
              "| B | history | arm | kernel us | apply_torch us | ratio | verdict |", "|---|---|---|---|---|---|---|"]
        for r in krecs:
            k, t = r["kernel_us"], r["torch_us"]
            L.append(f"| {r['B']} | {r['n']} | {r['arm']} | {f3(k)} | {f3(t)} | {t[0] / k[0]:.1f} | "
                     f"{'faster' if k[0] < t[1] else 'NOT faster'} |")
    else:
        L.append("Unmeasured: this part was not run.")
    L += ["", "## (b) ms per decoded token through `generate()`, Llama-3-8B geometry at full depth", ""]
    if grecs:
        new = next(iter(grecs.values()))["new"]
        base_name = "the parent commit" if parent else "THIS tree with the switch off (the parent commit was not measured)"
        L += [f"32 layers, vocabulary 128256, random frozen weights, a text-only prompt of {CTX} tokens, greedy, "
              f"`repetition_penalty=1.2, no_repeat_ngram_size=3`, one-call step (`CAMBRIAN_AMD_DECODE_STEP=1`); ms per decoded token "
              f"= (wall clock of `generate()` for 1 + {new} tokens - that for 1 token, device synchronised) / {new}; median of 3 "
              "windows (min - max), every arm in its own process.  `+ apply_torch`: the same loop with `processors.apply_torch` in "
              f"the kernel's place.  `no processors`: {base_name}.  **faster** = the kernel arm's median is below the "
              "`apply_torch` arm's fastest window; `cost` = kernel arm - no-processor arm.", "",
              "| weights | B | step + kernel | step + apply_torch | no processors | cost ms / token | kernel vs apply_torch |",
              "|---|---|---|---|---|---|---|"]
        for prec in ("bf16", "fp8"):
            for B in BATCHES:
                k, t = grecs.get((f"{prec}-kernel", B)), grecs.get((f"{prec}-torch", B))
                z = grecs.get((f"{prec}-parent", B)) or grecs.get((f"{prec}-none", B))
                if k is None and t is None and z is None:
                    continue
                cell = lambda r: f3(r["ms"]) if r else "unmeasured"
                cost = f"{k['ms'][0] - z['ms'][0]:+.3f}" if k and z else "unmeasured"
                verdict = "unmeasured" if not (k and t) else ("faster" if k["ms"][0] < t["ms"][1] else "NOT faster")
                L.append(f"| {'e4m3' if prec == 'fp8' else prec} | {B} | {cell(k)} | {cell(t)} | {cell(z)} | {cost} | {verdict} |")
        L += ["", "Rows or cells that are missing above are unmeasured."]
    else:
        L.append("Unmeasured: this part was not run.  What one more launch per token costs through `generate()`, and how it compares "
                 "with `apply_torch` in the loop or with the parent commit, is not known.")
    L += ["", "## (c) Resources of `decode_process_kernel` (hipcc, gfx950)", ""]
    if resources:
        L += ["| kernel | VGPRs | AGPRs | SGPRs | LDS bytes | scratch bytes / lane | VGPR spills | SGPR spills | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|---|"]
        for r in resources:
            L.append(f"| `{r['name']}` | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('LDS')} | "
                     f"{r.get('ScratchSize')} | {r.get('VGPRs Spill')} | {r.get('SGPRs Spill')} | {r.get('Occupancy')} |")
    else:
        L.append("Unmeasured.")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(f"wrote {path}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_process.md"))
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--new", type=int, default=64, help="decoded tokens per window")
    ap.add_argument("--quick", action="store_true", help="batch 1 only")
    ap.add_argument("--precisions", default="bf16,fp8")
    ap.add_argument("--parent-tree", help="checkout of the parent commit, library built: the no-processor arm runs there")
    ap.add_argument("--from-log", help="a run's output: write the note again without running anything")
    ap.add_argument("--log", default=os.path.join(tempfile.gettempdir(), "bench_decode_process.log"),
                    help="where the children's records are kept (input of --from-log)")
    ap.add_argument("--resources", help="JSON written by --dump-resources; without it hipcc is run now")
    ap.add_argument("--dump-resources", metavar="FILE")
    ap.add_argument("--kernel-child", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("TREE", "ARM"))
    a = ap.parse_args()
    if a.kernel_child:
        return kernel_child()
    if a.child:
        return generate_child(a.child[0], a.child[1], a.new, a.quick)
    if a.dump_resources:
        with open(a.dump_resources, "w") as fh:
            json.dump(resource_usage("decode_process.hip", "decode_process_kernel"), fh)
        return
    if a.resources:
        with open(a.resources) as fh:
            resources = json.load(fh)
    else:
        resources = resource_usage("decode_process.hip", "decode_process_kernel")
    if a.from_log:
        return write_note(a.out, a.from_log, resources, bool(a.parent_tree))
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    me = os.path.abspath(__file__)
    with open(a.log, "w") as log:
        def run(args, env_extra):
            env = dict(os.environ, **env_extra)
            for k in ("CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_KV_FP8", "CAMBRIAN_AMD_DECODE_SAMPLE", "CAMBRIAN_AMD_DECODE_BEAM"):
                env.pop(k, None)
            p = subprocess.run([sys.executable, me] + args, env=env, capture_output=True, text=True)
            log.write(p.stdout)
            log.flush()
            sys.stdout.write(p.stdout)
            if p.returncode != 0:
                raise SystemExit(f"{args}: exit {p.returncode}\n{p.stderr[-3000:]}")

        if "a" in a.parts:
            run(["--kernel-child"], {"CAMBRIAN_AMD_DECODE_PROCESS": "1"})
        if "b" in a.parts:
            for prec in a.precisions.split(","):
                for mode in ("kernel", "torch", "parent" if a.parent_tree else "none"):
                    tree = a.parent_tree if mode == "parent" else ROOT
                    env = {"CAMBRIAN_AMD_DECODE_STEP": "1", "CAMBRIAN_AMD_DECODE_FP8": "1" if prec == "fp8" else "0",
                           "CAMBRIAN_AMD_DECODE_PROCESS": "1" if mode in ("kernel", "torch") else "0"}
                    run(["--child", tree, f"{prec}-{mode}", "--new", str(a.new)] + (["--quick"] if a.quick else []), env)
    write_note(a.out, a.log, resources, bool(a.parent_tree))


if __name__ == "__main__":
    main()
