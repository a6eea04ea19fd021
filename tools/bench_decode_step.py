"""Decode steps of ``generate()``: one library call per token (``CAMBRIAN_AMD_DECODE_STEP=1``: ``cmb_decode_next`` +
``cmb_decode_step``) against the per-launch loop (``=0``, the default: the yardstick), same box, same run.

    python tools/bench_decode_step.py [--out profiles/decode_step.md] [--new 64] [--quick] [--parent-tree DIR]
                                      [--yardstick-repeats N]
    python tools/bench_decode_step.py --from-log FILE               # no GPU: the table again from a run's output
    python tools/bench_decode_step.py --dump-resources FILE         # no GPU: hipcc's register / LDS / scratch report
    python tools/bench_decode_step.py --fp4 [--new 32] [--quick]    # the one-call step on MXFP4 / e4m3 / bf16 weights; prints
                                                                    # the records tools/bench_decode_linear.py --fp4 --step-log reads
    python tools/bench_decode_step.py --sample [--out profiles/decode_sample.md] [--new 32] [--arms bf16-on,bf16-off,...]
                                      [--parent-tree DIR] [--from-log FILE] [--resources FILE]     # see ``sample_main``

Llama-3-8B geometry at full depth (32 layers, vocabulary 128256) with random frozen weights, text-only prompt of 2048
tokens, batch 1 / 4 / 16, bf16 weights and e4m3 weights (``CAMBRIAN_AMD_DECODE_FP8=1``), greedy without an eos id and with an
eos id that never fires (a token the greedy run does not produce; the child checks that the tokens stay the same).  Each
arm runs in a fresh child process, the arms alternating.  What is timed is the host's wall clock ``generate()`` with the device synchronised — the host's time per token is the subject — as
    ms per decoded token = (T(1 + new tokens) - T(1 token)) / new
where T(1 token) is the prefill and the first selection alone (median of 3), so the prefill is not in the figure.  Three
windows per number (median, min - max).  A row is **faster** when the on arm's median is below the off arm's fastest window.
``--parent-tree DIR``: a checkout of the parent commit with its own library built; its loop (there is no switch there) is
timed by the same child as one more arm, to show that this tree's off arm is the parent's; ``--yardstick-repeats N`` then
runs the off arm and the parent N more times each at batch 1, alternating, each in a fresh process: how far one arm moves
from process to process, which the three windows of a single process do not show.  A run without a GPU fails; nothing is
estimated."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [1, 4, 16]
CTX = 2048
TAG = "BENCH_DECODE_STEP "
YTAG = "BENCH_DECODE_STEP_YARDSTICK "


def child(tree: str, arm: str, new: int, quick: bool) -> None:
    sys.path.insert(0, tree)
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_step: no GPU visible")
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == os.path.abspath(tree)
    prec, switch = arm.split("-")                       # bf16 | fp8 | fp4, on | off | parent
    assert ops.decode_fp8_enabled() == (prec == "fp8")
    if hasattr(ops, "decode_fp4_enabled"):
        assert ops.decode_fp4_enabled() == (prec == "fp4")
    if switch != "parent":
        assert ops.decode_step_enabled() == (switch == "on")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=dt)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()
    calls = {"step": 0}
    if hasattr(ops, "decode_step"):
        real = ops.decode_step

        def counted(*a, **kw):
            calls["step"] += 1
            return real(*a, **kw)

        ops.decode_step = counted

    def gen(ids, n, eos):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n, eos_token_id=eos)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B in (BATCHES[:1] if quick else BATCHES):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, cfg.vocab_size, (B, CTX), generator=g).to(dev)
        calls["step"] = 0
        _, free = gen(ids, 1 + new, None)               # warm-up of every shape; and the tokens the greedy run produces
        assert free.shape == (B, 1 + new)
        assert calls["step"] == (new if switch == "on" else 0), f"{arm}: {calls['step']} step calls"
        eos = next(v for v in range(cfg.vocab_size) if not bool((free == v).any()))      # never fires
        base = statistics.median(gen(ids, 1, None)[0] for _ in range(3))
        rec = dict(arm=arm, B=B, ctx=CTX, new=new, prefill_ms=base, tokens=free[0, :8].tolist())
        for name, e in (("greedy", None), ("greedy_eos", eos)):
            win = []
            for _ in range(3):
                ms, out = gen(ids, 1 + new, e)
                assert torch.equal(out, free)
                win.append((ms - base) / new)
            rec[name] = (statistics.median(win), min(win), max(win))
        print(TAG + json.dumps(rec), flush=True)
        del ids


def fp4_step_section(log: str) -> list:
    """The lines of profiles/decode_fp4.md's one-call-step table from the output of ``--fp4``"""
    recs = {}
    with open(log) as fh:
        for ln in fh:
            if ln.startswith(TAG):
                r = json.loads(ln[len(TAG):])
                recs[r["arm"], r["B"]] = r

    def f(t3):
        return f"{t3[0]:.3f} ({t3[1]:.3f} - {t3[2]:.3f})"

    new = next(iter(recs.values()))["new"] if recs else 0
    lines = ["## ms per decoded token on the one-call step (`CAMBRIAN_AMD_DECODE_STEP=1`), Llama-3-8B at full depth", "",
             f"`python tools/bench_decode_step.py --fp4 --new {new}`: 32 layers, vocabulary 128256, random frozen weights, a text-only "
             f"prompt of {CTX} tokens, greedy without an eos id; ms per decoded token = (wall clock of `generate()` for 1 + {new} "
             f"tokens - that for 1 token, device synchronised) / {new}.  Median of 3 windows (min - max), each arm in its own "
             "process.  All three arms issue one `cmb_decode_step` per token; what differs is the weight format it streams.  "
             "**faster** = the fp4 median is below the other arm's fastest window.", "",
             "| B | fp4 ms / token | fp8 ms / token | bf16 ms / token | bf16 / fp4 | fp8 / fp4 | vs bf16 | vs fp8 |", "|---|---|---|---|---|---|---|---|"]
    for B in BATCHES:
        o, e, z = recs.get(("fp4-on", B)), recs.get(("fp8-on", B)), recs.get(("bf16-on", B))
        if o is None or e is None or z is None:
            continue
        k = "greedy"
        lines.append(f"| {B} | {f(o[k])} | {f(e[k])} | {f(z[k])} | {z[k][0] / o[k][0]:.2f} | {e[k][0] / o[k][0]:.2f} | "
                     f"{'faster' if o[k][0] < z[k][1] else 'not faster'} | {'faster' if o[k][0] < e[k][1] else 'not faster'} |")
    return lines


def resource_usage(source: str = "decode_next.hip", kernel: str = "decode_next_kernel") -> list:
    """hipcc's kernel-resource-usage remarks for ``kernel`` of ``source`` (no GPU needed)"""
    src = os.path.join(ROOT, "cambrian_amd", "csrc", source)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, cwd=os.path.dirname(src))
    if p.returncode != 0:
        raise SystemExit(p.stderr)
    out, cur = [], None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = dict(name=m.group(1)) if kernel in m.group(1) else None
            if cur is not None:
                out.append(cur)
            continue
        m = re.search(r"remark:\s+.*?(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1) if m.group(1).endswith("Spill") else m.group(1).split(" ")[0]] = int(m.group(2))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# --sample: sampled decoding, token selection on the device (CAMBRIAN_AMD_DECODE_SAMPLE=1) against torch's warpers
# ---------------------------------------------------------------------------------------------------------------------
STAG = "BENCH_DECODE_SAMPLE "
KTAG = "BENCH_DECODE_SAMPLE_KERNEL "
SAMPLERS = [("T", {}), ("T, top_p", dict(top_p=0.9)), ("T, top_k", dict(top_k=50))]
TEMPERATURE = 0.7


def sample_child(tree: str, arm: str, new: int, quick: bool) -> None:
    """One arm of ``--sample``: ``<bf16|fp8>-<on|off|parent>``.  Every arm has the step switch on; ``on`` has the sample switch
    on too, ``off`` is torch's warpers around ``plan.step`` (the yardstick), ``parent`` the parent commit's loop."""
    sys.path.insert(0, tree)
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_step: no GPU visible")
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == os.path.abspath(tree)
    prec, switch = arm.split("-")
    assert ops.decode_fp8_enabled() == (prec == "fp8") and ops.decode_step_enabled()
    if switch != "parent":
        assert ops.decode_sample_enabled() == (switch == "on")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=dt)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()
    calls = {"decode_step": 0, "decode_sample": 0}
    for name in calls:
        if hasattr(ops, name):
            def counted(*a, _real=getattr(ops, name), _name=name, **kw):
                calls[_name] += 1
                return _real(*a, **kw)

            setattr(ops, name, counted)

    def gen(ids, n, eos, kw):
        torch.manual_seed(ids.shape[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n, eos_token_id=eos, do_sample=True, temperature=TEMPERATURE, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B in (BATCHES[:1] if quick else BATCHES):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, cfg.vocab_size, (B, CTX), generator=g).to(dev)
        rec = dict(arm=arm, B=B, ctx=CTX, new=new, windows=0, moved=0)
        for label, kw in SAMPLERS:
            for k in calls:
                calls[k] = 0
            _, free = gen(ids, 1 + new, None, kw)                   # warm-up of every shape
            assert free.shape == (B, 1 + new)
            assert calls["decode_step"] == new and calls["decode_sample"] == ((1 + new) if switch == "on" else 0), (arm, calls)
            base = statistics.median(gen(ids, 1, None, kw)[0] for _ in range(3))
            eos = next(v for v in range(cfg.vocab_size) if not bool((free == v).any()))
            for name, e in (("", None), ("eos", eos)):
                win = []
                for _ in range(3):
                    ms, out = gen(ids, 1 + new, e, kw)
                    # the eos id is a token this arm's run does not draw, so it never fires and every window decodes 1 + new
                    # tokens.  Same seed, same stream: the tokens repeat unless the logits themselves move in their last bits
                    # from run to run, which a draw among near-equal candidates (unlike an argmax) shows; counted, not refused
                    assert out.shape == free.shape and (e is None or not bool((out == e).any())), f"{arm}: B {B} {label}: eos fired"
                    rec["windows"] += 1
                    rec["moved"] += int(not torch.equal(out, free))
                    win.append((ms - base) / new)
                rec[label + "|" + name] = (statistics.median(win), min(win), max(win))
        print(STAG + json.dumps(rec), flush=True)
        del ids


def sample_kernel_child(tree: str) -> None:
    """``cmb_decode_sample`` alone against ``cmb_decode_next`` at V = 128256, B = 1 and 16: device events around 200 launches
    (each followed by its RoPE-table launch), 5 windows."""
    sys.path.insert(0, tree)
    import torch
    from cambrian_amd import ops
    dev = torch.device("cuda:0")
    V, H, hd, launches = 128256, 64, 128, 200
    embed = torch.zeros(V, H, dtype=torch.bfloat16, device=dev)
    seed = torch.tensor([1], dtype=torch.int64, device=dev)
    for B in (1, 16):
        g = torch.Generator(device=dev).manual_seed(B)
        logits = torch.randn(B, (V + 7) // 8 * 8, generator=g, device=dev)[:, :V] * 3
        out = torch.zeros(B, 4, dtype=torch.int64, device=dev)
        pos, n_tok = torch.zeros(B, dtype=torch.int64, device=dev), torch.ones(B, dtype=torch.int64, device=dev)
        kv = torch.zeros(B, 8, dtype=torch.uint8, device=dev)
        x = torch.zeros(B, H, dtype=torch.bfloat16, device=dev)
        cos = torch.zeros(B, hd // 2, dtype=torch.float32, device=dev)
        sin = torch.zeros_like(cos)
        tail = (-1, None, out, 0, n_tok, pos, kv, 0, embed, x, hd, 5e5, cos, sin)
        inv = 1.0 / TEMPERATURE
        what = [("decode_next", lambda: ops.decode_next(logits, *tail)),
                ("decode_sample T", lambda: ops.decode_sample(logits, inv, 0, 1.0, seed, *tail)),
                ("decode_sample T, top_p 0.9", lambda: ops.decode_sample(logits, inv, 0, 0.9, seed, *tail)),
                ("decode_sample T, top_k 50", lambda: ops.decode_sample(logits, inv, 50, 1.0, seed, *tail)),
                ("decode_sample T, top_k 50, top_p 0.9", lambda: ops.decode_sample(logits, inv, 50, 0.9, seed, *tail))]
        for label, fn in what:
            for _ in range(20):
                fn()
            win = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    fn()
                b.record()
                b.synchronize()
                win.append(a.elapsed_time(b) * 1e3 / launches)
            print(KTAG + json.dumps(dict(B=B, what=label, us=(statistics.median(win), min(win), max(win)))), flush=True)


def sample_main(a) -> None:
    """``--sample``: writes profiles/decode_sample.md.  Arms ``<bf16|fp8>-<on|off|parent>`` and ``kernel``, each a fresh child
    process, on / off alternating; ``--arms`` runs a subset (a GPU session has a time limit: the runs' outputs, concatenated,
    make the table through ``--from-log``)."""
    out_path = a.out if a.out != os.path.join(ROOT, "profiles", "decode_step.md") else os.path.join(ROOT, "profiles", "decode_sample.md")
    arms = []
    for prec in ("bf16", "fp8"):
        arms += [prec + "-on", prec + "-off"] + ([prec + "-parent"] if a.parent_tree and prec == "bf16" else [])
    arms.append("kernel")
    if a.arms:
        arms = [x for x in a.arms.split(",") if x]
    recs, kern = {}, []
    if a.from_log:
        with open(a.from_log) as fh:
            for ln in fh:
                if ln.startswith(KTAG):
                    kern.append(json.loads(ln[len(KTAG):]))
                elif ln.startswith(STAG):
                    r = json.loads(ln[len(STAG):])
                    recs[r["arm"], r["B"]] = r
    else:
        for arm in arms:
            tree = a.parent_tree if arm.endswith("-parent") else ROOT
            prec, switch = (arm.split("-") + [""])[:2]
            env = dict(os.environ, CAMBRIAN_AMD_DECODE_FP8="1" if prec == "fp8" else "0", CAMBRIAN_AMD_DECODE_STEP="1",
                       CAMBRIAN_AMD_DECODE_SAMPLE="1" if switch == "on" else "0")
            for k in ("CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_LIB", "PYTHONPATH"):
                env.pop(k, None)
            cmd = [sys.executable, os.path.abspath(__file__), "--sample", "--child", os.path.abspath(tree), arm, "--new", str(a.new)] \
                + (["--quick"] if a.quick else [])
            p = subprocess.run(cmd, env=env, cwd=os.path.abspath(tree), capture_output=True, text=True, timeout=540)
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_decode_step --sample: child {arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if ln.startswith(KTAG):
                    kern.append(json.loads(ln[len(KTAG):]))
                    print(ln, flush=True)
                elif ln.startswith(STAG):
                    r = json.loads(ln[len(STAG):])
                    recs[r["arm"], r["B"]] = r
                    print(ln, flush=True)
    if a.resources:
        with open(a.resources) as fh:
            res = json.load(fh)
    else:
        res = resource_usage("decode_sample.hip", "decode_sample_kernel")

    def f(t3):
        return f"{t3[0]:.3f} ({t3[1]:.3f} - {t3[2]:.3f})"

    lines = ["# Sampled decoding in `generate()`: token selection on the device against torch's warpers", "",
             f"Command: `python tools/bench_decode_step.py --sample --new {a.new}`" + (" `--quick`" if a.quick else "")
             + (" `--parent-tree <checkout of the parent commit>`" if any(k[0].endswith("parent") for k in recs) else ""),
             "on an MI355X: Llama-3-8B geometry at full depth (32 layers, vocabulary 128256), random frozen weights, a text-only "
             f"prompt of {CTX} tokens, `do_sample=True`, temperature {TEMPERATURE} alone (`T`), with `top_p=0.9`, with `top_k=50`.  "
             f"ms per decoded token = (wall clock of `generate()` for 1 + {a.new} tokens - that for 1 token, device synchronised) "
             f"/ {a.new}.  Median of 3 windows (min - max in brackets), each arm in its own process, arms alternating.  Both arms "
             "run with `CAMBRIAN_AMD_DECODE_STEP=1`; `on` = `CAMBRIAN_AMD_DECODE_SAMPLE=1` (`cmb_decode_sample` + "
             "`cmb_decode_step`, two library calls per token), `off` = `0` (torch's warpers, `multinomial` and the embedding lookup "
             "around `plan.step`: the yardstick).  `eos` = an eos id the run does not draw, so it never fires: the off arm then "
             "reads `done` back every token, the on arm every 8.  A row is **faster** when the on arm's median is below the off "
             "arm's fastest window.  The two arms draw different random streams, so their tokens differ; every window of an arm "
             "repeats that arm's tokens under one seed.", "",
             "| weights | B | sampler | eos | on ms / token | off ms / token | off / on | verdict |", "|---|---|---|---|---|---|---|---|"]
    slow = []
    keys = [label + "|" + e for label, _ in SAMPLERS for e in ("", "eos")]
    for prec in ("bf16", "fp8"):
        for B in BATCHES:
            o, z = recs.get((prec + "-on", B)), recs.get((prec + "-off", B))
            if o is None or z is None:
                continue
            for k in keys:
                label, e = k.split("|")
                fast = o[k][0] < z[k][1]
                if not fast:
                    slow.append(f"{prec} B {B} {label}{' eos' if e else ''}")
                lines.append(f"| {prec} | {B} | {label} | {'yes' if e else 'no'} | {f(o[k])} | {f(z[k])} | {z[k][0] / o[k][0]:.2f} | "
                             f"{'faster' if fast else 'not faster'} |")
    lines += ["", "Not faster: " + ("; ".join(slow) if slow else "nowhere") + ".",
              "The switch stays off by default whatever this table says.", ""]
    moved = {sw: (sum(r.get("moved", 0) for k, r in recs.items() if k[0].endswith(sw)),
                  sum(r.get("windows", 0) for k, r in recs.items() if k[0].endswith(sw))) for sw in ("-on", "-off")}
    lines += ["Timed windows whose tokens differed from the same arm's first run under the same seed: "
              f"on {moved['-on'][0]} of {moved['-on'][1]}, off {moved['-off'][0]} of {moved['-off'][1]} (the sampler is "
              "deterministic given its logits; a draw among near-equal candidates shows a last-bit difference in the logits of "
              "two runs, which an argmax hides).  No window's eos id fired.", ""]
    if any(k[0].endswith("parent") for k in recs):
        lines += ["## The yardstick: this tree's off arm against the parent commit's loop", "",
                  "The parent commit (its own sources and its own build of the library, step switch on) timed by the same child as "
                  "one more arm.  `moved` = the distance of the two medians, `spread` = the wider of the two arms' windows.", "",
                  "| B | sampler | eos | off ms / token | parent ms / token | moved | spread | moved / parent |",
                  "|---|---|---|---|---|---|---|---|"]
        for B in BATCHES:
            z, p = recs.get(("bf16-off", B)), recs.get(("bf16-parent", B))
            if z is None or p is None:
                continue
            for k in keys:
                label, e = k.split("|")
                moved = abs(z[k][0] - p[k][0])
                spread = max(z[k][2] - z[k][1], p[k][2] - p[k][1])
                lines.append(f"| {B} | {label} | {'yes' if e else 'no'} | {f(z[k])} | {f(p[k])} | {moved:.3f} | {spread:.3f} | "
                             f"{moved / p[k][0] * 100:.2f} % |")
        lines.append("")
    if kern:
        lines += ["## The kernel alone", "",
                  "V = 128256, fp32 logits `randn * 3` with lm_head's padded row stride, device events around 200 launches (each "
                  "followed by its `cmb_rope_table` launch), median of 5 windows (min - max).", "",
                  "| B | call | us / call |", "|---|---|---|"]
        for r in kern:
            lines.append(f"| {r['B']} | `{r['what']}` | {r['us'][0]:.1f} ({r['us'][1]:.1f} - {r['us'][2]:.1f}) |")
        lines.append("")
    lines += ["## Kernel resource usage of `decode_sample_kernel` (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950)", "",
              "| VGPRs | AGPRs | SGPRs | VGPR spills | SGPR spills | LDS bytes | scratch bytes / lane | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('VGPRs Spill')} | {r.get('SGPRs Spill')} | "
                     f"{r.get('LDS')} | {r.get('ScratchSize')} | {r.get('Occupancy')} |")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_step.md"))
    ap.add_argument("--new", type=int, default=64, help="decoded tokens per window")
    ap.add_argument("--quick", action="store_true", help="batch 1 only (rehearsal)")
    ap.add_argument("--parent-tree", help="checkout of the parent commit, library built: one more arm")
    ap.add_argument("--yardstick-repeats", type=int, default=0, help="with --parent-tree: extra off / parent runs at batch 1")
    ap.add_argument("--from-log", help="a run's output: write the table again without running anything")
    ap.add_argument("--resources", help="JSON written by --dump-resources; without it hipcc is run now")
    ap.add_argument("--dump-resources", metavar="FILE")
    ap.add_argument("--child", nargs=2, metavar=("TREE", "ARM"))
    ap.add_argument("--sample", action="store_true", help="sampled decoding: the device sampler against torch's warpers")
    ap.add_argument("--arms", help="with --sample: a comma-separated subset of the arms to run")
    ap.add_argument("--fp4", action="store_true", help="the one-call step on MXFP4, e4m3 and bf16 weights (records on stdout)")
    a = ap.parse_args()
    if a.dump_resources:
        with open(a.dump_resources, "w") as fh:
            json.dump(resource_usage("decode_sample.hip", "decode_sample_kernel") if a.sample else resource_usage(), fh, indent=1)
        return
    if a.new < 16:
        ap.error("--new: at least 16")
    if a.sample:
        if a.child and a.child[1] == "kernel":
            sample_kernel_child(a.child[0])
        elif a.child:
            sample_child(a.child[0], a.child[1], a.new, a.quick)
        else:
            sample_main(a)
        return
    if a.child:
        child(a.child[0], a.child[1], a.new, a.quick)
        return
    arms = [("bf16-on", ROOT), ("bf16-off", ROOT)] + ([("bf16-parent", a.parent_tree)] if a.parent_tree else []) \
        + [("fp8-on", ROOT), ("fp8-off", ROOT)]
    if a.fp4:
        arms = [("fp4-on", ROOT), ("fp8-on", ROOT), ("bf16-on", ROOT)]
    recs, extra = {}, []

    def run(arm, tree, quick):
        prec, switch = arm.split("-")
        env = dict(os.environ, CAMBRIAN_AMD_DECODE_FP8="1" if prec == "fp8" else "0",
                   CAMBRIAN_AMD_DECODE_FP4="1" if prec == "fp4" else "0", CAMBRIAN_AMD_DECODE_STEP="1" if switch == "on" else "0")
        for k in ("CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_LIB", "PYTHONPATH"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(tree), arm, "--new", str(a.new)] \
            + (["--quick"] if quick else [])
        p = subprocess.run(cmd, env=env, cwd=os.path.abspath(tree), capture_output=True, text=True, timeout=420)
        if p.returncode != 0:                       # a child that failed ends the run: nothing else is started on the GPU
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"bench_decode_step: child {arm} exited with {p.returncode}")
        return [json.loads(ln[len(TAG):]) for ln in p.stdout.splitlines() if ln.startswith(TAG)]

    if a.from_log:
        with open(a.from_log) as fh:
            for ln in fh:
                if ln.startswith(YTAG):
                    extra.append(json.loads(ln[len(YTAG):]))
                elif ln.startswith(TAG):
                    r = json.loads(ln[len(TAG):])
                    recs[r["arm"], r["B"]] = r
        a.parent_tree = a.parent_tree or ("parent" if any(k[0] == "bf16-parent" for k in recs) else None)
    else:
        for arm, tree in arms:
            for r in run(arm, tree, a.quick):
                recs[r["arm"], r["B"]] = r
                print(TAG + json.dumps(r), flush=True)
        for _ in range(a.yardstick_repeats if a.parent_tree else 0):
            for arm, tree in (("bf16-off", ROOT), ("bf16-parent", a.parent_tree)):
                for r in run(arm, tree, True):
                    extra.append(r)
                    print(YTAG + json.dumps(r), flush=True)
    if a.fp4:           # the records are on stdout; profiles/decode_fp4.md is written by tools/bench_decode_linear.py --fp4 --step-log
        return
    if a.resources:
        with open(a.resources) as fh:
            res = json.load(fh)
    else:
        res = resource_usage()

    def f(t3):
        return f"{t3[0]:.3f} ({t3[1]:.3f} - {t3[2]:.3f})"

    lines = ["# Decode steps of `generate()`: one library call per token against the per-launch loop", "",
             f"Command: `python tools/bench_decode_step.py --new {a.new}`" + (" `--quick`" if a.quick else "")
             + (" `--parent-tree <checkout of the parent commit>`" if a.parent_tree else "")
             + (f" `--yardstick-repeats {len(extra) // 2}`" if extra else ""),
             f"on an MI355X: Llama-3-8B geometry at full depth (32 layers, vocabulary 128256), random frozen weights, a text-only "
             f"prompt of {CTX} tokens, greedy.  ms per decoded token = (wall clock of `generate()` for 1 + {a.new} tokens - that "
             "for 1 token, device synchronised) / " + f"{a.new}: the prefill is not in the figure, the host's time per token is.  "
             "Median of 3 windows (min - max in brackets), each arm in its own process, arms alternating.  `on` = "
             "`CAMBRIAN_AMD_DECODE_STEP=1` (`cmb_decode_next` + `cmb_decode_step`, two library calls per token), `off` = `0` (the "
             "per-launch loop, unchanged by this switch: the yardstick).  `eos` = an eos id that never fires: the off arm then "
             "reads `done` back every token, the on arm every 8.  A row is **faster** when the on arm's median is below the off "
             "arm's fastest window.", "",
             "| weights | B | loop | on ms / token | off ms / token | off / on | verdict |", "|---|---|---|---|---|---|---|"]
    slow = []
    for prec in ("bf16", "fp8"):
        for B in BATCHES:
            o, z = recs.get((prec + "-on", B)), recs.get((prec + "-off", B))
            if o is None or z is None:
                continue
            assert o["tokens"] == z["tokens"], "the arms decoded different tokens"
            for name, label in (("greedy", "greedy"), ("greedy_eos", "greedy, eos")):
                fast = o[name][0] < z[name][1]
                if not fast:
                    slow.append(f"{prec} B {B} {label}")
                lines.append(f"| {prec} | {B} | {label} | {f(o[name])} | {f(z[name])} | {z[name][0] / o[name][0]:.2f} | "
                             f"{'faster' if fast else 'not faster'} |")
    lines += ["", "Not faster: " + ("; ".join(slow) if slow else "nowhere") + ".",
              "The switch stays off by default whatever this table says.", ""]
    if a.parent_tree:
        lines += ["## The yardstick: this tree's off arm against the parent commit's loop", "",
                  "The parent commit (its own sources and its own build of the library) timed by the same child process as one "
                  "more arm.  `moved` = the distance of the two medians, `spread` = the wider of the two arms' windows (max - "
                  "min).", "",
                  "| B | loop | off ms / token | parent ms / token | moved | spread | moved / parent |", "|---|---|---|---|---|---|---|"]
        for B in BATCHES:
            z, p = recs.get(("bf16-off", B)), recs.get(("bf16-parent", B))
            if z is None or p is None:
                continue
            for name, label in (("greedy", "greedy"), ("greedy_eos", "greedy, eos")):
                moved = abs(z[name][0] - p[name][0])
                spread = max(z[name][2] - z[name][1], p[name][2] - p[name][1])
                lines.append(f"| {B} | {label} | {f(z[name])} | {f(p[name])} | {moved:.3f} | {spread:.3f} | {moved / p[name][0] * 100:.2f} % |")
        lines.append("")
        if extra:
            lines += [f"Batch 1 again, {len(extra) // 2} more fresh processes per arm, alternating (median of 3 windows each): the windows of "
                      "one process are narrower than the distance between two processes of the same arm, so that distance, not "
                      "the windows' spread, is the resolution of the comparison above.", "",
                      "| arm | greedy ms / token, per process | greedy, eos ms / token, per process |", "|---|---|---|"]
            for arm in ("bf16-off", "bf16-parent"):
                rs = [r for r in extra if r["arm"] == arm]
                lines.append(f"| {arm[5:]} | " + ", ".join(f"{r['greedy'][0]:.3f}" for r in rs) + " | "
                             + ", ".join(f"{r['greedy_eos'][0]:.3f}" for r in rs) + " |")
            lines.append("")
    lines += ["## Kernel resource usage of `decode_next_kernel` (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950)", "",
              "| VGPRs | AGPRs | SGPRs | VGPR spills | SGPR spills | LDS bytes | scratch bytes / lane | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('VGPRs Spill')} | {r.get('SGPRs Spill')} | "
                     f"{r.get('LDS')} | {r.get('ScratchSize')} | {r.get('Occupancy')} |")
    lines.append("(`cmb_decode_step` launches no kernel of its own.)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
