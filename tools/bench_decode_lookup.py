"""Prompt-lookup decoding in ``generate()`` (``prompt_lookup_num_tokens``): what a multi-token verify step costs, against the
same calls without the lookup arguments — the per-launch loop and the one-call step (``CAMBRIAN_AMD_DECODE_STEP=1``), both the
parent's code.  tools/bench_decode_step.py's method.

    python tools/bench_decode_lookup.py [--out profiles/decode_lookup.md] [--new 32] [--arms bf16-off,bf16-step,bf16-on,...,kernel]
    python tools/bench_decode_lookup.py --from-log FILE [--parity-log FILE]       # no GPU: the note again from a run's output

Llama-3-8B geometry at full depth (32 layers, vocabulary 128256) with random frozen weights, a text-only prompt of 2048 tokens,
batch 1, bf16 and e4m3 weights (``CAMBRIAN_AMD_DECODE_FP8=1``), greedy.  Each arm runs in a fresh child process, the arms
alternating; what is timed is the host's wall clock of ``generate()`` with the device synchronised,
    ms per emitted token = (T(1 + new tokens) - T(1 token)) / new,
three windows per number (median, min - max).  Random weights copy nothing and their top-2 margins are below bf16 rounding, so the on arm is driven by
``_draft_fn`` oracles with the acceptance FORCED (``lookup.accept`` replaced in the child): every draft kept, the first half of
every draft kept, none kept, with 3 / 7 / 15 drafts per step.  A row is **faster** only when its median
is below the yardstick's fastest window.  The kernel child times ``cmb_decode_attn_multi`` alone (device events) against one
and against Q ``cmb_decode_attn`` calls.  A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX = 2048
TAG = "BENCH_DECODE_LOOKUP "
KTAG = "BENCH_DECODE_LOOKUP_KERNEL "
DRAFTS = (3, 7, 15)
ORACLES = ("all wrong", "half right", "all right")


def child(arm: str, new: int) -> None:
    sys.path.insert(0, ROOT)
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_lookup: no GPU visible")
    prec, switch = arm.split("-")                       # bf16 | fp8, off | step | on
    assert ops.decode_fp8_enabled() == (prec == "fp8") and ops.decode_step_enabled() == (switch == "step")
    dev = torch.device("cuda:0")
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()
    V = cfg.vocab_size
    ids = torch.randint(0, V, (1, CTX), generator=torch.Generator().manual_seed(1)).to(dev)

    def gen(n, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    gen(1 + new)                                        # warm-up
    base = statistics.median(gen(1)[0] for _ in range(3))
    if switch != "on":
        win = [(gen(1 + new)[0] - base) / new for _ in range(3)]
        print(TAG + json.dumps(dict(arm=arm, new=new, prefill_ms=base, ms_token=(statistics.median(win), min(win), max(win)))),
              flush=True)
        return

    # A model of random weights has top-2 margins below the bf16 difference between a batched and a single-token step, so no
    # oracle can know which token a verify step will pick.  The acceptance is therefore FORCED: the drafts are arbitrary ids and
    # ``lookup.accept`` is replaced by the design's count.  A step's cost does not depend on which ids it carries or keeps.
    from cambrian_amd.model.language_model import lookup
    design = {"kind": "all wrong"}

    def forced_accept(draft, picked):
        return {"all right": len(draft), "half right": len(draft) // 2, "all wrong": 0}[design["kind"]]

    lookup.accept = forced_accept

    def oracle(kind):
        def fn(seq, n, *a):
            design["kind"] = kind
            return [(seq[-1] + 1 + i) % V for i in range(n)]
        return fn

    for kind in ORACLES:
        for d in DRAFTS:
            kw = dict(prompt_lookup_num_tokens=d, _draft_fn=oracle(kind))
            gen(1 + new, **kw)                          # warm-up of this row count
            win, per_step = [], []
            for _ in range(3):
                ms, out = gen(1 + new, **kw)
                st = dict(model.lookup_stats)
                win.append((ms - base) / new)
                per_step.append((ms - base) / max(1, st["steps"]))
            print(TAG + json.dumps(dict(arm=arm, new=new, oracle=kind, drafts=d, stats=st,
                                        ms_token=(statistics.median(win), min(win), max(win)),
                                        ms_step=(statistics.median(per_step), min(per_step), max(per_step)))), flush=True)


def kernel_child() -> None:
    sys.path.insert(0, ROOT)
    import torch
    from cambrian_amd import ops
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    nh, nkv, hd, launches = 32, 8, 128, 200
    g = torch.Generator(device=dev).manual_seed(0)
    for keys in (2048, 8192):
        kc = torch.randn(1, nkv, keys + 16, hd, generator=g, device=dev).to(bf)
        vc = torch.randn(1, nkv, keys + 16, hd, generator=g, device=dev).to(bf)
        valid = torch.ones(1, keys + 16, dtype=torch.bool, device=dev)
        for Q in (1, 4, 8, 16):
            t0 = keys - Q
            q = torch.randn(Q, nh * hd, generator=g, device=dev).to(bf)
            k = torch.randn(Q, nkv * hd, generator=g, device=dev).to(bf)
            v = torch.randn(Q, nkv * hd, generator=g, device=dev).to(bf)
            cos, sin = ops.rope_table(torch.arange(t0, t0 + Q, device=dev)[:, None], hd, 5e5)
            rows = [(q[j:j + 1], k[j:j + 1], v[j:j + 1], cos[j:j + 1].contiguous(), sin[j:j + 1].contiguous()) for j in range(Q)]

            def multi():
                ops.decode_attention_multi(q, k, v, cos, sin, kc, vc, t0, valid)

            def one():
                ops.decode_attention(*rows[0], kc, vc, t0 + Q - 1, valid)

            def q_of_them():
                for j in range(Q):
                    ops.decode_attention(*rows[j], kc, vc, t0 + j, valid)

            rec = dict(keys=keys, Q=Q, splits=ops.decode_attention_multi_plan(1, nkv, t0, Q)[0])
            for label, fn in (("multi", multi), ("one", one), ("q_calls", q_of_them)):
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
                rec[label] = (statistics.median(win), min(win), max(win))
            print(KTAG + json.dumps(rec), flush=True)


def f3(t3, digits=3):
    return f"{t3[0]:.{digits}f} ({t3[1]:.{digits}f} - {t3[2]:.{digits}f})"


def write_note(path, recs, kern, parity, new) -> None:
    lines = ["# Prompt-lookup decoding in `generate()`: the cost of a multi-token verify step", "",
             f"Command: `python tools/bench_decode_lookup.py --new {new}` on an MI355X: Llama-3-8B geometry at full depth (32 layers, "
             f"vocabulary 128256), random frozen weights, a text-only prompt of {CTX} tokens, batch 1, greedy.  ms per emitted token "
             f"= (wall clock of `generate()` for 1 + {new} tokens - that for 1 token, device synchronised) / {new}; ms per step = "
             "the same difference over the decode steps the call ran.  Median of 3 windows (min - max), each arm in its own "
             "process, arms alternating.  Yardsticks: the same call without the lookup arguments, on the per-launch loop (`loop`) "
             "and on the one-call step (`CAMBRIAN_AMD_DECODE_STEP=1`, `step`).  Random weights repeat nothing, and their top-2 margins are below the bf16 "
             "difference between a batched and a single-token step, so the drafts are arbitrary ids from a `_draft_fn` oracle and the "
             "acceptance is FORCED (`lookup.accept` replaced in the child: none / the first half / all of every draft kept); a "
             "step's cost does not depend on which ids it carries; the tokens such a run emits are not the model's (what the feature "
             "computes is the subject of tests/test_decode_lookup_gpu.py).  **faster** = the row's median is below the yardstick's fastest "
             "window; anything else is **NOT faster**.  Whether real checkpoints reach the acceptance of a row is not measured here.",
             ""]
    for prec in ("bf16", "fp8"):
        off, step = recs.get((prec + "-off",)), recs.get((prec + "-step",))
        rows = [r for k, r in recs.items() if k[0] == prec + "-on"]
        if off is None and step is None and not rows:
            continue
        lines += [f"## {prec} weights", ""]
        if off is not None:
            lines.append(f"- per-launch loop: {f3(off['ms_token'])} ms per token")
        if step is not None:
            lines.append(f"- one-call step: {f3(step['ms_token'])} ms per token")
        lines += ["", "| oracle | drafts | steps | accepted / drafted | ms per step | ms per emitted token | vs loop | vs step |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            st = r["stats"]

            def verdict(y):
                if y is None:
                    return "-"
                return "faster" if r["ms_token"][0] < y["ms_token"][1] else "NOT faster"
            lines.append(f"| {r['oracle']} | {r['drafts']} | {st['steps']} | {st['accepted']} / {st['drafted']} | "
                         f"{f3(r['ms_step'])} | {f3(r['ms_token'])} | {verdict(off)} | {verdict(step)} |")
        lines.append("")
    if kern:
        lines += ["## The attention kernel alone", "",
                  "`cmb_decode_attn_multi` at 32 query / 8 KV heads of 128, batch 1, bf16, Q new tokens on a cache of `keys` slots "
                  "in all, against ONE `cmb_decode_attn` call (a lower bound: it verifies one token) and against Q of them (what "
                  "verifying Q tokens cost before).  Device events around 200 calls, median of 5 windows (min - max), us per call "
                  "(the Q-calls column: per group of Q).  Verdicts compare with the Q calls.", "",
                  "| keys | Q | splits | multi us | one decode_attn us | Q decode_attn us | multi / one | vs Q calls |", "|---|---|---|---|---|---|---|---|"]
        for r in kern:
            lines.append(f"| {r['keys']} | {r['Q']} | {r['splits']} | {f3(r['multi'], 1)} | {f3(r['one'], 1)} | {f3(r['q_calls'], 1)} | "
                         f"{r['multi'][0] / r['one'][0]:.2f} | {'faster' if r['multi'][0] < r['q_calls'][1] else 'NOT faster'} |")
        lines.append("")
    if parity:
        lines += ["## Parity measured by tests/test_decode_lookup_gpu.py", "",
                  "`rel_err` (max |a - b| / max |b|) of `lookup_step`'s logits against Q successive per-token steps fed the same ids; "
                  "the bound is 2e-2.", "", "| model | weights | Q | t0 | rel_err |", "|---|---|---|---|---|"]
        for r in parity:
            lines.append(f"| {r['lm']} | {r['weights']} | {r['Q']} | {r['t0']} | {r['err']:.3g} |")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def read_parity(path):
    """The lines test_lookup_step_equals_per_token_steps prints (pytest -s)"""
    import re
    out = []
    with open(path) as fh:
        for ln in fh:
            m = re.search(r"lookup_step (\w+) (\w+) Q=(\d+) t0=(\d+): logits rel err against \d+ per-token steps ([0-9.e+-]+)", ln)
            if m:
                out.append(dict(lm=m.group(1), weights=m.group(2), Q=int(m.group(3)), t0=int(m.group(4)), err=float(m.group(5))))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_lookup.md"))
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--arms", default="bf16-off,bf16-on,bf16-step,fp8-off,fp8-on,fp8-step,kernel")
    ap.add_argument("--from-log")
    ap.add_argument("--parity-log")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        kernel_child() if a.child == "kernel" else child(a.child, a.new)
        return
    recs, kern, new = {}, [], a.new

    def take(ln):
        nonlocal new
        if ln.startswith(KTAG):
            kern.append(json.loads(ln[len(KTAG):]))
        elif ln.startswith(TAG):
            r = json.loads(ln[len(TAG):])
            new = r["new"]
            recs[(r["arm"],) if "oracle" not in r else (r["arm"], r["oracle"], r["drafts"])] = r
        else:
            return False
        return True

    if a.from_log:
        with open(a.from_log) as fh:
            for ln in fh:
                take(ln)
    else:
        for arm in [x for x in a.arms.split(",") if x]:
            prec, switch = (arm.split("-") + [""])[:2]
            env = dict(os.environ, CAMBRIAN_AMD_DECODE_FP8="1" if prec == "fp8" else "0",
                       CAMBRIAN_AMD_DECODE_STEP="1" if switch == "step" else "0")
            for k in ("CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_KV_FP8",
                      "CAMBRIAN_AMD_LIB", "PYTHONPATH"):
                env.pop(k, None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--new", str(a.new)]
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_decode_lookup: child {arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if take(ln):
                    print(ln, flush=True)
    write_note(a.out, recs, kern, read_parity(a.parity_log) if a.parity_log else [], new)


if __name__ == "__main__":
    main()
