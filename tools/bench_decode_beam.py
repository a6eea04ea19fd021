"""Beam search in ``generate()``: the device path (``CAMBRIAN_AMD_DECODE_BEAM=1`` with ``CAMBRIAN_AMD_DECODE_STEP=1``:
``cmb_decode_beam`` + ``cmb_decode_step``, two library calls per token) against the host path of the same commit
(model/language_model/beam.py and an ``index_select`` of the generated cache columns around ``plan.step``) and against the floor,
greedy decoding of ``prompts * num_beams`` rows through ``cmb_decode_next`` + ``cmb_decode_step`` (code this switch does not
touch).

    python tools/bench_decode_beam.py [--new 32] [--quick] > LOG           # on a GPU: one JSON line per measurement
    python tools/bench_decode_beam.py --kernels                             # the selection and the reorder alone (also what a
                                                                            # `rocprofv3 --kernel-trace --stats` run traces)
    python tools/bench_decode_beam.py --from-log LOG [--kernel-stats CSV] [--accuracy "TEXT"] [--out profiles/decode_beam.md]

Llama-3-8B geometry at full depth (32 layers, vocabulary 128256), random frozen weights, a text-only prompt of 2048 tokens, bf16
and e4m3 weights, ``num_beams`` 2 / 4 / 8 at one prompt and 4 at two prompts, no eos id (every arm decodes the same number of
tokens).  One process; the three arms of a configuration alternate window by window.  What is timed is the host's wall clock
around ``generate()`` with the device synchronised:
    ms per decoded token = (T(1 + new tokens) - T(1 + new / 2 tokens)) / (new / 2)
(the shorter call, median of 3, takes the prefill, the cache set-up and the first selection out of the figure; a call of one
token would not do, it never builds the plan), three windows per figure.  The host arm is reached by
setting ``ops.DECODE_BEAM_MAX = 0``, which sends ``_beam_search`` to its host loop with the plan in place.  No ratio is a
pass / fail bound: the report states the overhead over the floor and the gain over the host path next to the windows' spread.
A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CTX = 2048
CONFIGS = [(1, 2), (1, 4), (1, 8), (2, 4)]
TAG, KTAG = "BENCH_DECODE_BEAM ", "BENCH_DECODE_BEAM_KERNEL "


def _events(fn, launches=100, windows=5):
    import torch
    for _ in range(10):
        fn()
    win = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        win.append(a.elapsed_time(b) * 1e3 / launches)
    return statistics.median(win), min(win), max(win)


def kernels() -> None:
    """``decode_beam`` without caches (rows + group + flag + RoPE table) and the reorder alone, device events."""
    import torch
    from cambrian_amd import lib as L, ops
    from cambrian_amd.model.language_model import beam as BM
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_beam: no GPU visible")
    dev = torch.device("cuda:0")
    V, H, hd, nkv, layers, M, L0 = 128256, 4096, 128, 8, 32, 64, CTX
    embed = torch.zeros(V, H, dtype=torch.bfloat16, device=dev)
    for B, nb in CONFIGS:
        R = B * nb
        g = torch.Generator(device=dev).manual_seed(R)
        logits = torch.randn(R, (V + 7) // 8 * 8, generator=g, device=dev)[:, :V] * 3
        st = BM.BeamState(B, nb, M, dev)
        for s in range(3):
            BM.beam_update(st, torch.randn(R, 4096, generator=g, device=dev), s, None, False)
        state = ops.DecodeBeamState(B, nb, M, dev)
        state.run_score.copy_(st.run_score.reshape(-1))
        state.unsat.fill_(1)
        state.fin_score.fill_(-1e9)
        keep = state.buf.clone()
        pos, n_tok = torch.zeros(R, dtype=torch.int64, device=dev), torch.full((R,), CTX, dtype=torch.int64, device=dev)
        kv = torch.zeros(R, CTX + M, dtype=torch.uint8, device=dev)
        x = torch.zeros(R, H, dtype=torch.bfloat16, device=dev)
        cos = torch.zeros(R, hd // 2, dtype=torch.float32, device=dev)
        sin = torch.zeros_like(cos)

        def select():
            state.buf.copy_(keep)                              # every call starts from the same state (a 100 KB copy)
            ops.decode_beam(logits, nb, -1, state, 3, n_tok, pos, kv, L0 + 3, embed, x, hd, 5e5, cos, sin)

        us = _events(select)
        copy = _events(lambda: state.buf.copy_(keep))
        print(KTAG + json.dumps(dict(B=B, nb=nb, what="selection: rows + group + flag + RoPE table", us=us, copy_us=copy)), flush=True)
        caches = [torch.randn(R, nkv, CTX + M, hd, device=dev).to(torch.bfloat16) for _ in range(2 * layers)]
        rows = []
        for l in range(layers):
            row = L.DecodeLayer()
            row.kcache, row.vcache = caches[2 * l].data_ptr(), caches[2 * l + 1].data_ptr()
            rows.append(row)
        kc = caches[0]
        desc = L.DecodeStepDesc(B=R, layers=layers, nkv=nkv, hd=hd, c_sb=kc.stride(0), c_sh=kc.stride(1), c_st=kc.stride(2))
        table = (L.DecodeLayer * layers)(*rows)
        for name, par in (("a rotation of every prompt's rows", [(i + 1) % nb for _ in range(B) for i in range(nb)]),
                          ("the identity (skipped)", [i for _ in range(B) for i in range(nb)])):
            parent = torch.tensor(par, dtype=torch.int32, device=dev)
            for G in (1, 16, 63):
                us = _events(lambda: ops.decode_beam_reorder(desc, table, parent, nb, L0, L0 + G))
                moved = 2 * G * layers * 2 * nkv * hd * R * 2 if "rotation" in name else 0
                print(KTAG + json.dumps(dict(B=B, nb=nb, what=f"reorder, {G} generated columns, {name}", us=us, bytes=moved)),
                      flush=True)
        del caches


def bench(new: int, quick: bool) -> None:
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_beam: no GPU visible")
    dev = torch.device("cuda:0")
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()
    os.environ["CAMBRIAN_AMD_DECODE_STEP"] = "1"
    os.environ["CAMBRIAN_AMD_DECODE_BEAM"] = "1"
    calls = {"decode_beam": 0, "decode_step": 0, "decode_next": 0}
    for name in calls:
        def counted(*a, _real=getattr(ops, name), _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        setattr(ops, name, counted)
    beam_max = ops.DECODE_BEAM_MAX

    def run(arm, ids, nb, n):
        ops.DECODE_BEAM_MAX = 0 if arm == "host" else beam_max
        for k in calls:
            calls[k] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if arm == "floor":
            out = model.generate(ids.repeat_interleave(nb, 0), max_new_tokens=n)
        else:
            out = model.generate(ids, max_new_tokens=n, num_beams=nb)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        ops.DECODE_BEAM_MAX = beam_max
        want = dict(fused=(n, n - 1, 0), host=(0, n - 1, 0), floor=(0, n - 1, n))[arm]
        assert n == 1 or (calls["decode_beam"], calls["decode_step"], calls["decode_next"]) == want, (arm, calls)
        return ms, out

    arms = ("fused", "host", "floor")
    for prec in ("bf16", "fp8"):
        os.environ["CAMBRIAN_AMD_DECODE_FP8"] = "1" if prec == "fp8" else "0"
        for B, nb in (CONFIGS[:1] if quick else CONFIGS):
            g = torch.Generator().manual_seed(B)
            ids = torch.randint(0, cfg.vocab_size, (B, CTX), generator=g).to(dev)
            toks = {arm: run(arm, ids, nb, 1 + new)[1] for arm in arms}             # warm-up of every shape
            half = new // 2
            base = {arm: statistics.median(run(arm, ids, nb, 1 + half)[0] for _ in range(3)) for arm in arms}
            win = {arm: [] for arm in arms}
            for _ in range(3):
                for arm in arms:
                    ms, out = run(arm, ids, nb, 1 + new)
                    win[arm].append((ms - base[arm]) / (new - half))
            rec = dict(prec=prec, B=B, nb=nb, ctx=CTX, new=new, same_tokens=bool(torch.equal(toks["fused"], toks["host"])))
            for arm in arms:
                rec[arm] = (statistics.median(win[arm]), min(win[arm]), max(win[arm]))
                rec[arm + "_half_ms"] = base[arm]
            print(TAG + json.dumps(rec), flush=True)
            del ids


def report(log: str, out_path: str, stats_csv: str, accuracy: str) -> None:
    recs, kern = [], []
    with open(log) as fh:
        for ln in fh:
            if ln.startswith(KTAG):
                kern.append(json.loads(ln[len(KTAG):]))
            elif ln.startswith(TAG):
                recs.append(json.loads(ln[len(TAG):]))

    def f(t3):
        return f"{t3[0]:.3f} ({t3[1]:.3f} - {t3[2]:.3f})"

    new = recs[0]["new"] if recs else 0
    lines = ["# Beam search in `generate()`: the device path against the host path and the greedy floor", "",
             f"Command: `python tools/bench_decode_beam.py --new {new}` on an MI355X: Llama-3-8B geometry at full depth (32 layers, "
             f"vocabulary 128256), random frozen weights, a text-only prompt of {CTX} tokens, no eos id.  ms per decoded token = (wall "
             f"clock of `generate()` for 1 + {new} tokens - that for 1 + {new // 2} tokens, device synchronised) / {new - new // 2}: tokens "
             f"{new // 2 + 1} to {new} of a call, with {new // 2} to {new - 1} generated columns to reorder.  Median of 3 windows (min - "
             "max in brackets), one process, the arms alternating window by window.  `fused` = `cmb_decode_beam` + `cmb_decode_step` "
             "(two library calls per token), `host` = the same commit's host loop (beam.py's torch selection, an `index_select` of the "
             "generated cache columns, the embedding lookup and the RoPE table around `plan.step`), `floor` = greedy decoding of "
             "prompts x num_beams rows through `cmb_decode_next` + `cmb_decode_step`.  The floor's code is not touched by this "
             "switch, so it is measured on this commit.  `spread` = the widest window range (max - min) of the three arms.  No ratio "
             "here is a pass / fail bound.", "",
             "| weights | prompts | num_beams | fused ms / token | host ms / token | floor ms / token | fused - floor | host / fused | spread "
             "| same tokens |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        spread = max(r[a][2] - r[a][1] for a in ("fused", "host", "floor"))
        lines.append(f"| {r['prec']} | {r['B']} | {r['nb']} | {f(r['fused'])} | {f(r['host'])} | {f(r['floor'])} | "
                     f"{r['fused'][0] - r['floor'][0]:+.3f} ({(r['fused'][0] / r['floor'][0] - 1) * 100:+.1f} %) | "
                     f"{r['host'][0] / r['fused'][0]:.2f} | {spread:.3f} | {'yes' if r['same_tokens'] else 'no'} |")
    lines += ["", "`same tokens`: whether the fused and the host arm returned the same ids on these random weights (their logits carry "
              "the same bits; the selections differ in the last bits of the log-sum-exp, so a near-tie may resolve the other way).", ""]
    if kern:
        lines += ["## The launches alone", "",
                  "V = 128256, fp32 logits `randn * 3` with lm_head's padded row stride, a state after three steps; 32 layers of bf16 "
                  "caches [rows, 8, 2112, 128]; device events around 100 calls, median of 5 windows (min - max).  The selection call "
                  "is preceded by a copy that restores the state block, timed alone in the last column.", "",
                  "| prompts | num_beams | call | us / call | bytes moved | GB/s | state copy us |", "|---|---|---|---|---|---|---|"]
        for r in kern:
            by = r.get("bytes")
            lines.append(f"| {r['B']} | {r['nb']} | {r['what']} | {r['us'][0]:.1f} ({r['us'][1]:.1f} - {r['us'][2]:.1f}) | "
                         f"{by if by else '-'} | {by / r['us'][0] / 1e3:.0f} | {'-' if 'copy_us' not in r else format(r['copy_us'][0], '.1f')} |"
                         if by else
                         f"| {r['B']} | {r['nb']} | {r['what']} | {r['us'][0]:.1f} ({r['us'][1]:.1f} - {r['us'][2]:.1f}) | - | - | "
                         f"{'-' if 'copy_us' not in r else format(r['copy_us'][0], '.1f')} |")
        lines.append("")
    if stats_csv:
        lines += ["## Per kernel (`rocprofv3 --kernel-trace --stats` around `--kernels`, a run of its own)", "",
                  "| kernel | calls | average us | min us | max us |", "|---|---|---|---|---|"]
        with open(stats_csv) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                if "decode_beam" not in name and "rope_table" not in name:
                    continue
                lines.append(f"| `{name.split('(')[0][-60:]}` | {row.get('Calls')} | {float(row.get('AverageNs', 0)) / 1e3:.1f} | "
                             f"{float(row.get('MinNs', 0)) / 1e3:.1f} | {float(row.get('MaxNs', 0)) / 1e3:.1f} |")
        lines.append("")
    if accuracy:
        lines += ["## Accuracy of the scores", "", accuracy, ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=32, help="decoded tokens per window")
    ap.add_argument("--quick", action="store_true", help="the first configuration only (rehearsal)")
    ap.add_argument("--kernels", action="store_true", help="the selection and the reorder alone")
    ap.add_argument("--from-log", help="a run's output: write the report without running anything")
    ap.add_argument("--kernel-stats", help="with --from-log: rocprofv3's kernel stats CSV of a --kernels run")
    ap.add_argument("--accuracy", help="with --from-log: the accuracy paragraph (figures printed by tests/test_decode_beam_gpu.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_beam.md"))
    a = ap.parse_args()
    if a.from_log:
        report(a.from_log, a.out, a.kernel_stats, a.accuracy)
    elif a.kernels:
        kernels()
    else:
        bench(a.new, a.quick)


if __name__ == "__main__":
    main()
