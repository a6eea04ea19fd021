"""The reusable prompt prefix of ``generate()`` (``prefill_prefix`` / ``generate(prefix=...)``) and its kernel, measured.

    python tools/bench_prefix.py [--out profiles/prefix_cache.md] [--arms kernel,generate,towers]
    python tools/bench_prefix.py --from-log FILE                  # no GPU: the note again from a run's output

(a) ``kernel``: ``cmb_extend_attn`` alone at the Llama-3-8B geometry (32 query / 8 KV heads of 128), bf16, Q in 16 / 64 / 256 new
tokens on t0 in 640 / 2048 cached slots, batch 1 and 8, against ceil(Q / 16) calls of ``cmb_decode_attn_multi`` (what a chunk
cost on the existing kernel; it takes no padded chunk) and against the torch body of ``LlamaAttention.extend`` from the same
projections on (``ops.rope`` on q and k, the cache writes, SDPA under the dense ``ops.extend_mask``).  Device events around 50
calls after 10 warm-up calls, median of 5 windows (min - max), us per call.
(b) ``generate``: a text-only Llama-3-8B geometry at full depth (32 layers, vocabulary 128256), random frozen weights, bf16:
8 questions of 32 tokens over one 640-token head, 8 new tokens each.  The parent's path — 8 calls of ``generate(cat(head,
question))`` — against one ``prefill_prefix`` plus 8 calls of ``generate(question, prefix=)`` and plus ONE call with the 8
questions as a batch.  Host wall clock with the device synchronised, one warm-up pass, median of 5 passes (min - max).
(c) ``towers``: the same comparison on the release-8B model with the four full-size towers, the SVA connector and the in-LLM hook
built with random weights the way ``bench.py`` builds them (``bench.build_model``), an image token in the head.  If that arm
cannot run the note says that the row is missing and why.

A row is **faster** only when its median is below the yardstick's fastest window; anything else is **NOT faster**.  Each arm
runs in a fresh child process.  A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTAG = "BENCH_PREFIX_KERNEL "
GTAG = "BENCH_PREFIX_GENERATE "
TTAG = "BENCH_PREFIX_TOWERS "
HEAD, QUESTION, NEW, QUESTIONS = 640, 32, 8, 8


def kernel_child() -> None:
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from cambrian_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix: no GPU visible")
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    nh, nkv, hd, launches = 32, 8, 128, 50
    g = torch.Generator(device=dev).manual_seed(0)
    for B in (1, 8):
        for t0 in (640, 2048):
            for Q in (16, 64, 256):
                kc = torch.randn(B, nkv, t0 + Q, hd, generator=g, device=dev).to(bf)
                vc = torch.randn(B, nkv, t0 + Q, hd, generator=g, device=dev).to(bf)
                valid = torch.ones(B, t0 + Q, dtype=torch.bool, device=dev)
                q = torch.randn(B * Q, nh * hd, generator=g, device=dev).to(bf)
                k = torch.randn(B * Q, nkv * hd, generator=g, device=dev).to(bf)
                v = torch.randn(B * Q, nkv * hd, generator=g, device=dev).to(bf)
                pos = (t0 + torch.arange(Q, device=dev))[None].expand(B, Q)
                cos, sin = ops.rope_table(pos, hd, 5e5)
                mask = ops.extend_mask(valid, t0, Q)[:, None]
                # the existing kernel takes 16 tokens of every sequence per call: slices of the [B, Q] token grid
                q3, k3, v3 = q.view(B, Q, -1), k.view(B, Q, -1), v.view(B, Q, -1)
                c3, s3 = cos.view(B, Q, -1), sin.view(B, Q, -1)
                parts = [tuple(x[:, j:j + 16].reshape(B * 16, -1).contiguous() for x in (q3, k3, v3, c3, s3)) for j in range(0, Q, 16)]

                def extend():
                    ops.extend_attention(q, k, v, cos, sin, kc, vc, t0, valid)

                def multi_calls():
                    for i, (qq, kk, vv, cc, ss) in enumerate(parts):
                        ops.decode_attention_multi(qq, kk, vv, cc, ss, kc, vc, t0 + 16 * i, valid)

                def torch_body():
                    qr = ops.rope(q.view(B * Q, nh, hd), cos, sin).view(B, Q, nh, hd).transpose(1, 2)
                    kc[:, :, t0:] = ops.rope(k.view(B * Q, nkv, hd), cos, sin).view(B, Q, nkv, hd).transpose(1, 2)
                    vc[:, :, t0:] = v.view(B, Q, nkv, hd).transpose(1, 2)
                    F.scaled_dot_product_attention(qr, kc, vc, attn_mask=mask, enable_gqa=True)

                rec = dict(B=B, t0=t0, Q=Q, splits=ops.extend_attention_plan(B, nkv, t0, Q)[0])
                for label, fn in (("extend", extend), ("multi", multi_calls), ("torch", torch_body)):
                    for _ in range(10):
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


def _time_paths(model, head, qs, tag, **head_kw) -> None:
    """The three paths over one head and QUESTIONS questions, ms for all questions: (median, min, max) of 5 passes."""
    import torch

    def whole():
        for n in range(QUESTIONS):
            model.generate(torch.cat([head, qs[n:n + 1]], 1), max_new_tokens=NEW, **head_kw)

    def singles():
        cache = model.prefill_prefix(head, **head_kw)
        for n in range(QUESTIONS):
            model.generate(qs[n:n + 1], prefix=cache, max_new_tokens=NEW)

    def batch():
        model.generate(qs, prefix=model.prefill_prefix(head, **head_kw), max_new_tokens=NEW)

    def prefix_only():
        model.prefill_prefix(head, **head_kw)

    rec = {}
    for label, fn in (("whole", whole), ("singles", singles), ("batch", batch), ("prefill_prefix", prefix_only)):
        fn()                                            # warm-up
        win = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            win.append((time.perf_counter() - t) * 1e3)
        rec[label] = (statistics.median(win), min(win), max(win))
    print(tag + json.dumps(rec), flush=True)


def generate_child() -> None:
    sys.path.insert(0, ROOT)
    import torch
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix: no GPU visible")
    dev = torch.device("cuda:0")
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()
    gen = torch.Generator().manual_seed(1)
    head = torch.randint(0, cfg.vocab_size, (1, HEAD), generator=gen).to(dev)
    qs = torch.randint(0, cfg.vocab_size, (QUESTIONS, QUESTION), generator=gen).to(dev)
    _time_paths(model, head, qs, GTAG)


def towers_child() -> None:
    """The release-8B model of bench.py (four full-size towers, SVA connector, in-LLM hook, random weights): the head holds the
    image token at ``config.image_position`` and is HEAD ids long before the image expansion."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix: no GPU visible")
    dev = torch.device("cuda:0")
    model, cfg = bench.build_model(dev)
    model.requires_grad_(False).eval()
    gen = torch.Generator().manual_seed(1)
    head = torch.randint(0, cfg.vocab_size, (1, HEAD), generator=gen)
    head[0, cfg.image_position] = -200
    head = head.to(dev)
    qs = torch.randint(0, cfg.vocab_size, (QUESTIONS, QUESTION), generator=gen).to(dev)
    towers = model.get_model().get_vision_tower_aux_list()
    images = [torch.randn(1, 3, t.image_size, t.image_size, generator=gen).to(dev, torch.bfloat16) for t in towers]
    _time_paths(model, head, qs, TTAG, images=images, image_sizes=[(336, 336)])


def f3(t3, digits=1):
    return f"{t3[0]:.{digits}f} ({t3[1]:.{digits}f} - {t3[2]:.{digits}f})"


def verdict(row, yard):
    return "faster" if row[0] < yard[1] else "NOT faster"


def _paths_table(r):
    return ["| path | ms for 8 questions | verdict |", "|---|---|---|",
            f"| 8 x `generate(cat(head, question))` | {f3(r['whole'])} | yardstick |",
            f"| `prefill_prefix` + 8 x `generate(question, prefix=)` | {f3(r['singles'])} | {verdict(r['singles'], r['whole'])} |",
            f"| `prefill_prefix` + 1 x `generate(8 questions, prefix=)` | {f3(r['batch'])} | {verdict(r['batch'], r['whole'])} |",
            f"| (`prefill_prefix` alone) | {f3(r['prefill_prefix'])} | - |", ""]


def write_note(path, kern, gen, tow, tow_missing) -> None:
    lines = ["# Reusable prompt prefix: `cmb_extend_attn` and `generate(prefix=...)`", "",
             "Command: `python tools/bench_prefix.py` on an MI355X.  **faster** = the row's median is below the yardstick's fastest "
             "window; anything else is **NOT faster**.", ""]
    if kern:
        lines += ["## (a) The attention kernel alone", "",
                  "`cmb_extend_attn` at 32 query / 8 KV heads of 128, bf16, Q new tokens per sequence on t0 cached slots, all valid, "
                  "against ceil(Q / 16) calls of `cmb_decode_attn_multi` and against the torch body (`ops.rope` on q and k, the cache "
                  "writes, SDPA under the dense `ops.extend_mask`, the mask built outside the timed region).  Device events around 50 "
                  "calls after 10 warm-up calls, median of 5 windows (min - max), us per call.", "",
                  "| B | t0 | Q | splits | extend us | multi calls us | torch body us | vs multi calls | vs torch body |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in kern:
            lines.append(f"| {r['B']} | {r['t0']} | {r['Q']} | {r['splits']} | {f3(r['extend'])} | {f3(r['multi'])} | {f3(r['torch'])} | "
                         f"{verdict(r['extend'], r['multi'])} | {verdict(r['extend'], r['torch'])} |")
        lines.append("")
    if gen:
        lines += ["## (b) `generate()`: 8 questions over one head", "",
                  f"Text-only Llama-3-8B geometry at full depth (32 layers, vocabulary 128256), random frozen weights, bf16, greedy: "
                  f"{QUESTIONS} questions of {QUESTION} tokens over one head of {HEAD} tokens, {NEW} new tokens each.  Host wall clock "
                  "with the device synchronised, ms for all 8 questions, one warm-up pass, median of 5 passes (min - max).  The "
                  "yardstick is the parent commit's path, 8 calls of `generate(cat(head, question))`.  The decoder alone is timed.", ""]
        lines += _paths_table(gen)
    if tow or tow_missing:
        lines += ["## (c) The same with the towers and the SVA connector in the head", "",
                  "The release-8B model as `bench.py` builds it (`bench.build_model`: CLIP-L, SigLIP, DINOv2 and ConvNeXt-XXL at full "
                  f"size, SVA connector, in-LLM hook, random weights), one 336 x 336 image, the image token inside the {HEAD} head ids "
                  "(the head is longer after the image expansion); everything else as in (b).", ""]
        lines += _paths_table(tow) if tow else [f"**This row is missing**: the arm did not run ({tow_missing}).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_cache.md"))
    ap.add_argument("--arms", default="kernel,generate,towers")
    ap.add_argument("--from-log")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        {"kernel": kernel_child, "generate": generate_child, "towers": towers_child}[a.child]()
        return
    kern, gen, tow, tow_missing = [], {}, {}, ""

    def take(ln):
        if ln.startswith(KTAG):
            kern.append(json.loads(ln[len(KTAG):]))
        elif ln.startswith(GTAG):
            gen.update(json.loads(ln[len(GTAG):]))
        elif ln.startswith(TTAG):
            tow.update(json.loads(ln[len(TTAG):]))
        else:
            return False
        return True

    if a.from_log:
        with open(a.from_log) as fh:
            for ln in fh:
                take(ln)
    else:
        env = dict(os.environ)
        for k in ("CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_FP4",
                  "CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_KV_FP8", "CAMBRIAN_AMD_LIB", "PYTHONPATH"):
            env.pop(k, None)
        for arm in [x for x in a.arms.split(",") if x]:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm]
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
            if p.returncode == 1 and arm == "towers":   # a Python exception in the last arm: the note says the row is missing
                sys.stderr.write(p.stdout + p.stderr)
                tow_missing = (p.stderr.strip().splitlines() or ["exit status 1"])[-1][:200]
                continue
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_prefix: child {arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if take(ln):
                    print(ln, flush=True)
    write_note(a.out, kern, gen, tow, tow_missing)


if __name__ == "__main__":
    main()
