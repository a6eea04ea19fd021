"""Decode steps of ``generate()`` on an e4m3 K / V cache (``CAMBRIAN_AMD_DECODE_KV_FP8=1``, cmb_decode_attn_kv8) against the
bf16 cache (``=0``, the default: the yardstick), same tree, same run.  Writes profiles/decode_kv8.md.

    python tools/bench_decode_kv8.py [--out profiles/decode_kv8.md] [--new 32] [--ctx 2048,8192] [--batches 1,4,16]
                                     [--weights bf16,fp8] [--log FILE] [--skip-errors]
    python tools/bench_decode_kv8.py --kernel-child                  # the attention call alone; prints records for --from-log
    python tools/bench_decode_kv8.py --from-log FILE [--out ...]     # no GPU: the note again from a run's output
    python tools/bench_decode_kv8.py --not-measured [--out ...]      # no GPU: the note with the resource table only

The method is tools/bench_decode_step.py's.  Llama-3-8B geometry at full depth (32 layers, vocabulary 128256) with random
frozen weights, text-only prompts of 2048 and 8192 tokens, batch 1 / 4 / 16, bf16 weights and e4m3 weights
(``CAMBRIAN_AMD_DECODE_FP8=1``), greedy without an eos id, the one-call step (``CAMBRIAN_AMD_DECODE_STEP=1``) on in both arms.
Each arm runs in a fresh child process, the arms alternating.  What is timed is the host's wall clock of ``generate()`` with
the device synchronised,
    ms per decoded token = (T(1 + new tokens) - T(1 token)) / new
where T(1 token) is the prefill (with the e4m3 cache: the prefill and the quantisation of its K / V) and the first selection
alone (median of 3).  Three windows per number (median, min - max).  A row is **faster** only when the on arm's median is
below the off arm's fastest window.  Peak memory is ``torch.cuda.max_memory_allocated`` over one ``generate()`` of 1 + new
tokens, the weights included.  A child of its own measures what the cache costs in accuracy: the relative L2 error of the
attention output against the bf16 cache on Gaussian K / V at 2048 keys, and that of the first decode step's logits on the
tiny model of tests/test_decode_kv8_gpu.py; another times the attention call alone (``kernel_child``), which reaches 16 rows
x 8192 keys — the ``generate()`` arms were run up to 32768 prompt tokens per call.  A run without a GPU fails; nothing is
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
TAG = "BENCH_DECODE_KV8 "
ETAG = "BENCH_DECODE_KV8_ERROR "
KTAG = "BENCH_DECODE_KV8_KERNEL "
KERNELS = ("decode_attn_kv8_kernel", "kv_quantize_kernel")


def _model(cfg, dev):
    import torch
    from cambrian_amd.model.language_model import cambrian_llama as CL
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    return model.requires_grad_(False).eval()


def child(arm: str, new: int, ctxs, batches) -> None:
    sys.path.insert(0, ROOT)
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_kv8: no GPU visible")
    prec, switch = arm.split("-")                       # bf16 | fp8 weights, on | off = e4m3 | bf16 cache
    assert ops.decode_fp8_enabled() == (prec == "fp8") and ops.decode_step_enabled()
    assert ops.decode_kv_fp8_enabled() == (switch == "on")
    dev = torch.device("cuda:0")
    cfg = CL.llama3_8b_config()
    model = _model(cfg, dev)
    calls = {"step": 0, "kv8": 0}
    real_step = ops.decode_step

    def counted(*a, **kw):
        calls["step"] += 1
        calls["kv8"] += kw.get("kv8") is not None
        return real_step(*a, **kw)

    ops.decode_step = counted

    def gen(ids, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for ctx in ctxs:
        for B in batches:
            g = torch.Generator().manual_seed(B)
            ids = torch.randint(0, cfg.vocab_size, (B, ctx), generator=g).to(dev)
            calls["step"] = calls["kv8"] = 0
            torch.cuda.reset_peak_memory_stats()
            _, free = gen(ids, 1 + new)                  # warm-up of every shape; and the peak of one call
            peak = torch.cuda.max_memory_allocated()
            assert free.shape == (B, 1 + new)
            assert calls["step"] == new and calls["kv8"] == (new if switch == "on" else 0), f"{arm}: {calls}"
            base = statistics.median(gen(ids, 1)[0] for _ in range(3))
            win = []
            for _ in range(3):
                ms, out = gen(ids, 1 + new)
                assert torch.equal(out, free)
                win.append((ms - base) / new)
            rec = dict(arm=arm, B=B, ctx=ctx, new=new, prefill_ms=base, peak_gb=peak / 2 ** 30,
                       ms=(statistics.median(win), min(win), max(win)), tokens=free[0, :8].tolist())
            print(TAG + json.dumps(rec), flush=True)
            del ids, free, out
            torch.cuda.empty_cache()


def error_child() -> None:
    """What the e4m3 cache costs against the bf16 cache, measured: the kernel's output on Gaussian K / V, and the logits of
    the first decode step of a tiny model."""
    sys.path.insert(0, ROOT)
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_kv8: no GPU visible")
    dev = torch.device("cuda:0")

    def l2(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm()).item()

    B, nh, nkv, hd, n = 2, 32, 8, 128, 2049             # 2048 cached keys + the new one
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, h * hd, generator=g).to(torch.bfloat16).to(dev) for h in (nh, nkv, nkv))
    K, V = (torch.randn(B, nkv, n, hd, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    cos, sin = ops.rope_table(torch.full((B, 1), n - 1, device=dev), hd, 500000.0)
    valid = torch.ones(B, n, dtype=torch.bool, device=dev)
    want = ops.decode_attention(q, k, v, cos, sin, K.clone(), V.clone(), n - 1, valid)
    kc, vc = (ops.kv_quantize_e4m3(x, ops.KvCacheE4M3.empty(B, nkv, n, hd, dev), n - 1) for x in (K, V))
    got = ops.decode_attention_kv8(q, k, v, cos, sin, kc, vc, n - 1, valid)
    print(ETAG + json.dumps(dict(what="attn", keys=n - 1, geometry=[nh, nkv, hd], rel_l2=l2(got, want),
                                 k_entries=l2(kc.dequantize()[:, :, :n - 1], K[:, :, :n - 1].float()))), flush=True)

    cfg = CL.CambrianConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, rms_norm_eps=1e-5, max_position_embeddings=512, rope_theta=500000.0)
    torch.manual_seed(3)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model.requires_grad_(False).eval()
    ids = torch.randint(1, 512, (3, 9), generator=torch.Generator().manual_seed(3)).to(dev)
    seen = []
    real_step = ops.decode_step

    def keep(*a, **kw):
        r = real_step(*a, **kw)
        seen.append(r.clone())
        return r

    ops.decode_step = keep
    os.environ["CAMBRIAN_AMD_DECODE_STEP"] = "1"
    for flag in ("0", "1"):
        os.environ["CAMBRIAN_AMD_DECODE_KV_FP8"] = flag
        model.generate(ids, max_new_tokens=2)
    assert len(seen) == 2
    print(ETAG + json.dumps(dict(what="logits", rel_l2=l2(seen[1], seen[0]),
                                 max_abs=(seen[1] - seen[0]).abs().max().item(), logit_absmax=seen[0].abs().max().item(),
                                 same_argmax=bool((seen[1].argmax(-1) == seen[0].argmax(-1)).all()))), flush=True)


def kernel_child() -> None:
    """One attention call alone, Llama-3-8B geometry: ``ops.decode_attention`` on a bf16 cache against
    ``ops.decode_attention_kv8`` on the e4m3 cache of the same values; us per call from device events around 50 calls, median of
    3 windows (min - max).  Allocates the caches only, so it reaches 16 rows x 8192 keys, which the ``generate()`` arms leave out."""
    sys.path.insert(0, ROOT)
    import torch
    from cambrian_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_kv8: no GPU visible")
    dev = torch.device("cuda:0")
    nh, nkv, hd = 32, 8, 128
    for B, keys in ((1, 2048), (16, 2048), (1, 8192), (4, 8192), (16, 8192)):
        n = keys + 1
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(B, h * hd, generator=g).to(torch.bfloat16).to(dev) for h in (nh, nkv, nkv))
        K, V = (torch.randn(B, nkv, n, hd, device=dev).to(torch.bfloat16) for _ in range(2))
        cos, sin = ops.rope_table(torch.full((B, 1), keys, device=dev), hd, 500000.0)
        valid = torch.ones(B, n, dtype=torch.bool, device=dev)
        kc, vc = (ops.kv_quantize_e4m3(x, ops.KvCacheE4M3.empty(B, nkv, n, hd, dev), keys) for x in (K, V))
        rec = dict(B=B, keys=keys, geometry=[nh, nkv, hd], splits=ops.decode_attention_plan(B, nkv, keys)[0])
        for name, fn in (("off", lambda: ops.decode_attention(q, k, v, cos, sin, K, V, keys, valid)),
                         ("on", lambda: ops.decode_attention_kv8(q, k, v, cos, sin, kc, vc, keys, valid))):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            win = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                win.append(e0.elapsed_time(e1) / 50 * 1e3)
            rec[name] = (statistics.median(win), min(win), max(win))
        cache_bytes = 2 * B * nkv * keys * hd
        rec["off_tbs"], rec["on_tbs"] = 2 * cache_bytes / rec["off"][0] / 1e6, cache_bytes * (hd + 4) / hd / rec["on"][0] / 1e6
        print(KTAG + json.dumps(rec), flush=True)
        del K, V, kc, vc


def resource_usage() -> list:
    """hipcc's kernel-resource-usage remarks for the kernels of decode_attn_kv8.hip (no GPU needed)"""
    src = os.path.join(ROOT, "cambrian_amd", "csrc", "decode_attn_kv8.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, cwd=os.path.dirname(src))
    if p.returncode != 0:
        raise SystemExit(p.stderr)
    out, cur = [], None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = dict(name=m.group(1)) if any(k in m.group(1) for k in KERNELS) else None
            if cur is not None:
                out.append(cur)
            continue
        m = re.search(r"remark:\s+.*?(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1) if m.group(1).endswith("Spill") else m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def _pretty(name: str) -> str:
    m = re.search(r"decode_attn_kv8_kernelILi(\d+)ELi(\d+)E", name)
    if m:
        return f"`decode_attn_kv8_kernel<hd {m.group(1)}, GP {m.group(2)}>`"
    m = re.search(r"kv_quantize_kernelILi(\d+)E", name)
    return f"`kv_quantize_kernel<{m.group(1)} lanes per row>`" if m else f"`{name}`"


def resource_section(res: list) -> list:
    lines = ["## Kernel resources (`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`)", "",
             "No instantiation spills or uses scratch.  GP is the number of query heads per KV head the instantiation holds "
             "(1, 2, 3-4, 5-8).", "",
             "| kernel | VGPR | AGPR | SGPR | VGPR spill | SGPR spill | scratch B / lane | LDS B / workgroup | waves / SIMD |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {_pretty(r['name'])} | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('VGPRs Spill')} | "
                     f"{r.get('SGPRs Spill')} | {r.get('ScratchSize')} | {r.get('LDS')} | {r.get('Occupancy')} |")
    bad = [r["name"] for r in res if r.get("VGPRs Spill") or r.get("SGPRs Spill") or r.get("ScratchSize")]
    if bad:
        raise SystemExit(f"bench_decode_kv8: spills or scratch in {bad}")
    return lines


HEAD = ["# Decode steps on an e4m3 K / V cache (`cmb_decode_attn_kv8`, `CAMBRIAN_AMD_DECODE_KV_FP8=1`)", "",
        "Written by `tools/bench_decode_kv8.py`; the method is in its docstring.  The switch is off by default whatever this "
        "table says: the e4m3 cache changes numerics, and nothing here is a measurement of task quality on a real checkpoint.", ""]


def kernel_section(kern: list) -> list:
    if not kern:
        return ["## The attention call alone: not measured", ""]
    lines = ["## The attention call alone (us per call, both launches of a split call)", "",
             "`ops.decode_attention` on a bf16 cache (`off`) against `ops.decode_attention_kv8` on the e4m3 cache of the same "
             f"Gaussian values (`on`), nh / nkv / hd = {' / '.join(str(x) for x in kern[0]['geometry'])}, the library's own split; device "
             "events around 50 calls, median of 3 windows (min - max), one process.  TB/s counts the cache bytes the call has to "
             "read (bf16: 2 hd per row, e4m3: hd + 4).  **faster** as above.", "",
             "| B | cached keys | splits | on us | off us | off / on | verdict | on TB/s | off TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in kern:
        on, off = r["on"], r["off"]
        lines.append(f"| {r['B']} | {r['keys']} | {r['splits']} | {on[0]:.1f} ({on[1]:.1f} - {on[2]:.1f}) | {off[0]:.1f} ({off[1]:.1f} - "
                     f"{off[2]:.1f}) | {off[0] / on[0]:.2f} | {'**faster**' if on[0] < off[1] else '**not faster**'} | "
                     f"{r['on_tbs']:.2f} | {r['off_tbs']:.2f} |")
    return lines + [""]


def note(recs: dict, errs: list, res: list, cmd: str, kern: list = ()) -> list:
    lines = list(HEAD)

    def f(t3):
        return f"{t3[0]:.3f} ({t3[1]:.3f} - {t3[2]:.3f})"

    if not recs:
        lines += ["## Speed and memory: not measured", "",
                  "No GPU run of the tool could be had for this note; nothing is claimed about speed or memory.", ""]
    else:
        new = next(iter(recs.values()))["new"]
        lines += ["## ms per decoded token and peak memory, Llama-3-8B at full depth", "",
                  f"`{cmd}`: 32 layers, vocabulary 128256, random frozen weights, text-only prompts, greedy without an eos id, the "
                  f"one-call step on in both arms; ms per decoded token = (wall clock of `generate()` for 1 + {new} tokens - that "
                  f"for 1 token, device synchronised) / {new}.  Median of 3 windows (min - max), each arm in its own process, arms "
                  "alternating.  `on` = the e4m3 cache, `off` = the bf16 cache on the same tree.  **faster** = the on arm's "
                  "median is below the off arm's fastest window; anything else is **not faster**.  Peak = "
                  "`torch.cuda.max_memory_allocated` over one call, weights included.", "",
                  "| weights | context | B | on ms / token | off ms / token | off / on | verdict | on peak GiB | off peak GiB | "
                  "on prefill ms | off prefill ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        keys = sorted({(p, c, b) for (p, s, c, b) in recs}, key=lambda k: (k[0] != "bf16", k[1], k[2]))
        missing = []
        for prec, ctx, B in keys:
            on, off = recs.get((prec, "on", ctx, B)), recs.get((prec, "off", ctx, B))
            if on is None or off is None:
                missing.append(f"{prec} weights, context {ctx}, B {B}")
                continue
            lines.append(f"| {prec} | {ctx} | {B} | {f(on['ms'])} | {f(off['ms'])} | {off['ms'][0] / on['ms'][0]:.2f} | "
                         f"{'**faster**' if on['ms'][0] < off['ms'][1] else '**not faster**'} | {on['peak_gb']:.2f} | "
                         f"{off['peak_gb']:.2f} | {on['prefill_ms']:.0f} | {off['prefill_ms']:.0f} |")
        lines.append("")
        want = {(p, c, b) for p in ("bf16", "fp8") for c in (2048, 8192) for b in (1, 4, 16)}
        rest = sorted(want - set(keys))
        if rest or missing:
            lines += ["Not measured in this run: " + "; ".join(
                [f"{p} weights, context {c}, B {b}" for p, c, b in rest] + missing) + ".", ""]
    if errs:
        lines += ["## What the cache costs in accuracy (measured, not asserted by any test)", ""]
        for e in errs:
            if e["what"] == "attn":
                lines.append(f"- Attention output of one decode step against the bf16 cache, Gaussian K / V (bf16 N(0, 1)), "
                             f"{e['keys']} cached keys, geometry nh / nkv / hd = {e['geometry'][0]} / {e['geometry'][1]} / "
                             f"{e['geometry'][2]}, 2 rows: relative L2 error **{e['rel_l2']:.4f}** (the K entries themselves: "
                             f"{e['k_entries']:.4f}).")
            else:
                lines.append(f"- fp32 logits of the first decode step of the tiny model of tests/test_decode_kv8_gpu.py (2 layers, "
                             f"H 256, 4 heads / 2 KV heads of 64, vocabulary 512; 3 prompts of 9 tokens) against the bf16 cache: "
                             f"relative L2 error **{e['rel_l2']:.4f}**, largest absolute difference {e['max_abs']:.4f} at a largest "
                             f"|logit| of {e['logit_absmax']:.3f}; the argmax of every row is "
                             f"{'the same' if e['same_argmax'] else 'NOT the same'}.")
        lines += ["", "Gaussian data and a random tiny model say nothing about a trained checkpoint's outlier channels; task "
                  "quality is unmeasured.", ""]
    else:
        lines += ["## Accuracy: not measured", ""]
    lines += kernel_section(list(kern))
    lines += resource_section(res)
    return lines


def parse(text: str):
    recs, errs, kern = {}, [], []
    for ln in text.splitlines():
        if ln.startswith(TAG):
            r = json.loads(ln[len(TAG):])
            prec, switch = r["arm"].split("-")
            recs[prec, switch, r["ctx"], r["B"]] = r
        elif ln.startswith(ETAG):
            errs.append(json.loads(ln[len(ETAG):]))
        elif ln.startswith(KTAG):
            kern.append(json.loads(ln[len(KTAG):]))
    return recs, errs, kern


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_kv8.md"))
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--ctx", default="2048,8192")
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--weights", default="bf16,fp8")
    ap.add_argument("--log", help="also keep the children's output here")
    ap.add_argument("--from-log")
    ap.add_argument("--not-measured", action="store_true")
    ap.add_argument("--skip-errors", action="store_true", help="do not run the accuracy and kernel-alone children (a second run into one log)")
    ap.add_argument("--child")
    ap.add_argument("--error-child", action="store_true")
    ap.add_argument("--kernel-child", action="store_true")
    a = ap.parse_args()
    ctxs, batches = [int(x) for x in a.ctx.split(",")], [int(x) for x in a.batches.split(",")]
    if a.child:
        return child(a.child, a.new, ctxs, batches)
    if a.error_child:
        return error_child()
    if a.kernel_child:
        return kernel_child()
    cmd = f"python tools/bench_decode_kv8.py --new {a.new} --ctx {a.ctx} --batches {a.batches} --weights {a.weights}"
    if a.not_measured:
        text = ""
    elif a.from_log:
        text = open(a.from_log).read()
        cmds = re.findall(r"^BENCH_DECODE_KV8_CMD (.*)$", text, re.M)       # a log may hold several runs, one after the other
        cmd = "`, then `".join(cmds) if cmds else cmd
    else:
        text = "BENCH_DECODE_KV8_CMD " + cmd + "\n"
        base = {k: v for k, v in os.environ.items() if not k.startswith("CAMBRIAN_AMD_DECODE_")}
        base["CAMBRIAN_AMD_DECODE_STEP"] = "1"
        jobs = [] if a.skip_errors else [(["--error-child"], {}), (["--kernel-child"], {})]
        for prec in a.weights.split(","):
            for switch in ("on", "off"):                 # the arms alternate
                jobs.append((["--child", f"{prec}-{switch}"], {"CAMBRIAN_AMD_DECODE_FP8": "1" if prec == "fp8" else "0",
                                                              "CAMBRIAN_AMD_DECODE_KV_FP8": "1" if switch == "on" else "0"}))
        for extra, env in jobs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--new", str(a.new), "--ctx", a.ctx, "--batches",
                                a.batches] + extra, env={**base, **env}, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            text += p.stdout
            if a.log:
                with open(a.log, "w") as fh:
                    fh.write(text)
            if p.returncode != 0:                        # a child that failed ends the run: nothing more is started
                raise SystemExit(f"bench_decode_kv8: {extra} exited with {p.returncode}")
    recs, errs, kern = parse(text)
    with open(a.out, "w") as fh:
        fh.write("\n".join(note(recs, errs, resource_usage(), cmd, kern)) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
