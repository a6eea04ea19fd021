"""Decode steps at 32 and 64 rows: the wide weight-streaming linear (``cmb_decode_linear_wide``, five launches per layer, behind
``CAMBRIAN_AMD_DECODE_LINEAR_WIDE=1``) against the stock sequence that runs there with the switch off — two norm launches, four
BLAS calls, a SwiGLU pass and two adds, which is what the code before the kernel does at these rows: the yardstick.

    python tools/bench_decode_linear_wide.py [--out profiles/decode_linear_wide.md] [--iters 30] [--quick] [--no-generate]
    python tools/bench_decode_linear_wide.py --from-log FILE [--out ...]      # write the note again from a run's output
    python tools/bench_decode_linear_wide.py --dump-resources FILE            # no GPU: hipcc's register / LDS / scratch report

Method of tools/bench_decode_linear.py: Llama-3-8B, Yi-34B (Llama blocks) and Phi-3-mini (Phi-3 block) in bf16, context 2048,
batch 32 and 64; each arm runs in a fresh child process (one per geometry and arm, the arms alternating), every child under a
time limit, and a child that fails ends the run.  HIP events after a warm-up of every timed shape, three windows per number
(median, min - max).  Rows:
  * the five linears alone — qkv, o, gate_up, down and lm_head: ``ops.decode_linear_wide`` in the on arm, in the off arm the
    sequence it replaces (norm + GEMM, GEMM + add, norm + GEMM + SwiGLU, GEMM with the skip connection as C, norm + GEMM +
    cast).  The on arm also times ``ops.decode_linear`` on 16 rows of the same weights: the narrow kernel's weight stream;
  * one ``layer.decode`` call with random frozen weights;
  * ms per decoded token through ``generate()``: Llama-3-8B at full depth, a text-only prompt of 2048 tokens, greedy,
    (wall clock for 1 + n tokens - that for 1 token) / n.
Every call takes the next of a ring of weight sets of at least 768 MB (three times the last-level cache).  MB = weight bytes
of the shapes; GB/s = those bytes / time.  A row is **faster** only when the on arm's median is below the off arm's fastest
window; anything else is **NOT faster**.  A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import json
import os
import re
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMS = {"llama3-8b": dict(lm="llama", hidden_size=4096, intermediate_size=14336, num_attention_heads=32, num_key_value_heads=8,
                           vocab_size=128256),
         "yi-34b": dict(lm="llama", hidden_size=7168, intermediate_size=20480, num_attention_heads=56, num_key_value_heads=8,
                        vocab_size=64000),
         "phi3-mini": dict(lm="phi3", hidden_size=3072, intermediate_size=8192, num_attention_heads=32, num_key_value_heads=32,
                           vocab_size=32064)}
BATCHES = [32, 64]
CTX = 2048
HBM_TBPS = 6.3
RING_BYTES = 768 << 20
LINEARS = ("qkv", "o", "gate_up", "down", "lm_head")
TAG = "BENCH_DECODE_LINEAR_WIDE "
CHILD_TIMEOUT = 420


def linear_shapes(g: dict) -> dict:
    """name -> (N, K) of the five (packed) weights"""
    H, inter, nh, nkv = g["hidden_size"], g["intermediate_size"], g["num_attention_heads"], g["num_key_value_heads"]
    hd = H // nh
    return {"qkv": ((nh + 2 * nkv) * hd, H), "o": (H, nh * hd), "gate_up": (2 * inter, H), "down": (H, inter),
            "lm_head": (g["vocab_size"], H)}


def _timed(torch, fn, n):
    """median / min / max of 3 windows of n calls, microseconds per call"""
    res = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        b.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / n)
    return statistics.median(res), min(res), max(res)


def child(geom: str, arm: str, iters: int, warmup: int, quick: bool) -> None:
    import torch
    import torch.nn.functional as F
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL, cambrian_phi3 as CP
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_linear_wide: no GPU visible")
    on = arm == "on"
    assert ops.decode_linear_wide_enabled() == on and ops.decode_attention_enabled()
    assert not ops.decode_fp8_enabled() and not ops.decode_fp4_enabled()
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    g = dict(GEOMS[geom])
    lm = g.pop("lm")
    mod = CP if lm == "phi3" else CL
    shapes = linear_shapes(g)
    g.pop("vocab_size")
    cfg = mod.CambrianConfig(vocab_size=64, num_hidden_layers=1, rms_norm_eps=1e-5, rope_theta=500000.0,
                             max_position_embeddings=16384, **g)
    torch.manual_seed(0)
    wb = {k: n * kk * 2 for k, (n, kk) in shapes.items()}
    layer_bytes = sum(wb[k] for k in LINEARS[:4])
    ring = max(4, -(-RING_BYTES // layer_bytes))
    cls = CP.Phi3DecoderLayer if lm == "phi3" else CL.LlamaDecoderLayer
    layers = [cls(cfg, dev, dt).requires_grad_(False) for _ in range(ring)]
    att = layers[0].self_attn
    nkv, hd = att.nkv, att.hd
    H = g["hidden_size"]
    eps = 1e-5
    rings = {k: max(4, -(-RING_BYTES // wb[k])) for k in LINEARS}
    weights = {k: [torch.randn(shapes[k], device=dev, dtype=dt) * shapes[k][1] ** -0.5 for _ in range(rings[k])] for k in LINEARS}
    nw = torch.ones(H, device=dev, dtype=dt)
    calls = {"wide": 0}
    real = ops.decode_linear_wide

    def counted(*a, **kw):
        calls["wide"] += 1
        return real(*a, **kw)

    ops.decode_linear_wide = counted

    for B in (BATCHES[:1] if quick else BATCHES):
        t = CTX
        kc = torch.randn(B, nkv, CTX + 8, hd, device=dev, dtype=dt)
        vc = torch.randn(B, nkv, CTX + 8, hd, device=dev, dtype=dt)
        mask = torch.ones(B, CTX + 8, dtype=torch.bool, device=dev)
        x = torch.randn(B, 1, H, device=dev, dtype=dt)
        x2 = x.reshape(B, H)
        xs = {k: torch.randn(B, shapes[k][1], device=dev, dtype=dt) for k in LINEARS}
        cos, sin = ops.rope_table(torch.full((B, 1), CTX, device=dev), hd, 500000.0)

        def layer_call(i):
            layers[i % ring].decode(x, cos, sin, kc, vc, t, mask)

        def lin_call(name, narrow=False):
            ws, n = weights[name], rings[name]
            xin, res = (xs[name][:16], x2[:16]) if narrow else (xs[name], x2)
            if on:
                kw = {"qkv": dict(norm_weight=nw, eps=eps), "o": dict(residual=res),
                      "gate_up": dict(norm_weight=nw, eps=eps, act="swiglu"), "down": dict(residual=res),
                      "lm_head": dict(norm_weight=nw, eps=eps, out_dtype=torch.float32)}[name]
                fn = ops.decode_linear if narrow else real
                return lambda i: fn(xin, ws[i % n], **kw)
            if name == "qkv":
                return lambda i: F.linear(ops.rmsnorm(xin, nw, eps), ws[i % n])
            if name == "o":
                return lambda i: res + F.linear(xin, ws[i % n])
            if name == "gate_up":
                return lambda i: ops.swiglu_packed(F.linear(ops.rmsnorm(xin, nw, eps), ws[i % n]))
            if name == "lm_head":
                return lambda i: F.linear(ops.rmsnorm(xin, nw, eps), ws[i % n]).float()
            return lambda i: torch.addmm(res, xin, ws[i % n].t())

        fns = {k: lin_call(k) for k in LINEARS}
        rec = dict(geom=geom, arm=arm, B=B, ctx=CTX, ring=ring, rings=rings, iters=iters, bytes=wb, layer_bytes=layer_bytes)
        with torch.no_grad():
            calls["wide"] = 0
            for i in range(max(warmup, ring)):
                layer_call(i)
            assert calls["wide"] == (4 * max(warmup, ring) if on else 0), f"{arm}: {calls['wide']} wide calls in the layers"
            for k in LINEARS:
                for i in range(max(warmup, 4)):
                    fns[k](i)
            torch.cuda.synchronize()
            rec["layer_us"] = _timed(torch, layer_call, iters)
            for k in LINEARS:
                rec[k + "_us"] = _timed(torch, fns[k], iters)
            if on and B == BATCHES[0]:                   # the narrow kernel's stream on 16 rows of the same weights
                for k in LINEARS:
                    fn = lin_call(k, narrow=True)
                    for i in range(max(warmup, 4)):
                        fn(i)
                    rec[k + "_narrow16_us"] = _timed(torch, fn, iters)
        print(TAG + json.dumps(rec), flush=True)


def child_generate(arm: str, new: int, quick: bool) -> None:
    import torch
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_linear_wide: no GPU visible")
    on = arm == "on"
    assert ops.decode_linear_wide_enabled() == on and not ops.decode_fp8_enabled() and not ops.decode_fp4_enabled()
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = CL.llama3_8b_config()
    torch.manual_seed(0)
    model = CL.CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=dt)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
    model.requires_grad_(False).eval()
    calls = {"wide": 0}
    real = ops.decode_linear_wide

    def counted(*a, **kw):
        calls["wide"] += 1
        return real(*a, **kw)

    ops.decode_linear_wide = counted

    def gen(ids, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B in (BATCHES[:1] if quick else BATCHES):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, cfg.vocab_size, (B, CTX), generator=g).to(dev)
        calls["wide"] = 0
        _, free = gen(ids, 1 + new)                       # warm-up of every shape
        assert free.shape == (B, 1 + new)
        want = new * (4 * cfg.num_hidden_layers + 1) if on else 0
        assert calls["wide"] == want, f"{arm}: {calls['wide']} wide calls, expected {want}"
        base = statistics.median(gen(ids, 1)[0] for _ in range(3))
        win = [(gen(ids, 1 + new)[0] - base) / new for _ in range(3)]
        rec = dict(geom="llama3-8b", arm=arm, B=B, ctx=CTX, new=new, prefill_ms=base,
                   token_ms=(statistics.median(win), min(win), max(win)))
        print(TAG + json.dumps(rec), flush=True)
        del ids


def resource_usage() -> list:
    """hipcc's kernel-resource-usage remarks for decode_linear_wide.hip (no GPU needed): one dict per instantiation"""
    src = os.path.join(ROOT, "cambrian_amd", "csrc", "decode_linear_wide.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, cwd=os.path.dirname(src))
    if p.returncode != 0:
        raise SystemExit(p.stderr)
    out, cur = [], None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = dict(name=m.group(1)) if "decode_linear_wide_kernel" in m.group(1) else None
            if cur is not None:
                out.append(cur)
            continue
        m = re.search(r"remark:\s+.*?(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1) if m.group(1).endswith("Spill") else m.group(1).split(" ")[0]] = int(m.group(2))
    for r in out:
        m = re.search(r"ILi(\d)ELi(\d)ELb([01])E", r["name"])
        r["pairs"], r["blocks"], r["norm"] = int(m.group(1)), int(m.group(2)), bool(int(m.group(3)))
    bad = [r["name"] for r in out if r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"]]
    if bad or not out:
        raise SystemExit(f"bench_decode_linear_wide: spills or scratch in {bad}")
    return out


def write_note(a, recs: dict, gens: dict, res: list) -> None:
    def f(t3, d=1):
        return f"{t3[0]:.{d}f} ({t3[1]:.{d}f} - {t3[2]:.{d}f})"

    def verdict(o, z):
        return "faster" if o[0] < z[1] else "NOT faster"

    lines = ["# Decode steps at 32 and 64 rows: `cmb_decode_linear_wide` (five launches per layer) against the stock sequence", "",
             f"Command: `python tools/bench_decode_linear_wide.py --iters {a.iters} --warmup {a.warmup}`"
             + (" `--quick`" if a.quick else ""),
             f"on {a.host}, bf16, context {CTX}, random frozen weights; HIP events, median of 3 windows of {a.iters} "
             "calls (min - max in brackets), each arm in its own process, arms alternating.  `on` = "
             "`CAMBRIAN_AMD_DECODE_LINEAR_WIDE=1`, `off` = `0`: the stock sequence these rows run without the kernel, the yardstick.  "
             "Every call takes the next of a ring of weight sets of at least 768 MB.  MB = weight bytes of the shapes; GB/s = MB / "
             f"on-arm time, the share is of the ~{HBM_TBPS} TB/s an MI355X achieves from HBM.  A row is **faster** only when the on "
             "arm's median is below the off arm's fastest window; anything else is **NOT faster**.  The default stays off.", "",
             "## One `layer.decode` call", "",
             "| model | B | layer MB | on us | off us | off / on | on GB/s | of HBM | verdict |", "|---|---|---|---|---|---|---|---|---|"]
    tally = {"faster": [], "NOT faster": []}
    for geom in GEOMS:
        for B in BATCHES:
            o, z = recs.get((geom, B, "on")), recs.get((geom, B, "off"))
            if o is None or z is None:
                continue
            mb = o["layer_bytes"]
            gbs = mb / (o["layer_us"][0] * 1e-6) / 1e9
            v = verdict(o["layer_us"], z["layer_us"])
            tally[v].append(f"layer {geom} B {B}")
            lines.append(f"| {geom} | {B} | {mb / 1e6:.1f} | {f(o['layer_us'])} | {f(z['layer_us'])} | "
                         f"{z['layer_us'][0] / o['layer_us'][0]:.2f} | {gbs:.0f} | {gbs / (HBM_TBPS * 1e3) * 100:.0f} % | {v} |")
    lines += ["", "## The five linears alone (on: one `ops.decode_linear_wide` call; off: the sequence it replaces)", "",
              "`narrow 16` is `ops.decode_linear` on 16 rows of the same ring of weights in the same process: the narrow kernel's "
              "weight stream, for the GB/s columns to be read against.", "",
              "| model | B | linear | N x K | MB | on us | off us | off / on | on GB/s | of HBM | narrow 16 us | narrow 16 GB/s | verdict |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for geom in GEOMS:
        shapes = linear_shapes({k: v for k, v in GEOMS[geom].items() if k != "lm"})
        for B in BATCHES:
            o, z = recs.get((geom, B, "on")), recs.get((geom, B, "off"))
            if o is None or z is None:
                continue
            nar = recs.get((geom, BATCHES[0], "on"), {})
            for k in LINEARS:
                mb = o["bytes"][k]
                gbs = mb / (o[k + "_us"][0] * 1e-6) / 1e9
                n16 = nar.get(k + "_narrow16_us")
                v = verdict(o[k + "_us"], z[k + "_us"])
                tally[v].append(f"{k} {geom} B {B}")
                lines.append(f"| {geom} | {B} | {k} | {shapes[k][0]} x {shapes[k][1]} | {mb / 1e6:.1f} | {f(o[k + '_us'])} | "
                             f"{f(z[k + '_us'])} | {z[k + '_us'][0] / o[k + '_us'][0]:.2f} | {gbs:.0f} | "
                             f"{gbs / (HBM_TBPS * 1e3) * 100:.0f} % | " + (f"{f(n16)} | {mb / (n16[0] * 1e-6) / 1e9:.0f}" if n16 else "- | -")
                             + f" | {v} |")
    lines += ["", "## ms per decoded token through `generate()`, Llama-3-8B at full depth", ""]
    if gens:
        new = next(iter(gens.values()))["new"]
        lines += [f"32 layers, vocabulary 128256, a text-only prompt of {CTX} tokens, greedy on the per-launch loop; ms per decoded token = "
                  f"(wall clock of `generate()` for 1 + {new} tokens - that for 1 token, device synchronised) / {new}.  Median of 3 "
                  "windows (min - max), each arm in its own process.", "",
                  "| B | on ms / token | off ms / token | off / on | verdict |", "|---|---|---|---|---|"]
        for B in BATCHES:
            o, z = gens.get((B, "on")), gens.get((B, "off"))
            if o is None or z is None:
                continue
            v = verdict(o["token_ms"], z["token_ms"])
            tally[v].append(f"generate llama3-8b B {B}")
            lines.append(f"| {B} | {f(o['token_ms'], 2)} | {f(z['token_ms'], 2)} | {z['token_ms'][0] / o['token_ms'][0]:.2f} | {v} |")
    else:
        lines.append("Not measured in this run.")
    lines += ["", "## Verdict", "",
              "Faster (on median below off minimum): " + ("; ".join(tally["faster"]) if tally["faster"] else "nowhere") + ".", "",
              "NOT faster: " + ("; ".join(tally["NOT faster"]) if tally["NOT faster"] else "nowhere") + ".", "",
              "The switch stays off by default (`config.decode_linear_wide` / `CAMBRIAN_AMD_DECODE_LINEAR_WIDE`).", "",
              "## Kernel resources (hipcc, gfx950)", "",
              "No instantiation spills or uses scratch.  Slab rows = 16 x pairs; row blocks = ceil(M / 16).", "",
              "| slab rows | row blocks | norm prologue | VGPRs | AGPRs | SGPRs | VGPR spills | SGPR spills | LDS bytes | scratch bytes / lane | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in sorted(res, key=lambda r: (r["pairs"], r["blocks"], r["norm"])):
        lines.append(f"| {16 * r['pairs']} | {r['blocks']} | {'yes' if r['norm'] else 'no'} | {r['VGPRs']} | {r['AGPRs']} | {r['TotalSGPRs']} | "
                     f"{r['VGPRs Spill']} | {r['SGPRs Spill']} | {r['LDS']} | {r['ScratchSize']} | {r['Occupancy']} |")
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print(f"bench_decode_linear_wide: wrote {a.out}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_linear_wide.md"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--new", type=int, default=16, help="decoded tokens per generate() window")
    ap.add_argument("--quick", action="store_true", help="first batch only (rehearsal)")
    ap.add_argument("--no-generate", action="store_true", help="skip the generate() rows")
    ap.add_argument("--from-log", help="a run's output; write the note again without running anything")
    ap.add_argument("--host", default=f"`{socket.gethostname()}` (MI355X)", help="how the note names the machine")
    ap.add_argument("--resources", help="JSON written by --dump-resources; without it hipcc is run now")
    ap.add_argument("--dump-resources", metavar="FILE")
    ap.add_argument("--child", nargs=2, metavar=("GEOM", "ARM"))
    a = ap.parse_args()
    if a.dump_resources:
        with open(a.dump_resources, "w") as fh:
            json.dump(resource_usage(), fh, indent=1)
        return
    if a.iters < 20:
        ap.error("--iters: at least 20")
    if a.child:
        if a.child[0] == "generate":
            child_generate(a.child[1], a.new, a.quick)
        else:
            child(a.child[0], a.child[1], a.iters, a.warmup, a.quick)
        return
    recs, gens = {}, {}

    def take(ln):
        if ln.startswith(TAG):
            r = json.loads(ln[len(TAG):])
            if "token_ms" in r:
                gens[r["B"], r["arm"]] = r
            else:
                recs[r["geom"], r["B"], r["arm"]] = r
            return True
        return False

    if a.from_log:
        with open(a.from_log) as fh:
            for ln in fh:
                take(ln)
    else:
        for geom in list(GEOMS) + ([] if a.no_generate else ["generate"]):
            for arm in ("on", "off"):
                env = dict(os.environ, CAMBRIAN_AMD_DECODE_LINEAR_WIDE="1" if arm == "on" else "0", CAMBRIAN_AMD_DECODE_FP8="0",
                           CAMBRIAN_AMD_DECODE_FP4="0")
                for name in ("CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_STEP"):
                    env.pop(name, None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", geom, arm, "--iters", str(a.iters),
                       "--warmup", str(a.warmup), "--new", str(a.new)] + (["--quick"] if a.quick else [])
                p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
                if p.returncode != 0:               # a child that failed ends the run: nothing else is started on the GPU
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit(f"bench_decode_linear_wide: child {geom}/{arm} exited with {p.returncode}")
                for ln in p.stdout.splitlines():
                    if take(ln):
                        print(ln, flush=True)
    if a.resources:
        with open(a.resources) as fh:
            res = json.load(fh)
    else:
        res = resource_usage()
    write_note(a, recs, gens, res)


if __name__ == "__main__":
    main()
