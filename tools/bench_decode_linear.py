"""Decode step of one decoder layer: the weight-streaming linear kernel (``cmb_decode_linear``, five launches per layer)
against the stock sequence (``CAMBRIAN_AMD_DECODE_LINEAR=0``: two norm launches, four BLAS calls, a SwiGLU pass and two
adds), same box, same run.  The off arm is the yardstick; the table this writes decides the default of
``ops.DECODE_LINEAR_DEFAULT_MAX_ROWS``.

    python tools/bench_decode_linear.py [--out profiles/decode_linear.md] [--iters 50] [--quick] [--resources FILE]
    python tools/bench_decode_linear.py --dump-resources FILE       # no GPU: hipcc's register / LDS / scratch report
    python tools/bench_decode_linear.py --fp8 [--out profiles/decode_fp8.md] [--resources FILE]
    python tools/bench_decode_linear.py --fp8 --dump-resources FILE
    python tools/bench_decode_linear.py --fp4 [--out profiles/decode_fp4.md] [--resources FILE] [--step-log FILE]
    python tools/bench_decode_linear.py --fp4 --dump-resources FILE

``--fp8`` measures the e4m3 weight stream (``cmb_decode_linear_fp8``, ``layer.decode(..., fp8=True)``) against the bf16
``decode_linear`` arm — today's default path, the yardstick — by the same method; the ring is at least 768 MB of the 1-byte
weights, MB and GB/s count one byte per weight, and a row is faster when the fp8 median is below the bf16 arm's minimum
window.  A weight the row quantiser does not reach (K > ``ops.DECODE_FP8_MAX_K``: Yi-34B's down_proj) is timed alone on
random finite e4m3 bytes — time does not depend on the values — and the layer that holds it refuses the mode, quantises nothing and
runs on bf16, as it does in ``generate()``; the layer table reads that off the layers and says so.

``--fp4`` measures the MXFP4 weight stream (``cmb_decode_linear_fp4``, ``layer.decode(..., fp4=True)``) against BOTH the bf16
arm and the e4m3 arm, three arms alternating per geometry, by the same method; every ring is sized by the MXFP4 bytes (17 / 32
byte per weight: nibbles + scales), which is what MB and GB/s count for that arm.  No weight is out of the block quantiser's
reach, so the Yi-34B layers take the mode.  ``--step-log FILE``: the output of ``tools/bench_decode_step.py --fp4``, whose
ms-per-token rows become the note's last table.

For Llama-3-8B, Yi-34B (Llama blocks) and Phi-3-mini (Phi-3 block) in bf16, context 2048, batch 1 / 4 / 16, each arm runs in
a fresh child process (one per geometry and arm, the arms alternating) and times with HIP events after a warm-up of every
timed shape, three windows per number (median, min - max):
  * ``layer``  one ``layer.decode`` call with random frozen weights;
  * the four linears alone: ``ops.decode_linear`` in the on arm, in the off arm the sequence it replaces —
    ``qkv`` norm + GEMM, ``o`` GEMM + add, ``gate_up`` norm + GEMM + SwiGLU, ``down`` GEMM with the skip connection as C.
Every call uses the next of a ring of weight sets (at least four, and at least 768 MB in total — three times the 256 MB
last-level cache), as a model's layers are distinct tensors, so no weight byte is served from the cache the previous call
left.  ``MB`` is the weight bytes of the shapes; GB/s = those bytes / time, shown against the ~6.3 TB/s an MI355X achieves
from HBM.  A regime (geometry x batch) counts as faster when the on arm's median layer time is below the off arm's MINIMUM
window.  A run without a GPU fails; nothing is estimated."""
from __future__ import annotations

import argparse
import json
import os
import re
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMS = {"llama3-8b": dict(lm="llama", hidden_size=4096, intermediate_size=14336, num_attention_heads=32, num_key_value_heads=8),
         "yi-34b": dict(lm="llama", hidden_size=7168, intermediate_size=20480, num_attention_heads=56, num_key_value_heads=8),
         "phi3-mini": dict(lm="phi3", hidden_size=3072, intermediate_size=8192, num_attention_heads=32, num_key_value_heads=32)}
BATCHES = [1, 4, 16]
CTX = 2048
HBM_TBPS = 6.3
RING_BYTES = 768 << 20
LINEARS = ("qkv", "o", "gate_up", "down")


def linear_shapes(g: dict) -> dict:
    """name -> (N, K) of the four (packed) weights"""
    H, inter, nh, nkv = g["hidden_size"], g["intermediate_size"], g["num_attention_heads"], g["num_key_value_heads"]
    hd = H // nh
    return {"qkv": ((nh + 2 * nkv) * hd, H), "o": (H, nh * hd), "gate_up": (2 * inter, H), "down": (H, inter)}


def weight_bytes(g: dict, elem: int = 2) -> dict:
    """``elem``: bytes per weight, or "fp4" = 17 / 32 (a nibble and 1 / 32 of a scale byte)"""
    if elem == "fp4":
        return {k: n * kk * 17 // 32 for k, (n, kk) in linear_shapes(g).items()}
    return {k: n * kk * elem for k, (n, kk) in linear_shapes(g).items()}


def child(geom: str, arm: str, iters: int, warmup: int, quick: bool, ring_fp8: bool = False, ring_fp4: bool = False) -> None:
    import torch
    import torch.nn.functional as F
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL, cambrian_phi3 as CP
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_linear: no GPU visible")
    fp8, fp4 = arm == "fp8", arm == "fp4"
    on = arm == "on" or fp8 or fp4
    assert ops.decode_linear_enabled(1) == on and ops.decode_linear_enabled(16) == on and ops.decode_attention_enabled()
    assert ops.decode_fp8_enabled() == fp8 and ops.decode_fp4_enabled() == fp4
    low = {"fp4": True} if fp4 else {}
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    g = dict(GEOMS[geom])
    lm = g.pop("lm")
    mod = CP if lm == "phi3" else CL
    cfg = mod.CambrianConfig(vocab_size=64, num_hidden_layers=1, rms_norm_eps=1e-5, rope_theta=500000.0,
                             max_position_embeddings=16384, **g)
    torch.manual_seed(0)
    wb = weight_bytes(g, "fp4" if fp4 else (1 if fp8 else 2))        # the bytes a call streams
    # an fp8 run sizes BOTH arms' rings by the 1-byte weights, an fp4 run all three by the MXFP4 bytes
    ring_wb = weight_bytes(g, "fp4") if ring_fp4 else (weight_bytes(g, 1) if ring_fp8 else wb)
    ring = max(4, -(-RING_BYTES // sum(ring_wb.values())))
    cls = CP.Phi3DecoderLayer if lm == "phi3" else CL.LlamaDecoderLayer
    layers = [cls(cfg, dev, dt).requires_grad_(False) for _ in range(ring)]
    att = layers[0].self_attn
    nh, nkv, hd = att.nh, att.nkv, att.hd
    H = g["hidden_size"]
    eps = 1e-5
    shapes = linear_shapes(g)
    rings = {k: max(4, -(-RING_BYTES // ring_wb[k])) for k in LINEARS}

    def weight(k):
        w = torch.randn(shapes[k], device=dev, dtype=dt) * shapes[k][1] ** -0.5
        if fp4:
            return ops.decode_fp4_weight(w)
        if not fp8:
            return w
        if ops.decode_linear_fp8_weight_supported(1, w, "swiglu" if k == "gate_up" else None):
            return ops.decode_fp8_weight(w)
        q = torch.randint(0, 256, shapes[k], device=dev, dtype=torch.uint8)       # beyond the quantiser's reach: random bytes,
        q[(q & 0x7F) == 0x7F] = 0                                                 # none of them the two NaN codes
        return q, torch.full((shapes[k][0],), 2.0 ** -8 * shapes[k][1] ** -0.5, device=dev)

    weights = {k: [weight(k) for _ in range(rings[k])] for k in LINEARS}
    nw = torch.ones(H, device=dev, dtype=dt)

    def timed(fn, n):
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
            layers[i % ring].decode(x, cos, sin, kc, vc, t, mask, fp8=fp8, **low)

        def lin_call(name):
            ws, n, xin = weights[name], rings[name], xs[name]
            if on:
                kw = {"qkv": dict(norm_weight=nw, eps=eps), "o": dict(residual=x2),
                      "gate_up": dict(norm_weight=nw, eps=eps, act="swiglu"), "down": dict(residual=x2)}[name]
                if fp4:
                    return lambda i: ops.decode_linear_fp4(xin, *ws[i % n], **kw)
                if fp8:
                    return lambda i: ops.decode_linear_fp8(xin, *ws[i % n], **kw)
                return lambda i: ops.decode_linear(xin, ws[i % n], **kw)
            if name == "qkv":
                return lambda i: F.linear(ops.rmsnorm(xin, nw, eps), ws[i % n])
            if name == "o":
                return lambda i: x2 + F.linear(xin, ws[i % n])
            if name == "gate_up":
                return lambda i: ops.swiglu_packed(F.linear(ops.rmsnorm(xin, nw, eps), ws[i % n]))
            return lambda i: torch.addmm(x2, xin, ws[i % n].t())

        calls = {k: lin_call(k) for k in LINEARS}
        rec = dict(geom=geom, arm=arm, B=B, ctx=CTX, ring=ring, rings=rings, iters=iters, bytes=wb)
        with torch.no_grad():
            for i in range(max(warmup, ring)):
                layer_call(i)
            for k in LINEARS:
                for i in range(max(warmup, 4)):
                    calls[k](i)
            torch.cuda.synchronize()
            # whether the layers took the mode is read off the layers: the copies they cached, none when a weight was refused
            rec["layer_fp8"] = any(k.endswith("_fp8") for m in layers[0].modules() for k in m.__dict__)
            assert rec["layer_fp8"] == all(any(k.endswith("_fp8") for m in ly.modules() for k in m.__dict__) for ly in layers)
            rec["layer_fp4"] = any(k.endswith("_fp4") for m in layers[0].modules() for k in m.__dict__)
            assert rec["layer_fp4"] == all(any(k.endswith("_fp4") for m in ly.modules() for k in m.__dict__) for ly in layers)
            rec["layer_us"] = timed(layer_call, iters)
            for k in LINEARS:
                rec[k + "_us"] = timed(calls[k], iters)
        print("BENCH_DECODE_LINEAR " + json.dumps(rec), flush=True)


def resource_usage(fp8: bool = False, fp4: bool = False) -> list:
    """hipcc's kernel-resource-usage remarks for decode_linear.hip (``fp8`` / ``fp4``: decode_linear_fp8.hip / _fp4.hip with the
    Makefile's flag for that file; no GPU needed): one dict per instantiation"""
    stem = "decode_linear_fp4" if fp4 else ("decode_linear_fp8" if fp8 else "decode_linear")
    fp8 = fp8 or fp4                                         # the same extra flag
    src = os.path.join(ROOT, "cambrian_amd", "csrc", stem + ".hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage"]
                       + (["-fno-slp-vectorize"] if fp8 else []) + ["-c", src, "-o", os.devnull],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    if p.returncode != 0:
        raise SystemExit(p.stderr)
    out, cur = [], None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = dict(name=m.group(1)) if (stem + "_kernel") in m.group(1) else None
            if cur is not None:
                out.append(cur)
            continue
        m = re.search(r"remark:\s+.*?(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1) if m.group(1).endswith("Spill") else m.group(1).split(" ")[0]] = int(m.group(2))
    for r in out:
        m = re.search(r"ILi(\d)ELb([01])E", r["name"])
        r["tiles"], r["norm"] = int(m.group(1)), bool(int(m.group(2)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--fp8", action="store_true", help="the e4m3 weight stream against the bf16 decode_linear arm -> profiles/decode_fp8.md")
    ap.add_argument("--fp4", action="store_true", help="the MXFP4 weight stream against the bf16 and e4m3 arms -> profiles/decode_fp4.md")
    ap.add_argument("--step-log", help="with --fp4: output of tools/bench_decode_step.py --fp4 (ms per token on the one-call step)")
    ap.add_argument("--from-log", help="with --fp4: a run's output; write the note again without running anything")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="first batch only (rehearsal)")
    ap.add_argument("--resources", help="JSON written by --dump-resources; without it hipcc is run now")
    ap.add_argument("--dump-resources", metavar="FILE")
    ap.add_argument("--child", nargs=2, metavar=("GEOM", "ARM"))
    a = ap.parse_args()
    if a.fp4 and a.fp8:
        ap.error("--fp4 measures the e4m3 arm too: give one of --fp8 / --fp4")
    a.out = a.out or os.path.join(ROOT, "profiles", "decode_fp4.md" if a.fp4 else ("decode_fp8.md" if a.fp8 else "decode_linear.md"))
    if a.dump_resources:
        with open(a.dump_resources, "w") as fh:
            json.dump(resource_usage(a.fp8, a.fp4), fh, indent=1)
        return
    if a.iters < 30:
        ap.error("--iters: at least 30")
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup, a.quick, a.fp8, a.fp4)
        return
    recs = {}
    if a.fp4 and a.from_log:
        with open(a.from_log) as fh:
            for ln in fh:
                if ln.startswith("BENCH_DECODE_LINEAR "):
                    r = json.loads(ln[len("BENCH_DECODE_LINEAR "):])
                    recs[r["geom"], r["B"], r["arm"]] = r
    for geom in ([] if a.fp4 and a.from_log else GEOMS):
        for arm in (("fp4", "fp8", "on") if a.fp4 else ("fp8", "on") if a.fp8 else ("on", "off")):
            env = dict(os.environ, CAMBRIAN_AMD_DECODE_LINEAR="0" if arm == "off" else "1",
                       CAMBRIAN_AMD_DECODE_FP8="1" if arm == "fp8" else "0", CAMBRIAN_AMD_DECODE_FP4="1" if arm == "fp4" else "0")
            env.pop("CAMBRIAN_AMD_DECODE_ATTN", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", geom, arm, "--iters", str(a.iters),
                   "--warmup", str(a.warmup)] + (["--quick"] if a.quick else []) + (["--fp8"] if a.fp8 else []) + (["--fp4"] if a.fp4 else [])
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_decode_linear: child {geom}/{arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if ln.startswith("BENCH_DECODE_LINEAR "):
                    r = json.loads(ln[len("BENCH_DECODE_LINEAR "):])
                    recs[r["geom"], r["B"], r["arm"]] = r
                    print(ln, flush=True)
    if a.resources:
        with open(a.resources) as fh:
            res = json.load(fh)
    else:
        res = resource_usage(a.fp8, a.fp4)

    def f(t3):
        return f"{t3[0]:.1f} ({t3[1]:.1f} - {t3[2]:.1f})"

    if a.fp8:
        write_fp8(a, recs, res, f)
        return
    if a.fp4:
        write_fp4(a, recs, res, f)
        return

    lines = ["# Decode step: `cmb_decode_linear` (five launches per layer) against the stock sequence", "",
             f"Command: `python tools/bench_decode_linear.py --iters {a.iters} --warmup {a.warmup}`" + (" `--quick`" if a.quick else ""),
             f"on `{socket.gethostname()}` (MI355X), bf16, context {CTX}, one decoder layer with random frozen weights; HIP events, "
             f"median of 3 windows of {a.iters} calls (min - max in brackets), each arm in its own process, arms alternating.  "
             "`on` = `CAMBRIAN_AMD_DECODE_LINEAR=1`, `off` = `0` (the code path before the kernel existed: the yardstick).  Every call "
             "takes the next of a ring of weight sets of at least 768 MB.  MB = weight bytes of the shapes; GB/s = MB / on-arm time, "
             f"the share is of the ~{HBM_TBPS} TB/s an MI355X achieves from HBM.  A regime is **faster** when the on arm's median "
             "layer time is below the off arm's minimum window.", "",
             "## One `layer.decode` call", "",
             "| model | B | layer MB | on us | off us | off / on | on GB/s | of HBM | verdict |", "|---|---|---|---|---|---|---|---|---|"]
    verdicts = {}
    for geom in GEOMS:
        for B in BATCHES:
            o, z = recs.get((geom, B, "on")), recs.get((geom, B, "off"))
            if o is None or z is None:
                continue
            mb = sum(o["bytes"].values())
            gbs = mb / (o["layer_us"][0] * 1e-6) / 1e9
            fast = o["layer_us"][0] < z["layer_us"][1]
            verdicts[geom, B] = fast
            lines.append(f"| {geom} | {B} | {mb / 1e6:.1f} | {f(o['layer_us'])} | {f(z['layer_us'])} | "
                         f"{z['layer_us'][0] / o['layer_us'][0]:.2f} | {gbs:.0f} | {gbs / (HBM_TBPS * 1e3) * 100:.0f} % | "
                         f"{'faster' if fast else 'not faster'} |")
    lines += ["", "## The four linears alone (on: one `ops.decode_linear` call; off: the sequence it replaces)", "",
              "Read the small rows as launch counts, not as bandwidth: the timed loop issues every call from Python, as "
              "`generate()` does, and a call has a floor on the host that does not depend on the weight bytes (compare the rows "
              "of one linear across models: where the time stays put while the MB double, the floor is what is timed).  There the "
              "ratio is the launches and Python calls the fused call saves, and the GB/s column is not a figure of the kernel; "
              "only rows whose time grows with their MB say something about the weight stream.", "",
              "| model | B | linear | N x K | MB | on us | off us | off / on | on GB/s | of HBM |", "|---|---|---|---|---|---|---|---|---|---|"]
    for geom in GEOMS:
        shapes = linear_shapes({k: v for k, v in GEOMS[geom].items() if k != "lm"})
        for B in BATCHES:
            o, z = recs.get((geom, B, "on")), recs.get((geom, B, "off"))
            if o is None or z is None:
                continue
            for k in LINEARS:
                mb = o["bytes"][k]
                gbs = mb / (o[k + "_us"][0] * 1e-6) / 1e9
                lines.append(f"| {geom} | {B} | {k} | {shapes[k][0]} x {shapes[k][1]} | {mb / 1e6:.1f} | {f(o[k + '_us'])} | "
                             f"{f(z[k + '_us'])} | {z[k + '_us'][0] / o[k + '_us'][0]:.2f} | {gbs:.0f} | "
                             f"{gbs / (HBM_TBPS * 1e3) * 100:.0f} % |")
    fast = [f"{g} B {b}" for (g, b), v in verdicts.items() if v]
    slow = [f"{g} B {b}" for (g, b), v in verdicts.items() if not v]
    lines += ["", "## Verdict", "",
              "Faster (on median below off minimum): " + ("; ".join(fast) if fast else "nowhere") + ".",
              "Not faster: " + ("; ".join(slow) if slow else "nowhere") + ".", ""]
    from cambrian_amd import ops
    single = sorted({f"{k} at {g} B {b}" for (g, b, arm), r in recs.items() if arm == "on" for k in LINEARS
                     if r[k + "_us"][0] >= recs[g, b, "off"][k + "_us"][1]})
    lines += [f"Default in this tree: `ops.DECODE_LINEAR_DEFAULT_MAX_ROWS = {ops.DECODE_LINEAR_DEFAULT_MAX_ROWS}` (decode steps of at most "
              "that many sequences take the kernel unless `CAMBRIAN_AMD_DECODE_LINEAR` says otherwise; 0 = nowhere).  The rule is: on "
              "where the layer is faster, off where it is not.",
              "Single linears whose on-arm median is not below the off arm's minimum, inside layers that may still be faster as a "
              "whole: " + ("; ".join(single) if single else "none") + ".", "",
              "## Kernel resource usage (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950)", "",
              "| slab rows | norm prologue | VGPRs | AGPRs | SGPRs | LDS bytes | scratch bytes / lane | waves / SIMD |", "|---|---|---|---|---|---|---|---|"]
    for r in sorted(res, key=lambda r: (r["norm"], r["tiles"])):
        lines.append(f"| {8 * r['tiles']} | {'yes' if r['norm'] else 'no'} | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | "
                     f"{r.get('LDS')} | {r.get('ScratchSize')} | {r.get('Occupancy')} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def write_fp8(a, recs, res, f) -> None:
    """profiles/decode_fp8.md: the e4m3 stream (arm ``fp8``) against the bf16 ``decode_linear`` arm (``on``, the yardstick)"""
    from cambrian_amd import ops
    lines = ["# Decode step: `cmb_decode_linear_fp8` (e4m3 weights, one byte per weight) against the bf16 `cmb_decode_linear`", "",
             f"Command: `python tools/bench_decode_linear.py --fp8 --iters {a.iters} --warmup {a.warmup}`" + (" `--quick`" if a.quick else ""),
             f"on an MI355X, bf16 activations, context {CTX}, one decoder layer with random frozen weights; HIP "
             f"events, median of 3 windows of {a.iters} calls (min - max in brackets), each arm in its own process, arms alternating.  "
             "`fp8` = `CAMBRIAN_AMD_DECODE_FP8=1` (`layer.decode(..., fp8=True)`, `ops.decode_linear_fp8`), `bf16` = the default path "
             "(`ops.decode_linear`: the yardstick).  Every call takes the next of a ring of weight sets of at least 768 MB of the "
             "1-byte weights, in both arms.  MB = the bytes the arm streams (1 or 2 per weight); GB/s = fp8 MB / fp8 time, the share "
             f"is of the ~{HBM_TBPS} TB/s an MI355X achieves from HBM.  A row is **faster** when the fp8 arm's median is below the "
             "bf16 arm's minimum window.", "",
             "## One `layer.decode` call", "",
             "| model | B | fp8 MB | fp8 us | bf16 us | bf16 / fp8 | fp8 GB/s | of HBM | verdict |", "|---|---|---|---|---|---|---|---|---|"]
    slow = []
    for geom in GEOMS:
        for B in BATCHES:
            o, z = recs.get((geom, B, "fp8")), recs.get((geom, B, "on"))
            if o is None or z is None:
                continue
            if not o["layer_fp8"]:
                lines.append(f"| {geom} | {B} | - | {f(o['layer_us'])} | {f(z['layer_us'])} | - | - | - | not taken: the layer refused a weight (K > "
                             f"{ops.DECODE_FP8_MAX_K}, the row quantiser's reach, or K % 16), made no copy and ran on bf16 in both arms |")
                slow.append(f"{geom} B {B} layer (mode not taken)")
                continue
            mb = sum(o["bytes"].values())
            gbs = mb / (o["layer_us"][0] * 1e-6) / 1e9
            fast = o["layer_us"][0] < z["layer_us"][1]
            if not fast:
                slow.append(f"{geom} B {B} layer")
            lines.append(f"| {geom} | {B} | {mb / 1e6:.1f} | {f(o['layer_us'])} | {f(z['layer_us'])} | "
                         f"{z['layer_us'][0] / o['layer_us'][0]:.2f} | {gbs:.0f} | {gbs / (HBM_TBPS * 1e3) * 100:.0f} % | "
                         f"{'faster' if fast else 'not faster'} |")
    lines += ["", "## The four linears alone (one `ops.decode_linear_fp8` call against one `ops.decode_linear` call)", "",
              "Small linears sit on the host's launch floor (the timed loop issues every call from Python, as `generate()` does): "
              "where a linear's time stays put while its MB change, the floor is what is timed and the GB/s column is not a figure "
              "of the kernel.", "",
              "| model | B | linear | N x K | fp8 MB | fp8 us | bf16 us | bf16 / fp8 | fp8 GB/s | of HBM | verdict |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for geom in GEOMS:
        shapes = linear_shapes({k: v for k, v in GEOMS[geom].items() if k != "lm"})
        for B in BATCHES:
            o, z = recs.get((geom, B, "fp8")), recs.get((geom, B, "on"))
            if o is None or z is None:
                continue
            for k in LINEARS:
                mb = o["bytes"][k]
                gbs = mb / (o[k + "_us"][0] * 1e-6) / 1e9
                fast = o[k + "_us"][0] < z[k + "_us"][1]
                if not fast:
                    slow.append(f"{geom} B {B} {k}")
                lines.append(f"| {geom} | {B} | {k} | {shapes[k][0]} x {shapes[k][1]} | {mb / 1e6:.1f} | {f(o[k + '_us'])} | "
                             f"{f(z[k + '_us'])} | {z[k + '_us'][0] / o[k + '_us'][0]:.2f} | {gbs:.0f} | "
                             f"{gbs / (HBM_TBPS * 1e3) * 100:.0f} % | {'faster' if fast else 'not faster'} |")
    done = [f"{g} {k}: {'faster' if (g + ' B 1 ' + k) not in slow else 'NOT faster'}" for g in ("llama3-8b", "yi-34b")
            for k in ("gate_up", "down") if (g, 1, "fp8") in recs]
    lines += ["", "## Verdict", "",
              "The rows the mode exists for (B = 1, time grows with bytes) — " + "; ".join(done) + ".",
              "Not faster (fp8 median not below the bf16 minimum): " + ("; ".join(slow) if slow else "nowhere") + ".",
              "The mode stays opt-in whatever this table says: it changes numerics.", "",
              "## Kernel resource usage (`hipcc -Rpass-analysis=kernel-resource-usage -fno-slp-vectorize`, gfx950)", "",
              "| slab rows | norm prologue | VGPRs | AGPRs | SGPRs | VGPR spills | SGPR spills | LDS bytes | scratch bytes / lane | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r in sorted(res, key=lambda r: (r["norm"], r["tiles"])):
        lines.append(f"| {8 * r['tiles']} | {'yes' if r['norm'] else 'no'} | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | "
                     f"{r.get('VGPRs Spill')} | {r.get('SGPRs Spill')} | {r.get('LDS')} | {r.get('ScratchSize')} | {r.get('Occupancy')} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def write_fp4(a, recs, res, f) -> None:
    """profiles/decode_fp4.md: the MXFP4 stream (arm ``fp4``) against the bf16 ``decode_linear`` arm (``on``) and the e4m3 arm
    (``fp8``); a verdict against each on every row"""
    def verdict(o, z):
        return "faster" if o[0] < z[1] else "not faster"

    lines = ["# Decode step: `cmb_decode_linear_fp4` (MXFP4 weights, 4.25 bits per weight) against the bf16 and e4m3 linears", "",
             f"Command: `python tools/bench_decode_linear.py --fp4 --iters {a.iters} --warmup {a.warmup}`" + (" `--quick`" if a.quick else ""),
             f"on an MI355X, bf16 activations, context {CTX}, one decoder layer with random frozen weights; HIP "
             f"events, median of 3 windows of {a.iters} calls (min - max in brackets), each arm in its own process, the three arms "
             "alternating per geometry.  `fp4` = `CAMBRIAN_AMD_DECODE_FP4=1` (`layer.decode(..., fp4=True)`, `ops.decode_linear_fp4`), "
             "`fp8` = `CAMBRIAN_AMD_DECODE_FP8=1` (`ops.decode_linear_fp8`), `bf16` = the default path (`ops.decode_linear`).  Every "
             "call takes the next of a ring of weight sets of at least 768 MB of the MXFP4 bytes, in all three arms.  fp4 MB = "
             "17 / 32 byte per weight (nibbles and scale bytes); GB/s = fp4 MB / fp4 time, the share is of the "
             f"~{HBM_TBPS} TB/s an MI355X achieves from HBM.  A row is **faster** than an arm when the fp4 median is below that arm's "
             "minimum window; `not faster` is said where that is what it is.", "",
             "## One `layer.decode` call", "",
             "| model | B | fp4 MB | fp4 us | fp8 us | bf16 us | bf16 / fp4 | fp8 / fp4 | fp4 GB/s | of HBM | vs bf16 | vs fp8 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slow = []
    for geom in GEOMS:
        for B in BATCHES:
            o, e, z = recs.get((geom, B, "fp4")), recs.get((geom, B, "fp8")), recs.get((geom, B, "on"))
            if o is None or e is None or z is None:
                continue
            taken = "taken" if o["layer_fp4"] else "NOT taken (the layer refused a weight and ran on bf16)"
            e_note = "" if e["layer_fp8"] else " (the fp8 arm's layer refused a weight and ran on bf16)"
            mb = sum(o["bytes"].values())
            gbs = mb / (o["layer_us"][0] * 1e-6) / 1e9
            v16, v8 = verdict(o["layer_us"], z["layer_us"]), verdict(o["layer_us"], e["layer_us"])
            slow += [f"{geom} B {B} layer vs {n}" for n, v in (("bf16", v16), ("fp8", v8)) if v != "faster"]
            lines.append(f"| {geom} | {B} | {mb / 1e6:.1f} | {f(o['layer_us'])} | {f(e['layer_us'])} | {f(z['layer_us'])} | "
                         f"{z['layer_us'][0] / o['layer_us'][0]:.2f} | {e['layer_us'][0] / o['layer_us'][0]:.2f} | {gbs:.0f} | "
                         f"{gbs / (HBM_TBPS * 1e3) * 100:.0f} % | {v16}; mode {taken} | {v8}{e_note} |")
    lines += ["", "## The four linears alone (one `ops.decode_linear_fp4` call against one `ops.decode_linear_fp8` / `ops.decode_linear` call)", "",
              "Small linears sit on the host's launch floor (the timed loop issues every call from Python, as `generate()` does): "
              "where a linear's time stays put while its MB change, the floor is what is timed and the GB/s column is not a figure "
              "of the kernel.  Yi-34B's `down` (K = 20480) is past the e4m3 row quantiser's reach: its fp8 figure is the e4m3 kernel "
              "on random finite bytes, as in profiles/decode_fp8.md.", "",
              "| model | B | linear | N x K | fp4 MB | fp4 us | fp8 us | bf16 us | bf16 / fp4 | fp8 / fp4 | fp4 GB/s | of HBM | vs bf16 | vs fp8 |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for geom in GEOMS:
        shapes = linear_shapes({k: v for k, v in GEOMS[geom].items() if k != "lm"})
        for B in BATCHES:
            o, e, z = recs.get((geom, B, "fp4")), recs.get((geom, B, "fp8")), recs.get((geom, B, "on"))
            if o is None or e is None or z is None:
                continue
            for k in LINEARS:
                mb = o["bytes"][k]
                gbs = mb / (o[k + "_us"][0] * 1e-6) / 1e9
                v16, v8 = verdict(o[k + "_us"], z[k + "_us"]), verdict(o[k + "_us"], e[k + "_us"])
                slow += [f"{geom} B {B} {k} vs {n}" for n, v in (("bf16", v16), ("fp8", v8)) if v != "faster"]
                lines.append(f"| {geom} | {B} | {k} | {shapes[k][0]} x {shapes[k][1]} | {mb / 1e6:.1f} | {f(o[k + '_us'])} | "
                             f"{f(e[k + '_us'])} | {f(z[k + '_us'])} | {z[k + '_us'][0] / o[k + '_us'][0]:.2f} | "
                             f"{e[k + '_us'][0] / o[k + '_us'][0]:.2f} | {gbs:.0f} | {gbs / (HBM_TBPS * 1e3) * 100:.0f} % | {v16} | {v8} |")
    lines += ["", "## Verdict", "",
              "Not faster (fp4 median not below the other arm's minimum): " + ("; ".join(slow) if slow else "nowhere") + ".",
              "The mode stays opt-in whatever this table says: it changes numerics, and coarsely (about 11 % relative L2 error per "
              "weight on Gaussian weights; task quality on real checkpoints is unmeasured).", ""]
    if a.step_log:
        from bench_decode_step import fp4_step_section
        lines += fp4_step_section(a.step_log) + [""]
    lines += ["## Kernel resource usage (`hipcc -Rpass-analysis=kernel-resource-usage -fno-slp-vectorize`, gfx950)", "",
              "| slab rows | norm prologue | VGPRs | AGPRs | SGPRs | VGPR spills | SGPR spills | LDS bytes | scratch bytes / lane | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r in sorted(res, key=lambda r: (r["norm"], r["tiles"])):
        lines.append(f"| {8 * r['tiles']} | {'yes' if r['norm'] else 'no'} | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | "
                     f"{r.get('VGPRs Spill')} | {r.get('SGPRs Spill')} | {r.get('LDS')} | {r.get('ScratchSize')} | {r.get('Occupancy')} |")
    lines += ["", "The 32-row slab with the norm prologue is built for one workgroup per CU (`__launch_bounds__(256, 1)`): with two "
              "it needs 116 bytes of scratch per lane; its AGPRs are register overflow, not accumulators."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
