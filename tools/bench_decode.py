"""Decode step of one decoder layer: the fused kernel (``cmb_decode_attn``) against the stock SDPA branch
(``CAMBRIAN_AMD_DECODE_ATTN=0``), same box, same run.

    python tools/bench_decode.py [--out profiles/decode_attn.md] [--iters 100] [--quick]

For Llama-3-8B (32 / 8 / 128) and Yi-34B (56 / 8 / 128) in bf16, context 2048 and 8192, batch 1 and 16, each arm runs in a
fresh child process (one per model geometry and arm, alternating) and times with HIP events, after a warm-up:
  * ``layer``  one ``LlamaDecoderLayer.decode`` call (norms, projections, attention, o_proj, MLP), random frozen weights;
  * ``attn``   the attention part alone, from the projection outputs to the o_proj input: ``ops.decode_attention`` in the
               kernel arm, the SDPA body of ``LlamaAttention.decode`` (two ropes, two cache writes, SDPA) in the other.
Every call works on the next of a ring of K / V caches (>= 512 MB in total, at most 32 pairs), as the layers of a model do,
so a cache is not served from the last-level cache of the previous call.  ``bytes`` is what the algorithm must read of K and
V: 2 * B * nkv * ctx * hd * 2 B; GB/s = bytes / attn time, shown against the ~6.3 TB/s an MI355X achieves from HBM.
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

GEOMS = {"llama3-8b": dict(hidden_size=4096, intermediate_size=14336, num_attention_heads=32, num_key_value_heads=8),
         "yi-34b": dict(hidden_size=7168, intermediate_size=20480, num_attention_heads=56, num_key_value_heads=8)}
SHAPES = [(2048, 1), (2048, 16), (8192, 1), (8192, 16)]        # (context, batch)
HBM_TBPS = 6.3


def kv_bytes(B: int, nkv: int, ctx: int, hd: int) -> int:
    return 2 * B * nkv * ctx * hd * 2


def child(geom: str, arm: str, iters: int, warmup: int, quick: bool) -> None:
    import torch
    import torch.nn.functional as F
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import cambrian_llama as CL
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode: no GPU visible")
    assert ops.decode_attention_enabled() == (arm == "kernel")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    g = GEOMS[geom]
    cfg = CL.CambrianConfig(vocab_size=64, num_hidden_layers=1, rms_norm_eps=1e-5, rope_theta=500000.0,
                            max_position_embeddings=16384, **g)
    torch.manual_seed(0)
    layer = CL.LlamaDecoderLayer(cfg, dev, dt).requires_grad_(False)
    att = layer.self_attn
    nh, nkv, hd = att.nh, att.nkv, att.hd

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

    for ctx, B in (SHAPES[:1] if quick else SHAPES):
        t = ctx                                                   # ctx cached keys, the new token goes to slot ctx
        pair = 2 * B * nkv * (ctx + 8) * hd * 2
        ring = max(2, min(32, -(-(512 << 20) // pair)))
        caches = [(torch.randn(B, nkv, ctx + 8, hd, device=dev, dtype=dt), torch.randn(B, nkv, ctx + 8, hd, device=dev, dtype=dt))
                  for _ in range(ring)]
        mask = torch.ones(B, ctx + 8, dtype=torch.bool, device=dev)
        x = torch.randn(B, 1, g["hidden_size"], device=dev, dtype=dt)
        cos, sin = ops.rope_table(torch.full((B, 1), ctx, device=dev), hd, 500000.0)
        row = torch.randn(B, (nh + 2 * nkv) * hd, device=dev, dtype=dt)
        q, k, v = row[:, :nh * hd], row[:, nh * hd:(nh + nkv) * hd], row[:, (nh + nkv) * hd:]

        def layer_call(i):
            kc, vc = caches[i % ring]
            layer.decode(x, cos, sin, kc, vc, t, mask)

        def attn_call(i):
            kc, vc = caches[i % ring]
            if arm == "kernel":
                return ops.decode_attention(q, k, v, cos, sin, kc, vc, t, mask)
            km = mask[:, :t + 1]                                   # the SDPA body of LlamaAttention.decode
            qr = ops.rope(q.reshape(B, nh, hd), cos, sin).view(B, 1, nh, hd).transpose(1, 2)
            kc[:, :, t] = ops.rope(k.reshape(B, nkv, hd), cos, sin)
            vc[:, :, t] = v.reshape(B, nkv, hd)
            o = F.scaled_dot_product_attention(qr, kc[:, :, :t + 1], vc[:, :, :t + 1], attn_mask=km[:, None, None, :],
                                               enable_gqa=nkv != nh)
            return o.transpose(1, 2).reshape(B, 1, nh * hd)

        with torch.no_grad():
            for i in range(warmup):
                layer_call(i)
                attn_call(i)
            torch.cuda.synchronize()
            lay = timed(layer_call, iters)
            at = timed(attn_call, iters)
        rec = dict(geom=geom, arm=arm, ctx=ctx, B=B, nh=nh, nkv=nkv, hd=hd, ring=ring, iters=iters,
                   layer_us=lay, attn_us=at, kv_bytes=kv_bytes(B, nkv, ctx, hd),
                   plan=list(ops.decode_attention_plan(B, nkv, t)) if arm == "kernel" else None)
        print("BENCH_DECODE " + json.dumps(rec), flush=True)
        del caches
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn.md"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="first shape only (rehearsal)")
    ap.add_argument("--child", nargs=2, metavar=("GEOM", "ARM"))
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters: at least 50")
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup, a.quick)
        return
    recs = {}
    for geom in GEOMS:
        for arm in ("kernel", "sdpa"):
            env = dict(os.environ, CAMBRIAN_AMD_DECODE_ATTN="1" if arm == "kernel" else "0")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", geom, arm, "--iters", str(a.iters),
                   "--warmup", str(a.warmup)] + (["--quick"] if a.quick else [])
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
            if p.returncode != 0:                   # a child that failed ends the run: nothing else is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"bench_decode: child {geom}/{arm} exited with {p.returncode}")
            for ln in p.stdout.splitlines():
                if ln.startswith("BENCH_DECODE "):
                    r = json.loads(ln[len("BENCH_DECODE "):])
                    recs[r["geom"], r["ctx"], r["B"], r["arm"]] = r
                    print(ln, flush=True)
    lines = ["# Decode step: `cmb_decode_attn` against the SDPA branch", "",
             f"Command: `python tools/bench_decode.py --iters {a.iters} --warmup {a.warmup}`" + (" `--quick`" if a.quick else ""),
             f"on `{socket.gethostname()}` (MI355X), bf16, one `LlamaDecoderLayer`, random frozen weights; HIP events, median of 3 "
             f"windows of {a.iters} calls (min - max in brackets), each arm in its own process.  `attn` = projection outputs to o_proj "
             "input; `layer` = the whole `decode` call.  K / V bytes = 2 * B * nkv * ctx * hd * 2 B, the least the step must "
             f"read; the share is of the ~{HBM_TBPS} TB/s an MI355X achieves from HBM.", "",
             "| model | ctx | B | splits x chunk | attn kernel us | attn SDPA us | x | K/V MB | kernel GB/s | of HBM | layer kernel us | layer SDPA us | x |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for geom in GEOMS:
        for ctx, B in SHAPES:
            kr, sr = recs.get((geom, ctx, B, "kernel")), recs.get((geom, ctx, B, "sdpa"))
            if kr is None or sr is None:
                continue

            def f(t3):
                return f"{t3[0]:.1f} ({t3[1]:.1f} - {t3[2]:.1f})"

            gbs = kr["kv_bytes"] / (kr["attn_us"][0] * 1e-6) / 1e9
            lines.append(f"| {geom} | {ctx} | {B} | {kr['plan'][0]} x {kr['plan'][1]} | {f(kr['attn_us'])} | {f(sr['attn_us'])} | "
                         f"{sr['attn_us'][0] / kr['attn_us'][0]:.2f} | {kr['kv_bytes'] / 1e6:.1f} | {gbs:.0f} | "
                         f"{gbs / (HBM_TBPS * 1e3) * 100:.0f} % | {f(kr['layer_us'])} | {f(sr['layer_us'])} | "
                         f"{sr['layer_us'][0] / kr['layer_us'][0]:.2f} |")
            if kr["layer_us"][0] >= sr["layer_us"][0]:
                slower.append(f"{geom} ctx {ctx} B {B}")
    lines += ["", "Layer time with the kernel is lower at every listed shape." if not slower else
              "Layer time with the kernel is NOT lower at: " + "; ".join(slower) + "."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
