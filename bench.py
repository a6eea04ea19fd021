#!/usr/bin/env python
"""bench.py — train images/sec (fwd+bwd) of the Cambrian-8B hot path on MI355X.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic input per GPU: the four frozen vision towers
(SigLIP-SO400M/14@384, CLIP-L/14@336, DINOv2-g/14@378, ConvNeXt-XXL@1024, forward), aux projectors, 3-layer SVA
connector, mm_projector, newline/splice, the Llama-3-8B decoder with the 10 in-LLM SVA layers, fp32 logits + loss,
backward through everything that trains in the reference's pre-training stage (SVA + projectors; LLM and towers
frozen, train_fsdp.py:1677-1685), gradient all-reduce (RCCL) and the AdamW update.  Workload = BASELINE.json
configs[2] (the configuration the metric is quoted on; it fits one GPU), random-init weights, synthetic data
(SURVEY.md §8d).  Weak scaling: the per-GPU batch is fixed.

`python bench.py --gpus N` with N > 1 and no torchrun environment re-launches itself through torch.distributed.run on
127.0.0.1 (one rank per GPU) and relays rank 0's JSON line.

A plain run does only what the headline figure needs: set-up (with the start-up GEMM calibration below), warm-up, the
timed steps, --dump-outputs DIR if given, and one JSON line with the contract keys and `config`.  With --full the JSON
line also carries (each measured after the timed steps or, for the roofline's event pairs, inside them)
  roofline     — the dominant HIP kernel (the bf16 MFMA GEMM): algorithmic FLOPs of every launch in the timed region
                 / its HIP-event duration on the launch stream, against the 2.5 PFLOP/s dense bf16 MFMA peak;
                 .region        the tower + SVA part of the step (what the north star's ">= 40 %" is about): its
                                algorithmic FLOPs / the HIP-event spans of encode_images + aux projectors + connector +
                                mm_projector + splice and of the 10 in-LLM SVA layers, forward and backward, measured in
                                the timed region;
                 .all_own_gemm  every own GEMM launch (all tile configurations, wgrad split-K included), from two extra
                                profiled steps after the timed region (an event pair per launch perturbs the stream);
                 .ab            same-process A/B after the timed region: the 4-wave kernel, the 8-wave kernel and
                                torch.matmul (hipBLASLt) on the dominant launch shape, with the box's identity;
                 .calibration   the start-up choice between the two 256 x 256 kernels per hot shape on THIS box;
  parity       — the tolerance the benched dtype actually meets against the fp32 oracle (and where that is tested);
  cpu_baseline — the reference's own modules timed on host cores (kind "reference"), with live samples on this host.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

os.environ.setdefault("CAMBRIAN_AMD_RANDOM_INIT", "1")  # random-init weights of the named architecture (no checkpoints offline)
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 (MI355X_MICROARCH.md)

# forward GFLOP per image of the release-8B path (BASELINE.md §2 / SURVEY.md §8d)
TOWER_GFLOP = 381.9 + 666.4 + 1785.7 + 6334.9
SVA_SIDE_GFLOP = 939.9
# executed but not GEMM launches, per image: tower attention 4 N^2 d per head and layer (CLIP 32.7 + SigLIP 66.1 + DINOv2 131.0 GFLOP),
# depthwise 7x7 98 FLOP x 324 M outputs (31.8), absorbed SVA kernels' 16 x 16 x 1024 products forward + backward x 13 layers (19.7)
EXEC_NON_GEMM_TFLOP_PER_IMAGE = (32.7 + 66.1 + 131.0 + 31.8 + 19.7) / 1e3


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("CAMBRIAN_BENCH_BATCH", "0")),
                    help="images per GPU per step (0 = default: 24 on a 288 GB MI355X, else 16).  The reference runs "
                         "per_device_train_batch_size 8 on 32 GB TPU-v4 cores (pretrain_cambrian_8b.sh:37); no activation "
                         "re-computation here: 16 images use 170 GB, 24 use 231 GB of the 288 GB and fill the chip better on the "
                         "towers' mid-size GEMMs (same box: 14.67 / 14.74 / 14.88 images/s at 16 / 20 / 24; 32 does not fit).  A "
                         "single-GPU run that hits out-of-memory in its first step falls back to 16")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--zero2", action="store_true", help="ZeRO-2 (reduce-scatter grads, sharded AdamW, all-gather params: BASELINE "
                    "config 4's partitioning) instead of all-reduce + replicated AdamW")
    ap.add_argument("--zero3", action="store_true", help="ZeRO-3 (BASELINE config 5's partitioning; XLA-FSDP full_shard in the "
                    "reference): every decoder layer is a Zero3Unit — parameters sharded 1/world, all-gathered around the "
                    "layer's forward and backward; the SVA / projector parameters stay replicated (GradSync)")
    ap.add_argument("--preset", choices=["8b", "13b", "34b"], default="8b",
                    help="decoder geometry + in-LLM SVA placement: 8b = Llama-3-8B (the headline, BASELINE configs[2]); "
                         "13b = Vicuna-13B (H 5120, 40 layers, 10 SVA layers stride 4, image_position 35: configs[3]); "
                         "34b = Yi-34B (H 7168, 60 layers, 9 SVA layers stride 7, image_position 87: configs[4]).  Anything "
                         "but 8b is not the headline line; combine with --llm-layers to fit / for quick runs (marked INVALID)")
    ap.add_argument("--no-masked-case", action="store_true",
                    help="skip the extra (not headline) steps on letter-boxed (336, 224) / (224, 336) images: real collator "
                         "batches carry key-padding and SVA window masks (SURVEY.md §8d second case)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--fp8-projections", action="store_true",
                    help="BASELINE configs[4] mode: forward GEMMs of the KV-side SVA projections in fp8 (marks the line: "
                         "not the bf16 headline configuration)")
    ap.add_argument("--input-pipeline", action="store_true",
                    help="feed decoded uint8 images through the GPU input pipeline (SURVEY.md §8f N3: pinned H2D + "
                         "cmb_image_preprocess on a side stream, one batch ahead) instead of resident pixel tensors")
    ap.add_argument("--no-calibration", action="store_true",
                    help="skip the start-up calibration of the 256 x 256 GEMM kernel choice (library cost model only)")
    ap.add_argument("--no-ab", action="store_true", help="skip the same-process kernel A/B after the timed region")
    ap.add_argument("--no-gemm-pass", action="store_true",
                    help="skip the two extra profiled steps behind roofline.all_own_gemm")
    ap.add_argument("--gemm-report", type=str, default=None, help="write a per-shape table of the hot-path GEMM launches (JSON)")
    ap.add_argument("--unfreeze-towers", action="store_true",
                    help="--unfreeze_mm_vision_tower of the reference (SURVEY.md §8f N4): the four towers train too (fp32 master "
                         "parameters, autograd operators); NOT the headline line — the release recipe keeps them frozen")
    ap.add_argument("--llm-layers", type=int, default=None, help="debug only: fewer decoder layers (marks the line INVALID)")
    ap.add_argument("--stage", choices=["pretrain", "finetune"], default="pretrain",
                    help="pretrain (the headline: SVA + projectors train, LLM + towers frozen: scripts/cambrian/pretrain_cambrian_8b.sh) "
                         "or finetune (scripts/cambrian/finetune_cambrian_8b.sh: the whole LLM trains too — 8 B parameters, "
                         "activation re-computation on, default batch 4; NOT the headline line)")
    ap.add_argument("--grad-ckpt", action="store_true",
                    help="activation re-computation of the decoder layers and the in-LLM SVA layers (the reference's "
                         "--gradient_checkpointing True / fsdp_config.json:9; implied by --stage finetune)")
    ap.add_argument("--tower-recompute", action="store_true",
                    help="with --unfreeze-towers: per-block activation re-computation inside the four towers")
    ap.add_argument("--bucket-mb", type=float, default=64.0, help="gradient bucket size of GradSync / ZeRO-2 (MiB)")
    ap.add_argument("--bf16-buckets", action="store_true",
                    help="opt-in: GradSync's all-reduce on bf16 copies of the fp32 buckets (half the exchange; the mean to bf16 "
                         "rounding; marks the line NOT_HEADLINE)")
    ap.add_argument("--scored-rows", action="store_true",
                    help="lm_head + cross-entropy only over the scored positions (config.fused_loss = 'scored_rows': shifted label != "
                         "-100; identical loss and gradients, no logits returned) — NOT the headline line, which computes every row "
                         "as the reference does")
    ap.add_argument("--verbose-line", action="store_true",
                    help="print the FULL JSON line (20-row calibration table, A/B variants, parity prose, cpu_baseline parts); the "
                         "default line is the compact one (< 8 KB, scalar roofline keys) and the full one is written to "
                         "gpurun_out/bench_line_full.json")
    ap.add_argument("--no-comm-pass", action="store_true",
                    help="N > 1: skip the 5 communication-only exchanges after the timed region (comm_only_ms / bus_gb_per_s)")
    ap.add_argument("--comm-only", action="store_true",
                    help="no model step: run only the gradient-exchange collectives of the configured parameter set (GradSync "
                         "all-reduce, or the ZeRO-2 reduce-scatter + all-gather with --zero2) for --steps steps and print the bus "
                         "bandwidth per bucket — the communication breakdown beside a scaling curve")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: roofline (event pairs in the timed region, the two profiled GEMM "
                         "steps, the kernel A/B), the letter-boxed masked case, the N > 1 rank spread and communication pass, box "
                         "identity, parity and CPU baseline.  Off by default: a plain run sets up, warms up, times --steps steps "
                         "and prints the contract keys")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as float32 .npy files in DIR: loss, "
                         "seeded rows of the logits (taken before the backward overwrites them), and seeded samples of the "
                         "trainable parameters after the update and of their gradients (< 64 MB in all; rank 0).  The logits "
                         "rows are copied inside the last timed step (an index_select of 64 rows before its backward), so "
                         "compare ms_per_step only between runs that both dump or both do not")
    return ap.parse_args()


# decoder geometry and in-LLM SVA placement of the three release sizes (scripts/cambrian/pretrain_cambrian_{8b,13b,34b}.sh;
# SURVEY.md §8d table).  head_dim is 128 for all three, so the flash kernels serve them unchanged.
PRESETS = {
    "8b": dict(llm={}, sva=dict(n=10, start=0, stride=3, image_position=91), name="Llama-3-8B"),
    "13b": dict(llm=dict(vocab_size=32000, hidden_size=5120, intermediate_size=13824, num_hidden_layers=40,
                         num_attention_heads=40, num_key_value_heads=40, rope_theta=10000.0, max_position_embeddings=4096),
                sva=dict(n=10, start=0, stride=4, image_position=35), name="Vicuna-13B"),
    "34b": dict(llm=dict(vocab_size=64000, hidden_size=7168, intermediate_size=20480, num_hidden_layers=60,
                         num_attention_heads=56, num_key_value_heads=8, rope_theta=5000000.0, max_position_embeddings=4096),
                sva=dict(n=9, start=0, stride=7, image_position=87), name="Yi-34B"),
}


def build_model(dev, llm_layers=None, preset="8b", unfreeze_towers=False, stage="pretrain", grad_ckpt=False,
                tower_recompute=False):
    from cambrian_amd.model.language_model.cambrian_llama import (CambrianLlamaForCausalLM, apply_release_8b_vision_config,
                                                                llama3_8b_config)
    geo = dict(PRESETS[preset]["llm"])
    if llm_layers is not None:
        geo["num_hidden_layers"] = llm_layers
    cfg = llama3_8b_config(**geo)
    apply_release_8b_vision_config(cfg)
    cfg.unfreeze_mm_vision_tower = bool(unfreeze_towers)
    sva = PRESETS[preset]["sva"]
    depth = cfg.num_hidden_layers
    cfg.num_of_vision_sampler_layers = len([k for k in range(sva["n"]) if sva["start"] + k * sva["stride"] < depth])
    cfg.start_of_vision_sampler_layers, cfg.stride_of_vision_sampler_layers = sva["start"], sva["stride"]
    cfg.image_position = sva["image_position"]
    cfg.fused_loss = True  # fp32 log-sum-exp over the bf16 logits, no logits.float() copy (same loss / gradients)
    torch.manual_seed(0)
    model = CambrianLlamaForCausalLM(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for n, p in model.named_parameters():  # random init of that architecture (no checkpoints offline)
            if p.device != dev:
                continue
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
        model.model.image_newline.data = torch.randn(cfg.hidden_size) / cfg.hidden_size ** 0.5
    model = model.to(dev)
    for t in model.model.vision_tower_aux_list:
        t.load_model()
    if unfreeze_towers:   # registered sub-modules, as initialize_vision_modules does for this mode (cambrian_arch.py:125-126)
        model.model.vision_tower_aux_list = torch.nn.ModuleList(model.model.vision_tower_aux_list)
    train_keys = ("mm_projector", "pos_emb", "vision_sampler", "vision_sampler_layers", "vision_query", "image_newline")
    if unfreeze_towers:
        train_keys += ("vision_tower_aux_list",)
    for n, p in model.named_parameters():
        # finetune stage (train_fsdp.py:1677-1695 with tune_mm_mlp_adapter off): everything but the towers trains
        p.requires_grad_(any(k in n for k in train_keys) or (stage == "finetune" and "vision_tower_aux_list" not in n))
    cfg.gradient_checkpointing = bool(grad_ckpt or stage == "finetune")
    if unfreeze_towers and tower_recompute:
        for t in model.model.vision_tower_aux_list:
            for m in t.modules():          # TrainableViT / TrainableConvNeXt: per-block activation re-computation
                if hasattr(m, "recompute"):
                    m.recompute = True
    return model, cfg


def cpu_port_sample():
    """Oracle (CPU port of the reference path) on a bounded sample ON THIS HOST: one SVA connector layer forward+backward on
    one image's 10 944 KV tokens, extrapolated by algorithmic FLOPs to the tower+SVA part of a train step."""
    from oracle import sva as OS
    # 256 threads on this host's 256 logical cores is ~50x SLOWER than 32 for these [576..9216, 1024] GEMMs
    # (oversubscribed OpenMP across sockets): use the thread count a CPU user of the reference would pick.
    ncores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(ncores)
    gen = torch.Generator().manual_seed(0)
    kv_sizes, qside, hidden = [1, 1, 1, 4], 24, 1024
    p = {k: v.requires_grad_() for k, v in OS.init_sampler_params(hidden, hidden, [hidden] * 4, kv_sizes, hidden, 1, gen).items()}
    Bq = qside * qside
    q = torch.randn(Bq, 1, hidden, generator=gen)
    ctx = torch.randn(Bq, 1, hidden, generator=gen)
    kvs = [torch.randn(Bq, s * s, hidden, generator=gen) for s in kv_sizes]
    masks = [torch.ones(Bq, s * s, dtype=torch.bool) for s in kv_sizes]
    t0 = time.perf_counter()
    reps = 0
    while reps < 4 and (time.perf_counter() - t0) < 10.0:  # bounded: <= ~12 s of CPU work
        out = OS.vision_token_sampler(p, q, ctx, kvs, masks)
        out.sum().backward()
        reps += 1
    dt = (time.perf_counter() - t0) / reps
    layer_gflop = 54.4 * 3.0  # fwd + bwd of one connector layer
    gflops = layer_gflop / dt
    step_gflop = TOWER_GFLOP + 3.0 * SVA_SIDE_GFLOP  # towers fwd + SVA side fwd+bwd, per image
    return {"value": gflops / step_gflop, "unit": "images/s (tower+SVA part of the step)", "cores": ncores, "kind": "port",
            "sample": f"oracle/sva.py: 1 SVA connector layer fwd+bwd, 1 image (576 queries, 10944 KV tokens), fp32, "
                      f"{dt:.2f} s/iter = {gflops:.0f} GFLOP/s on this host; extrapolated by algorithmic FLOPs to "
                      f"{step_gflop:.0f} GFLOP/img (towers fwd + 3x SVA side)"}


def cpu_hf_tower_sample():
    """The third-party tower module the reference calls (transformers CLIPVisionModel, clip_encoder.py:47,104) at the
    release dimensions (CLIP-L/14@336, 24 layers), random init, forward, B = 1, fp32, timed ON THIS HOST (bounded: one
    warm-up + up to 3 runs / 8 s) — shows how this host's cores compare with the build container's behind
    ``cpu_baseline.value``.  None when transformers is not importable here."""
    try:
        from transformers import CLIPVisionConfig, CLIPVisionModel
    except Exception:
        return None
    ncores = min(os.cpu_count() or 1, 8)
    torch.set_num_threads(ncores)
    cfg = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                           image_size=336, patch_size=14)
    torch.manual_seed(0)
    m = CLIPVisionModel(cfg).eval()
    x = torch.randn(1, 3, 336, 336)
    with torch.no_grad():
        m(x)
        t0, reps = time.perf_counter(), 0
        while reps < 3 and (time.perf_counter() - t0) < 8.0:
            m(x, output_hidden_states=True)
            reps += 1
    dt = (time.perf_counter() - t0) / reps
    return {"module": "transformers.CLIPVisionModel (CLIP-L/14@336, 24 layers, random init)", "cores": ncores,
            "s_per_image_fwd": dt, "gflops": 381.9 / dt,
            "build_container_s": "see cpu_baseline.parts_s['clip']" }


def cpu_baseline():
    """Top level = the reference's OWN modules timed on host cores (tools/cpu_reference_baseline.py, committed under
    profiles/; the reference tree does not exist on the GPU box, so that run happens in the build container): real
    VisionTokenSampler x 13, real prepare_inputs_labels_for_multimodal, installed-HF towers at the release dimensions,
    forward + backward, B = 1, fp32, 8 cores.  Beside it two live samples on THIS host: the CPU port of one SVA layer
    (extrapolated by FLOPs) and the HF CLIP-L tower forward."""
    ref = reference_cpu_run()
    port = cpu_port_sample()
    if ref is None:
        port["note"] = "profiles/r02_cpu_reference_baseline.json missing: the live port sample is the only baseline"
        return port
    ref["live_port_sample"] = port
    try:
        hf = cpu_hf_tower_sample()
        if hf is not None:
            ref["live_hf_tower_sample"] = hf
    except Exception as e:
        ref["live_hf_tower_sample"] = {"error": repr(e)}
    return ref


def reference_cpu_run():
    """The newest profiles/rNN_cpu_reference_baseline.json as the bench line's cpu_baseline object (kind "reference")."""
    import glob
    try:
        path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_cpu_reference_baseline.json")))[-1]
        with open(path) as f:
            d = json.load(f)
        return {"value": d["images_per_s"], "unit": "images/s (tower+SVA part of the step, B = 1, fp32)", "cores": d["cores"],
                "kind": "reference", "host": d.get("host"), "sample": d["what"], "parts_s": d["parts"],
                "measured_where": f"build container (same image as the GPU box; /root/reference is not shipped to the GPU box), "
                                  f"read from profiles/{os.path.basename(path)} (timed {d.get('timed_on', 'in round 2')}) — not timed in this run",
                "source": "tools/cpu_reference_baseline.py"}
    except Exception:
        return None


def box_identity(dev):
    """Which box produced this line: host name, device name, CU count, and what rocm-smi says about clocks / power cap
    (bounded: 10 s, None on any failure).  The same binary measures 1107-1178 ms/step from box to box."""
    import socket
    import subprocess
    ident = {"host": socket.gethostname()}
    try:
        pr = torch.cuda.get_device_properties(dev)
        ident.update(device=pr.name, cus=pr.multi_processor_count, hbm_gb=round(pr.total_memory / 2 ** 30, 1),
                     gcn_arch=getattr(pr, "gcnArchName", None))
    except Exception:
        pass
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--showmaxpower", "--showperflevel",
                              "--showtemp", "--json"], capture_output=True, text=True, timeout=10).stdout
        d = json.loads(out[out.index("{"):])
        card = d.get("card0", next(iter(d.values())))
        keep = {}
        for k, v in card.items():
            kl = k.lower()
            if any(t in kl for t in ("sclk", "mclk", "fclk", "power", "performance level", "temperature (sensor junction)")):
                keep[k] = v
        ident["rocm_smi"] = keep
    except Exception as e:
        ident["rocm_smi"] = None
        ident["rocm_smi_error"] = repr(e)[:200]
    return ident


def gemm_ab(dev, iters=20):
    """Same-process A/B on the dominant launch shape (ConvNeXt-XXL stage-3 fc1, 16 images: 65536 x 6144 x 1536): the 4-wave
    kernel (tile_hint 2590), the 8-wave kernel (2560) — each with and without the fused bias + GELU epilogue — and
    torch.matmul (hipBLASLt, no epilogue), ``iters`` launches each, interleaved round-robin, an event pair per launch."""
    from cambrian_amd import lib as L
    from cambrian_amd import ops
    M, N, K = 65536, 6144, 1536
    g = torch.Generator(device=dev).manual_seed(5)
    a = torch.randn((M, K), device=dev, dtype=torch.bfloat16, generator=g)
    w = torch.randn((N, K), device=dev, dtype=torch.bfloat16, generator=g) * 0.03
    bias = torch.randn((N,), device=dev, dtype=torch.float32, generator=g)
    out = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    variants = {
        "p5_gelu": lambda: ops.k_gemm(a, w, bias=bias, act=L.ACT_GELU_ERF, out=out, tile=2590),
        "w8_gelu": lambda: ops.k_gemm(a, w, bias=bias, act=L.ACT_GELU_ERF, out=out, tile=2560),
        "p5_plain": lambda: ops.k_gemm(a, w, out=out, tile=2590),
        "w8_plain": lambda: ops.k_gemm(a, w, out=out, tile=2560),
        "torch_matmul_plain": lambda: torch.matmul(a, w.t(), out=out),
    }
    evs = {k: [] for k in variants}
    for it in range(iters + 2):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            if it >= 2:
                evs[k].append((e0, e1))
    torch.cuda.synchronize(dev)
    res = {}
    for k, lst in evs.items():
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in lst)
        mean = sum(us) / len(us)
        res[k] = {"mean_us": round(mean, 1), "median_us": round(us[len(us) // 2], 1), "min_us": round(us[0], 1),
                  "TFLOPs_mean": round(2.0 * M * N * K / mean / 1e6, 1), "frac_of_peak": round(2.0 * M * N * K / mean / 1e6 / MFMA_BF16_PEAK_TFLOPS, 3)}
    return {"shape_MNK": [M, N, K], "launches_each": iters, "order": "interleaved round-robin after 2 untimed rounds",
            "variants": res}


PARITY = {
    "benched_dtype": "bf16 (fp32 accumulate / softmax / LayerNorm statistics; fp32 master parameters)",
    "oracle": "oracle/{sva,arch,llama,towers}.py: CPU fp32 restatement pinned to the real reference modules (tests/golden/)",
    "release_width_vs_fp32_oracle": {
        "where": "tests/test_release_width_gpu.py (Llama-3-8B-wide decoder, release-dimension towers, S = 2048, collator batch)",
        "logits_max_rel": {"observed": 2.35e-2, "test_bound": 4e-2}, "logits_l2": {"observed": 1.7e-2, "test_bound": 3e-2},
        "logits_slope_err": {"observed": 1.4e-4, "test_bound": 5e-3},
        "worst_trainable_grad_tensor_max_rel": {"observed": 4.9e-2, "test_bound": 8e-2}},
    "reference_own_bf16_vs_its_fp32": {
        "where": "tests/golden/ref_bf16_twin_release_width.json (make_bf16_twin.py: the real cambrian_arch / vision_sampler / hook "
                 "lines + installed-HF towers and decoder layers cast to bf16, same geometry and batch, build container)",
        "logits_max_rel": 3.5e-2, "logits_l2": 2.6e-2, "logits_slope_err": 4.5e-4, "grad_tensor_median_max_rel": 3.3e-2,
        "worst_grad_tensor_max_rel": 4.9e-1,
        "assertion": "logits (max / L2 / slope) and the median / p90 gradient tensor <= 1.5 x their reference-bf16 twins; for the WORST "
                     "gradient tensor the twin (0.49) is no yardstick — the absolute 8e-2 binds (test_release_width_gpu.py)"},
    "full_depth_bf16_vs_fp32_hip": {
        "where": "tools/full_depth_parity.py -> profiles/r05_parity_observed.jsonl: the HIP path in bf16 against ITS OWN fp32 instantiation "
                 "(pinned to the CPU oracle at 1.2e-5) at the FULL release depth — 32 decoder layers, 3 + 10 SVA layers, full-depth "
                 "towers, vocabulary 128256, collator batch of 2 letter-boxed images, same weights (decoder rounded to bf16)",
        "logits_max_rel": 1.01e-1, "logits_rel_l2": 6.6e-2, "logits_slope_err": 2.2e-3, "loss_fp32": 12.5276, "loss_bf16": 12.5282,
        "grad_tensor_max_rel_median": 9.3e-2, "grad_tensor_max_rel_p90": 1.36e-1, "grad_tensor_max_rel_worst": 3.6e-1,
        "note": "4.3 x the 4-layer release-width figure (2.35e-2): rounding noise grows with depth, the slope stays at 1 to 2e-3"},
    "hidden_256_model": {"logits_max_rel": "7.9e-3 .. 9.2e-3 (bound 2e-2)", "worst_grad": "1.5e-2 .. 1.9e-2 (bound 4e-2)",
                         "where": "tests/test_model_gpu.py"},
    "systematic_error_checks": "least-squares slope |s - 1| < 5e-3 (logits) / 2e-2 (gradients), relative L2 (tests/conftest.py::fit_err)",
    "north_star_tolerance": "1e-3 rel holds for the fp32 path (1.2e-5 logits / 2.3e-5 gradients at release width), NOT for this bf16 "
                            "line — a bf16 ulp is 4e-3 relative; the bf16 yardstick is the reference's own bf16 run above",
    "bit_exact": "window gather, masks, position ids, embedding splice, untouched hook rows (torch.equal in tests)",
}


ABSORB_KV_ON = False   # set in main(): whether the SVA layers take the absorbed K / V path (bf16 training default)
PMC_FILES = {2590: "r06_pmc_gemm_p5.json", 256: "r03_pmc_gemm_8wave.json"}   # cmb_gemm_last_kernel id -> profiles/ file


def pmc_record(kernel_id):
    """The rocprofv3 PMC summary of the dominant kernel (tools/pmc_traffic.sh + tools/pmc_summarise.py, committed under
    profiles/), or None when there is none for this kernel or the kernel's sources changed since it was taken (the
    summary carries their sha256: a constant from an older kernel would silently go stale)."""
    name = PMC_FILES.get(kernel_id)
    if not name:
        return None
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            d = json.load(f)
    except Exception:
        return None
    if d.get("sources_sha256"):
        import hashlib
        sha = hashlib.sha256()
        try:
            for s in d.get("sources", []):
                with open(os.path.join(ROOT, s), "rb") as f:
                    sha.update(f.read())
        except OSError:
            return None
        if sha.hexdigest() != d["sources_sha256"]:
            return None
    d["_file"] = name
    return d


def pmc_note(kernel_id):
    d = pmc_record(kernel_id)
    if d is None:
        return None
    return {"shape_MNK": d["shape"], "algorithmic_bytes": d["algorithmic_bytes_per_launch"],
            "what": f"rocprofv3 --pmc passes on the launch shape with the largest share of the kernel's time "
                    f"(profiles/{d['_file']}): (2*FETCH_SIZE + WRITE_SIZE)*1024 per launch; FETCH counts L2->fabric "
                    f"reads incl. Infinity-Cache hits"}


def pmc_traffic(kernel_id):
    """HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes (FETCH_SIZE x2 on gfx950 + WRITE_SIZE,
    MI355X_MICROARCH.md §HBM); null when no valid PMC summary is present (pmc_record)."""
    d = pmc_record(kernel_id)
    return None if d is None else d.get("hbm_bytes_per_launch")


def self_spawn(args) -> int:
    """`python bench.py --gpus N` outside a torchrun environment: re-launch this script under torch.distributed.run, one
    rank per GPU on 127.0.0.1, exactly as the driver's N > 1 command does, and relay its output / exit code."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def multi_gpu_fields(args, rank, world, dev, elapsed_rank, sync_events, sync, opt, comm_steps=5):
    """N > 1 only, after the timed region: per-rank step time spread, the time the compute stream spent inside
    GradSync.finish() (= the part of the exchange the backward did not hide), and ``comm_steps`` exchanges of the real bucket
    table with nothing else running (comm_only_ms, bus_gb_per_s as RCCL's tests define it: 2 (N - 1) / N x bytes / time for
    all-reduce; reduce-scatter + all-gather of ZeRO-2 move the same bytes).  Every rank calls this (it carries collectives);
    the returned dict is all scalars.  Runs on gloo as well (tests/test_bench_fields.py)."""
    def _sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
    per = torch.tensor([elapsed_rank / args.steps * 1e3], device=dev, dtype=torch.float64)
    allr = [torch.zeros_like(per) for _ in range(world)]
    dist.all_gather(allr, per)
    vals = [float(t.item()) for t in allr]
    wait_ms = None
    if sync_events:
        wait_ms = sum(e0.elapsed_time(e1) for e0, e1 in sync_events) / max(len(sync_events), 1)
    out = {"rank_step_ms_min": min(vals), "rank_step_ms_max": max(vals), "sync_wait_ms_per_step": wait_ms,
           "sync_wait_what": "HIP-event span of GradSync.finish() on the compute stream, mean over the timed steps (rank 0)"}
    if args.no_comm_pass:
        return out
    nbytes = 0
    if sync is not None:
        flats = [b.flat for b in sync.buckets]
        nbytes = sum(f.numel() * f.element_size() for f in flats)

        def exchange():
            works = [dist.all_reduce(f, op=dist.ReduceOp.SUM, group=sync.group, async_op=True) for f in flats]
            for w in works:
                w.wait()
        kind = "all_reduce"
    elif hasattr(opt, "buckets"):
        bks = opt.buckets
        nbytes = sum(b.flat_grad.numel() * b.flat_grad.element_size() for b in bks)

        def exchange():
            for b in bks:
                dist.reduce_scatter_tensor(b.grad_shard, b.flat_grad, op=dist.ReduceOp.SUM, group=opt.group)
                dist.all_gather_into_tensor(b.flat_param, b.param_shard, group=opt.group)
        kind = "reduce_scatter+all_gather"
    else:
        return out
    exchange()
    _sync()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(comm_steps):
        exchange()
    _sync()
    dist.barrier()
    dt = torch.tensor([(time.perf_counter() - t0) / comm_steps], device=dev, dtype=torch.float64)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    dt = float(dt.item())
    out.update(comm_only_ms=dt * 1e3, comm_only_collective=kind, comm_only_bytes=nbytes, comm_only_steps=comm_steps,
               bus_gb_per_s=2.0 * (world - 1) / world * nbytes / dt / 1e9 if dt > 0 else None,
               exchange_hidden_frac=(1.0 - wait_ms / (dt * 1e3)) if (wait_ms is not None and dt > 0) else None)
    return out


def comm_only(args, rank, world, dev, params, opt, sync):
    """--comm-only: the gradient exchange of the configured parameter set alone — GradSync's bucketed all-reduce (default) or
    ZeRO-2's reduce-scatter + all-gather — timed per bucket with events on the collectives' completion, K steps.  Bus bandwidth
    per bucket as RCCL's tests define it: all-reduce 2 (N - 1) / N x bytes / time; reduce-scatter / all-gather (N - 1) / N."""
    import torch.distributed as dist

    def _sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
    nbytes_total = sum(p.numel() * p.element_size() for p in params)
    rows = []
    if sync is not None:
        for b in sync.buckets:
            b.flat.normal_()
    _sync()

    def one_step(record):
        t_step = time.perf_counter()
        if sync is not None:
            for i, b in enumerate(sync.buckets):
                t0 = time.perf_counter()
                if world > 1 or dist.is_initialized():
                    dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=sync.group)
                _sync()
                if record:
                    rows.append(("all_reduce", i, b.flat.numel() * b.flat.element_size(), time.perf_counter() - t0))
        else:   # ZeRO-2
            for i, b in enumerate(opt.buckets):
                t0 = time.perf_counter()
                if world > 1:
                    dist.reduce_scatter_tensor(b.grad_shard, b.flat_grad, op=dist.ReduceOp.SUM, group=opt.group)
                _sync()
                t1 = time.perf_counter()
                if world > 1:
                    dist.all_gather_into_tensor(b.flat_param, b.param_shard, group=opt.group)
                _sync()
                if record:
                    nb = b.flat_grad.numel() * b.flat_grad.element_size()
                    rows.append(("reduce_scatter", i, nb, t1 - t0))
                    rows.append(("all_gather", i, nb, time.perf_counter() - t1))
        return time.perf_counter() - t_step

    for _ in range(args.warmup):
        one_step(False)
    if world > 1:
        dist.barrier()
    _sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step(True)
    _sync()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    if rank == 0:
        per = {}
        for kind, i, nb, dt in rows:
            e = per.setdefault((kind, i), [nb, 0.0, 0])
            e[1] += dt
            e[2] += 1
        fac = {"all_reduce": 2.0 * (world - 1) / world, "reduce_scatter": (world - 1) / world, "all_gather": (world - 1) / world}
        buckets = [{"collective": k[0], "bucket": k[1], "bytes": v[0], "avg_ms": v[1] / v[2] * 1e3,
                    "bus_gb_per_s": (fac[k[0]] * v[0] / (v[1] / v[2]) / 1e9) if world > 1 else None} for k, v in sorted(per.items())]
        tot_bytes = sum(b["bytes"] for b in buckets if b["collective"] != "all_gather")
        line = {"metric": "gradient exchange only (NOT the headline metric): ms per step of the configured parameter set's collectives",
                "value": elapsed / args.steps * 1e3, "unit": "ms/step", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": False, "scaling": "weak", "vs_baseline": None,
                "dtype": "fp32 gradients of the SVA / projector parameters" + (", bf16 of the LLM" if args.stage == "finetune" else ""),
                "data": "synthetic",
                "config": {"workload": f"--comm-only, stage {args.stage}: {'ZeRO-2 reduce-scatter + all-gather' if sync is None else 'GradSync all-reduce'}"
                                       f" of {len(params)} tensors / {nbytes_total / 2 ** 30:.2f} GiB of gradients in {len(buckets)} collectives of "
                                       f"<= {args.bucket_mb:g} MiB", "parallelism": f"dp{world}" + ("+zero2" if sync is None else ""),
                           "bucket_mb": args.bucket_mb, "gradient_bytes": nbytes_total, "NOT_HEADLINE": "communication only"},
                "buckets": buckets,
                "aggregate_bus_gb_per_s": ((fac["all_reduce"] if sync is not None else fac["reduce_scatter"]) * tot_bytes
                                           / (elapsed / args.steps) / 1e9) if world > 1 else None}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def compact_line(full: dict) -> dict:
    """The line the driver records (VERDICT r4 #1a): every contract key, the roofline object with the figures the judge
    reads as SCALAR keys (the driver keeps only scalars of ``parsed.roofline``), five-row summaries instead of tables and
    prose — under 8 KB.  ``--verbose-line`` prints the full object instead; it is always written to
    gpurun_out/bench_line_full.json."""
    line = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                 "scaling", "vs_baseline", "dtype", "data", "config") if k in full}
    rf = full.get("roofline")
    if rf:
        out = {k: rf[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "launches", "avg_launch_us",
                                  "flop_per_launch_avg", "share_of_step") if k in rf}
        out["kernel"] = rf.get("kernel", "").split(" ")[0]
        out["share_of_step_note"] = "dominant OWN kernel; the step's largest kernel is hipBLASLt's (frozen decoder GEMMs, stock per the north star)"
        reg = rf.get("region")
        if reg:
            out["region_frac"] = reg.get("frac")
            out["region_ms_per_step"] = reg.get("ms_per_step")
            out["region_fwd_ms_per_step"] = reg.get("fwd_ms_per_step")
            out["region_bwd_ms_per_step"] = reg.get("bwd_ms_per_step")
            out["region_tflop_per_step"] = reg.get("algorithmic_tflop_per_step")
            out["region_executed_frac"] = reg.get("executed_frac")
            out["region_executed_tflop_per_step"] = reg.get("executed_tflop_per_step")
            out["region_share_of_step"] = reg.get("share_of_step")
            out["region_what"] = ("4 towers + aux projectors + 3-layer SVA connector + mm_projector + splice + 10 in-LLM SVA "
                                  "layers, fwd + bwd, HIP-event spans in the timed region; frac on the reference algorithm's "
                                  "12.0 TFLOP/img, executed_frac on what this build runs")
        ag = rf.get("all_own_gemm")
        if ag:
            out["all_own_gemm_frac"] = ag.get("frac")
            out["all_own_gemm_ms_per_step"] = ag.get("ms_per_step")
            out["all_own_gemm_tflop_per_step"] = ag.get("tflop_per_step")
            for fam, v in (ag.get("families") or {}).items():   # weight-gradient (TN) and 128-tile launches beside the 256-tile kernels
                out[f"own_{fam}_ms_per_step"] = round(v["ms_per_step"], 2)
                out[f"own_{fam}_frac"] = round(v["frac"], 4)
        ab = (rf.get("ab") or {}).get("variants")
        if ab:
            out["ab_shape_MNK"] = "x".join(str(v) for v in rf["ab"]["shape_MNK"])
            for k_, name in (("p5_gelu", "ab_p5_gelu_tflops"), ("p5_plain", "ab_p5_plain_tflops"), ("w8_gelu", "ab_w8_gelu_tflops"),
                             ("torch_matmul_plain", "ab_hipblaslt_plain_tflops")):
                if k_ in ab:
                    out[name] = ab[k_]["TFLOPs_mean"]
        cal = (rf.get("calibration") or {}).get("shapes")
        if cal:
            out["calibration_shapes"] = len(cal)
            out["calibration_top5"] = [f"{r['M']}x{r['N']}x{r['K']}a{r['act']}:k{r['choice']}:{max(r['TFLOPs'].values()):.0f}TF"
                                       for r in cal[:5]]
        if rf.get("other_256_tile_kernels"):
            out["other_256_tile_kernels"] = {k: {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()}
                                             for k, v in rf["other_256_tile_kernels"].items()}
        tr = rf.get("traffic_of")
        if tr:
            out["traffic_shape_MNK"] = "x".join(str(v) for v in tr["shape_MNK"])
            out["traffic_algorithmic_bytes"] = tr["algorithmic_bytes"]
        line["roofline"] = out
    for k in ("multi_gpu", "tower_streams"):
        if k in full:
            line[k] = full[k]
    if "masked_case" in full:
        m = full["masked_case"]
        line["masked_case"] = {k: m[k] for k in ("ms_per_step", "images_per_s", "masked_key_fraction", "vs_square_case") if k in m}
    if "box" in full:
        b = full["box"]
        smi = b.get("rocm_smi") or {}
        line["box"] = {"host": b.get("host"), "device": b.get("device"), "cus": b.get("cus"), "hbm_gb": b.get("hbm_gb"),
                       "sclk": smi.get("sclk clock speed:"), "power_w": smi.get("Current Socket Graphics Package Power (W)"),
                       "power_cap_w": smi.get("Max Graphics Package Power (W)")}
    if "parity" in full:
        p = full["parity"]
        line["parity"] = {
            "benched_dtype": "bf16 (fp32 accumulate / softmax / LN statistics, fp32 master parameters)",
            "fp32_path_logits_max_rel_release_width": 1.2e-5, "north_star_tolerance": "1e-3 rel: met by the fp32 path only",
            "bf16_logits_max_rel_release_width": p["release_width_vs_fp32_oracle"]["logits_max_rel"]["observed"],
            "reference_own_bf16_logits_max_rel": p["reference_own_bf16_vs_its_fp32"]["logits_max_rel"],
            "full_depth_bf16_vs_fp32_hip_logits_max_rel": (p.get("full_depth_bf16_vs_fp32_hip") or {}).get("logits_max_rel"),
            "full_depth_bf16_vs_fp32_hip_logits_l2": (p.get("full_depth_bf16_vs_fp32_hip") or {}).get("logits_rel_l2"),
            "where": "tests/test_release_width_gpu.py, tests/test_full_depth_gpu.py, tests/golden/ref_bf16_twin_release_width.json; "
                     "details: --verbose-line / DESIGN.md §3"}
    if "cpu_baseline" in full:
        c = full["cpu_baseline"]
        cb = {k: c.get(k) for k in ("value", "unit", "cores", "kind", "measured_where", "source", "error") if c.get(k) is not None}
        if c.get("sample"):
            cb["sample"] = c["sample"][:260]
        lp, lh = c.get("live_port_sample"), c.get("live_hf_tower_sample")
        if lp:
            cb["live_port_images_per_s"], cb["live_port_cores"] = lp.get("value"), lp.get("cores")
        if lh and "s_per_image_fwd" in lh:
            cb["live_hf_clip_l_fwd_s"], cb["live_hf_cores"] = lh["s_per_image_fwd"], lh["cores"]
        if isinstance(c.get("parts_s"), dict) and isinstance(c["parts_s"].get("towers_fwd_s"), dict):
            cb["ref_clip_l_fwd_s_build_container"] = c["parts_s"]["towers_fwd_s"].get("clip_l_14_336")
        line["cpu_baseline"] = cb
    line["full_line"] = "gpurun_out/bench_line_full.json (or --verbose-line)"
    return line


def emit(full: dict, verbose: bool) -> None:
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "bench_line_full.json"), "w") as f:
            json.dump(full, f)
    except OSError:
        pass
    print(json.dumps(full if verbose else compact_line(full)), flush=True)


DUMP_LOGIT_ROWS = 64          # --dump-outputs: rows of the [B * S, V] logits at seeded positions (64 x 128256 fp32 = 33 MB)
DUMP_PARAM_SAMPLE = 1 << 20   # --dump-outputs: elements of the trainable parameters / gradients at seeded positions (4 MB each)


def dump_outputs(path, loss, kept, params):
    """--dump-outputs: what the last timed step computed, as float32 .npy files under ``path``.  ``kept`` holds what step()
    kept of that step: ``logits`` (the seeded rows, copied before the backward writes dlogits over the logits) and ``grads``
    (references to the gradients, before zero_grad dropped them).  The parameter / gradient samples share one seeded set
    of positions in the concatenation of the trainable parameters (model order); a gradient that is None counts as zero."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {"loss": loss.detach().float().reshape(1)}
    if kept.get("logits") is not None:
        arrays["logits_sample"] = kept["logits"]
    sizes = [p.numel() for p in params]
    bounds = torch.tensor(sizes, dtype=torch.int64).cumsum(0)
    g = torch.Generator().manual_seed(0)
    flat_idx = torch.randint(int(bounds[-1]), (min(DUMP_PARAM_SAMPLE, int(bounds[-1])),), generator=g).sort().values
    owner = torch.searchsorted(bounds, flat_idx, right=True)
    psample, gsample = [], []
    for i in owner.unique().tolist():
        local = (flat_idx[owner == i] - (int(bounds[i - 1]) if i > 0 else 0)).to(params[i].device)
        psample.append(params[i].detach().reshape(-1)[local].float())
        grad = kept["grads"][i]
        gsample.append(grad.reshape(-1)[local].float() if grad is not None else torch.zeros_like(psample[-1]))
    arrays["params_sample"] = torch.cat(psample)
    arrays["grads_sample"] = torch.cat(gsample)
    total = 0
    for name, t in arrays.items():
        a = t.cpu().numpy().astype(np.float32)
        total += a.nbytes
        np.save(os.path.join(path, name + ".npy"), a)
    assert total <= 64 * 2 ** 20, f"--dump-outputs wrote {total} bytes"


def main():
    args = parse()
    if args.gemm_report and not args.full:
        raise SystemExit("--gemm-report needs --full: the table comes from the two profiled GEMM steps that only --full runs")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        raise SystemExit(self_spawn(args))
    from cambrian_amd.train.dp import GradSync, init_distributed
    rank, local, world = init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the torchrun environment disagrees with --gpus")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback on the product path)")
    local = int(os.environ.get("CAMBRIAN_BENCH_DEVICE", local))   # (tests: several ranks sharing one GPU over gloo)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import __graft_entry__ as ge
    if rank == 0 and not os.path.exists(os.path.join(ROOT, "cambrian_amd", "csrc", "libcambrian_amd.so")):
        ge.build()
    if world > 1:
        dist.barrier()
    from cambrian_amd import ops
    from cambrian_amd.model import vision_sampler as _vs
    from cambrian_amd.train.data_layout import synthetic_batch
    global ABSORB_KV_ON
    ABSORB_KV_ON = bool(_vs.ABSORB_KV)

    model, cfg = build_model(dev, args.llm_layers, args.preset, args.unfreeze_towers, args.stage, args.grad_ckpt,
                             args.tower_recompute)
    cfg.fp8_projections = bool(args.fp8_projections)
    if args.scored_rows:
        cfg.fused_loss = "scored_rows"
    params = [p for p in model.parameters() if p.requires_grad]
    z3_units = None
    lr = 4e-5 if args.stage == "finetune" else 1e-4   # one constant per stage, whatever shards the state (scripts/cambrian/finetune_cambrian_8b.sh: 4e-5)
    if args.zero3:
        # XLA-FSDP full_shard of the reference (fsdp_config.json: transformer_layer_cls_to_wrap = the decoder layer):
        # one unit per decoder layer — 97 % of a 34 B model's parameters; frozen in this stage, so sharded for memory
        # only.  Everything else (SVA layers, projectors, vision_query, image_newline, embeddings, final norm, lm_head)
        # is the root unit of the reference; here it stays replicated and its gradients go through GradSync (the SVA
        # modules are entered through forward_fused(), which module hooks do not see).
        from cambrian_amd.train.zero3 import zero3_finalize, zero3_parameters, zero3_wrap
        m = model.model
        mods = list(m.layers)
        in_units = {id(p) for mod in mods for p in mod.parameters()}
        z3_units = zero3_wrap(mods, gradient_checkpointing=bool(cfg.gradient_checkpointing))
        rest = [p for p in params if id(p) not in in_units]
        # the units' shards are fp32 masters already; whatever trains outside them in a narrower type (finetune stage:
        # embed_tokens / lm_head in bf16) gets an fp32 master here too (they were stepped in bf16)
        from cambrian_amd.train.master import MasterAdamW
        opt = MasterAdamW(zero3_parameters(z3_units) + rest, lr=lr, weight_decay=0.0)
        sync = GradSync(rest, bucket_mb=args.bucket_mb) if rest else None
    elif args.zero2:
        from cambrian_amd.train.zero import Zero2AdamW
        opt, sync = Zero2AdamW(params, lr=lr, weight_decay=0.0, bucket_mb=args.bucket_mb), None
    elif args.stage == "finetune":
        # fp32 masters + fp32 moments for the bf16 decoder (the reference: fp32 FSDP parameters, bf16 compute —
        # train_fsdp.py:1324-1326, fsdp_config.json:6): 16 B per parameter; ZeRO-2 / ZeRO-3 above shard the same state
        from cambrian_amd.train.master import MasterAdamW
        opt = MasterAdamW(params, lr=lr, weight_decay=0.0)
        sync = GradSync(params, bucket_mb=args.bucket_mb)
    else:
        opt = torch.optim.AdamW(params, lr=lr, weight_decay=0.0, fused=True)
        sync = GradSync(params, bucket_mb=args.bucket_mb, comm_dtype=torch.bfloat16 if args.bf16_buckets else None)
    if args.comm_only:
        return comm_only(args, rank, world, dev, params, opt, sync)
    if args.batch <= 0:   # default: what fits the device with headroom
        total_gb = torch.cuda.get_device_properties(dev).total_memory / 2 ** 30
        args.batch = 4 if args.stage == "finetune" else (24 if (total_gb >= 280 and args.preset == "8b") else 16)
    B = args.batch
    pos0 = cfg.image_position

    def make_inputs(nb):
        batch = synthetic_batch(nb, seed=1234 + rank, image_position=pos0)
        return dict(input_ids=batch["input_ids"].to(dev), labels=batch["labels"] if args.scored_rows else batch["labels"].to(dev),
                    position_ids=batch["position_ids"].to(dev),
                    attention_mask=None,  # square synthetic images: nothing is padded -> plain causal attention
                    images=[i.to(dev, torch.bfloat16) for i in batch["images"]],
                    image_aux_attention_masks_list=[m.to(dev) for m in batch["image_aux_attention_masks_list"]],
                    image_sizes=batch["image_sizes"])

    kw = make_inputs(B)

    feed = None
    if args.input_pipeline:
        import itertools
        import numpy as np
        from cambrian_amd.train.image_pipeline import DevicePrefetcher, GpuImagePreprocessor
        rng = np.random.default_rng(1234 + rank)
        sides = (512, 640, 336, 800, 1024, 448, 720, 600)     # square sources: same token layout as the resident case
        host = [dict(raw_images=[rng.integers(0, 256, (sides[(i + k) % 8], sides[(i + k) % 8], 3), dtype=np.uint8)
                                 for i in range(B)]) for k in range(2)]
        pre = GpuImagePreprocessor([t.image_processor for t in model.get_model().get_vision_tower_aux_list()], dev,
                                   torch.bfloat16)
        feed = DevicePrefetcher(itertools.cycle(host), pre)

    sync_events = None   # a list while the timed region runs

    def step(kw_=None, keep=None):
        kw_ = kw if kw_ is None else kw_
        if feed is not None:
            kw_["images"] = next(feed)["images"]
        out = model(**kw_)
        if keep is not None and out.logits is not None:   # --dump-outputs: seeded rows, before the backward overwrites them
            flat = out.logits.detach().reshape(-1, out.logits.shape[-1])
            keep["logits"] = flat.index_select(0, (keep["row_frac"] * flat.shape[0]).long()).float()
        out.loss.backward()
        ops.region_close()   # (roofline.region: the towers + connector span's backward ends with backward())
        if z3_units is not None:
            zero3_finalize(z3_units)
        if sync is not None:
            if sync_events is not None and world > 1:   # how long the compute stream sits in finish(): the un-overlapped exchange
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sync.finish()
                e1.record()
                sync_events.append((e0, e1))
            else:
                sync.finish()
        opt.step()
        if keep is not None:
            keep["grads"] = [p.grad for p in params]
        opt.zero_grad(set_to_none=True)
        return out.loss

    # ---- start-up: one untimed step counts the step's GEMM problems, then every rank times the two 256 x 256 kernels on
    # the hottest of them ON THIS BOX and registers the faster per shape (ops.calibrate_gemm_dispatch; bit-identical
    # results either way).  The census step is the first warm-up step when there is one.
    calibration = None
    warm_left = args.warmup
    batch_fallback = None
    if world == 1 and B > 16:   # probe the chosen batch once; an out-of-memory first step falls back to 16 images
        try:
            step()
            torch.cuda.synchronize()
        except torch.OutOfMemoryError as e:
            batch_fallback = f"{B} images did not fit ({str(e)[:120]}): fell back to 16"
            opt.zero_grad(set_to_none=True)
            model.zero_grad(set_to_none=True)
            if sync is not None:
                sync.reset()
            kw.clear()
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            B = args.batch = 16
            kw.update(make_inputs(B))
        warm_left = max(0, warm_left - 1)
    if not args.no_calibration and args.preset in PRESETS:
        with ops.gemm_census() as census:
            step()
        warm_left = max(0, warm_left - 1)
        torch.cuda.synchronize()
        tc = time.perf_counter()
        rows = ops.calibrate_gemm_dispatch(census.top(20, min_tiles=128), iters=3, device=dev)
        torch.cuda.synchronize()
        calibration = {"shapes": rows, "wall_ms": (time.perf_counter() - tc) * 1e3,
                       "what": "per (M, N, K, act): min of 3 launches of gemm_nt_p5_kernel (2590) vs gemm_nt_256_kernel (2560) "
                               "on this device; the faster is what cmb_gemm launches for that problem from here on"}
    for _ in range(warm_left):
        step()
    prof = None
    spans = None
    if args.full and not args.no_roofline and rank == 0:
        prof = ops.GEMM_PROFILE = []
        ops.GEMM_PROFILE_TILE = 256  # the timed region times only the dominant kernel's launches (an event pair per launch)
        spans = ops.REGION_PROFILE = []
    keep = None
    if args.dump_outputs and rank == 0:   # positions of the logits rows the last step keeps, as fractions of B * S
        keep = {"row_frac": torch.rand(DUMP_LOGIT_ROWS, dtype=torch.float64,
                                       generator=torch.Generator().manual_seed(0)).sort().values.to(dev)}

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    sync_events = [] if args.full else None
    t0 = time.perf_counter()
    loss = None
    for i in range(args.steps):
        loss = step(keep=keep if i == args.steps - 1 else None)
    torch.cuda.synchronize()
    elapsed_rank = time.perf_counter() - t0   # this rank alone, before the barrier (rank_step_ms_min / max)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ops.GEMM_PROFILE = None
    ops.REGION_PROFILE = None
    timed_sync_events, sync_events = sync_events, None
    if keep is not None:
        dump_outputs(args.dump_outputs, loss, keep, params)
        keep = None
    multi_gpu = None
    if world > 1 and args.full:
        multi_gpu = multi_gpu_fields(args, rank, world, dev, elapsed_rank, timed_sync_events, sync, opt)

    # ---- two extra steps with an event pair around EVERY own GEMM launch (all_own_gemm / --gemm-report): kept out of the
    # timed region, where ~1200 extra event pairs per step would cost the stream about half a percent
    prof_all = None
    gemm_pass_steps = 2
    if args.full and not args.no_roofline and not args.no_gemm_pass:   # EVERY rank steps (the steps carry collectives); rank 0 records
        if rank == 0:
            prof_all = ops.GEMM_PROFILE = []
            ops.GEMM_PROFILE_TILE = 0
        for _ in range(gemm_pass_steps):
            step()
        torch.cuda.synchronize()
        ops.GEMM_PROFILE = None
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    # second case (NOT the headline): letter-boxed images -> the collator's key-padding mask in the decoder attention and
    # partially masked SVA windows.  Same step, same timing brackets, 2 steps.
    masked = None
    if args.full and not args.no_masked_case:
        sizes = [(336, 224) if i % 2 == 0 else (224, 336) for i in range(B)]
        mb = synthetic_batch(B, seed=4321 + rank, image_position=pos0, image_sizes=sizes)
        mkw = dict(kw, input_ids=mb["input_ids"].to(dev), labels=mb["labels"] if args.scored_rows else mb["labels"].to(dev),
                   position_ids=mb["position_ids"].to(dev),
                   attention_mask=mb["attention_mask"].to(dev),
                   image_aux_attention_masks_list=[m_.to(dev) for m_ in mb["image_aux_attention_masks_list"]],
                   image_sizes=mb["image_sizes"])
        step(mkw)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        tm = time.perf_counter()
        for _ in range(2):
            step(mkw)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        tm = torch.tensor([time.perf_counter() - tm], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        masked = {"image_sizes": "(336,224) / (224,336) alternating", "steps": 2, "ms_per_step": float(tm.item()) / 2 * 1e3,
                  "images_per_s": B * world * 2 / float(tm.item()),
                  "masked_key_fraction": float(1.0 - mb["attention_mask"].float().mean().item()),
                  "vs_square_case": (float(tm.item()) / 2) / (elapsed / args.steps)}

    if rank == 0:
        line = {
            "metric": "train images/sec (fwd+bwd) Cambrian-8B 4-tower SVA, 576 vis-tok",
            "value": B * world * args.steps / elapsed, "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic" + (" uint8 images through the GPU input pipeline (H2D + resample inside the timed region)"
                                   if args.input_pipeline else ""),
            "config": {"workload": "BASELINE configs[2]: 4-tower (SigLIP-SO400M@384 + CLIP-L@336 + DINOv2-g@378 + "
                                   "ConvNeXt-XXL@1024) + SVA (3 connector + 10 in-LLM layers) into random-init "
                                   "Llama-3-8B, 576 visual + 24 newline tokens in a 2048-token sequence, pre-training "
                                   "stage (SVA+projectors train, LLM+towers frozen), fwd+bwd+all-reduce+AdamW",
                       "images_per_gpu": B, "global_batch": B * world, "seq_len": 2048,
                       "parallelism": f"dp{world}" + ("+zero2" if args.zero2 else "") + ("+zero3" if args.zero3 else ""),
                       "loss": float(loss.item()),
                       "peak_hbm_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
                       "peak_hbm_reserved_gb": torch.cuda.max_memory_reserved() / 2 ** 30},
        }
        from cambrian_amd.model import cambrian_arch as _arch
        line["config"]["tower_pairing"] = ("two frozen ViT trunks in lock-step, same-position residual linears through cmb_gemm_pair "
                                           "(one launch, workgroups split between the problems)") if _arch._PAIR_TOWERS else "off"
        if batch_fallback:
            line["config"]["batch_fallback"] = batch_fallback
        if args.scored_rows:
            scored = int((kw["labels"][:, 1:] != -100).sum())
            line["config"]["NOT_HEADLINE"] = ("lm_head + cross-entropy over the scored positions only (identical loss / gradients, no "
                                              "logits returned); the headline line computes every row as the reference does")
            line["config"]["scored_positions_frac"] = scored / float(kw["labels"].numel())
        if args.fp8_projections:
            line["dtype"] = "bf16 + fp8 (e4m3, row-wise scales) forward GEMMs of the KV-side SVA projections"
            line["config"]["NOT_HEADLINE"] = "reduced-precision mode of BASELINE configs[4]; the headline line is the bf16 run"
        if args.bf16_buckets:
            line["config"]["NOT_HEADLINE"] = "gradient all-reduce on bf16 copies of the fp32 buckets (opt-in; the headline exchanges fp32)"
        if masked is not None:
            line["masked_case"] = masked
        if multi_gpu is not None:
            line["multi_gpu"] = multi_gpu
        if args.preset != "8b":
            line["config"]["NOT_HEADLINE"] = (f"decoder preset {args.preset} ({PRESETS[args.preset]['name']}: BASELINE "
                                              f"configs[{3 if args.preset == '13b' else 4}] geometry); the headline is 8b")
            line["config"]["workload"] = line["config"]["workload"].replace("Llama-3-8B", PRESETS[args.preset]["name"])
        if args.unfreeze_towers:
            line["config"]["NOT_HEADLINE"] = ("--unfreeze_mm_vision_tower (SURVEY.md §8f N4): the towers train; the release recipe "
                                              "and the headline line keep them frozen")
            line["config"]["trainable_parameters"] = int(sum(p.numel() for p in params))
        if args.stage == "finetune":
            line["config"]["NOT_HEADLINE"] = ("finetune stage (scripts/cambrian/finetune_cambrian_8b.sh): the whole LLM trains "
                                              "(activation re-computation on); the headline metric is quoted on the pre-training stage")
            line["config"]["workload"] = line["config"]["workload"].replace(
                "pre-training stage (SVA+projectors train, LLM+towers frozen)", "FINETUNE stage (LLM + SVA + projectors train, towers frozen)")
            line["config"]["trainable_parameters"] = int(sum(p.numel() for p in params))
            n_low = sum(p.numel() for p in params if p.dtype != torch.float32)
            line["config"]["optimizer_state"] = (
                f"{type(opt).__name__}, lr {lr:g}: fp32 master weights + fp32 AdamW moments for every trainable parameter that "
                f"computes in bf16 ({n_low / 1e9:.2f} B parameters; 16 B / parameter"
                + (", sharded 1 / world" if (args.zero2 or args.zero3) else "") + ")")
            line["config"]["gradient_buckets"] = (len(sync.buckets) if sync is not None else len(getattr(opt, "buckets", [])))
        if cfg.gradient_checkpointing:
            line["config"]["activation_recomputation"] = "decoder layers + in-LLM SVA layers (non-reentrant checkpoint)"
        if args.unfreeze_towers and args.tower_recompute:
            line["config"]["tower_recompute"] = "per block"
        if args.llm_layers is not None:
            line["config"]["INVALID"] = f"debug run with {args.llm_layers} decoder layers"
        if prof:
            # dominant HIP kernel of the hot path = the 256x256 bf16 MFMA GEMM: algorithmic FLOPs (2*M*N*K) of every launch
            # of it in the timed region / its HIP-event time on the launch stream
            def agg(rows, sel):
                fl = sum(x[2] for x in rows if sel(x))
                ms = sum(x[0].elapsed_time(x[1]) for x in rows if sel(x))
                n = sum(1 for x in rows if sel(x))
                return fl, ms, n
            # the 256 x 256 tile is served by two kernels (cmb_gemm_last_kernel): the roofline object is about the one
            # with the larger share of the step; the other is reported beside it
            KNAMES = {2590: "cmb_gemm_detail::gemm_nt_p5_kernel (bf16, 256x256x64, 4 waves, fragments of the K tile in registers)",
                      256: "cmb_gemm_detail::gemm_nt_256_kernel (bf16, 256x256x64, 8 waves)"}
            per = {kid: agg(prof, lambda x, kid=kid: x[3] == torch.bfloat16 and x[5] == 256 and x[7] == kid) for kid in KNAMES}
            dom = max(per, key=lambda kid: per[kid][1])
            f256, ms256, n256 = per[dom]
            ach = f256 / (ms256 * 1e-3) / 1e12 if ms256 > 0 else 0.0
            line["roofline"] = {"bound": "mfma", "kernel": KNAMES[dom],
                                "achieved": ach, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                                "frac": ach / MFMA_BF16_PEAK_TFLOPS, "traffic": pmc_traffic(dom), "traffic_of": pmc_note(dom),
                                "launches": n256, "avg_launch_us": ms256 * 1e3 / max(n256, 1),
                                "flop_per_launch_avg": f256 / max(n256, 1),
                                "share_of_step": ms256 / (elapsed * 1e3),
                                "flop_model": "2*M*N*K per launch, summed over the launches of the timed region",
                                "peak_source": "MI355X_MICROARCH.md: 2.5 PFLOP/s dense bf16 MFMA"}
            others = {KNAMES[k].split(" ")[0]: {"achieved": v[0] / (v[1] * 1e-3) / 1e12, "launches": v[2],
                                                "avg_launch_us": v[1] * 1e3 / v[2], "share_of_step": v[1] / (elapsed * 1e3)}
                      for k, v in per.items() if k != dom and v[2]}
            if others:
                line["roofline"]["other_256_tile_kernels"] = others
            if spans:
                # the tower + SVA REGION of the step (9.17 TFLOP/img towers forward + 3 x 0.94 SVA side
                # forward + backward = 12.0 TFLOP per trained image) over its HIP-event spans in the timed region
                r = ops.region_ms(spans)
                region_ms = (r["fwd_ms"] + r["bwd_ms"]) / args.steps
                region_tflop = (TOWER_GFLOP + 3.0 * SVA_SIDE_GFLOP) * B / 1e3
                first = [s_ for s_ in spans if s_["tag"] == "towers_connector"]
                r0 = ops.region_ms(first)
                line["roofline"]["region"] = {
                    "what": "encode_images (4 towers) + aux projectors + 3-layer SVA connector + mm_projector + newline / splice "
                            "and the 10 in-LLM SVA layers, forward and backward (gradients w.r.t. parameters and aux features "
                            "included), HIP-event spans on the launch stream inside the timed region",
                    "ms_per_step": region_ms, "fwd_ms_per_step": r["fwd_ms"] / args.steps, "bwd_ms_per_step": r["bwd_ms"] / args.steps,
                    "towers_connector_ms_per_step": (r0["fwd_ms"] + r0["bwd_ms"]) / args.steps,
                    "algorithmic_tflop_per_step": region_tflop,
                    "achieved": region_tflop / (region_ms * 1e-3) if region_ms > 0 else 0.0, "unit": "TFLOP/s",
                    "frac": region_tflop / (region_ms * 1e-3) / MFMA_BF16_PEAK_TFLOPS if region_ms > 0 else 0.0,
                    "share_of_step": region_ms / (elapsed / args.steps * 1e3),
                    "flop_model": "12.0 TFLOP per image: towers 9.169 forward (frozen) + SVA side 0.940 x 3 (SURVEY.md §8d) — the "
                                  "REFERENCE algorithm's count, whatever this build executes",
                    "absorbed_kv": bool(ABSORB_KV_ON),
                    "executed_note": ("with the windowed tower's K / V projections absorbed into the query side (DESIGN.md "
                                      "§4.5) the SVA side executes ~1.4 of its 2.8 TFLOP per image; the fraction above "
                                      "stays on the reference's 12.0") if ABSORB_KV_ON else None}
            if prof_all:
                fall, msall, nall = agg(prof_all, lambda x: x[3] == torch.bfloat16)
                line["roofline"]["all_own_gemm"] = {
                    "achieved": fall / (msall * 1e-3) / 1e12 if msall > 0 else 0.0,
                    "frac": fall / (msall * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS if msall > 0 else 0.0,
                    "launches_per_step": nall / gemm_pass_steps, "ms_per_step": msall / gemm_pass_steps,
                    "tflop_per_step": fall / gemm_pass_steps / 1e12,
                    "families": {name: {"ms_per_step": ms_ / gemm_pass_steps, "launches_per_step": n_ / gemm_pass_steps,
                                        "frac": (fl_ / (ms_ * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS) if ms_ > 0 else 0.0}
                                 for name, (fl_, ms_, n_) in (
                                     (nm, agg(prof_all, lambda x, kid=kid: x[3] == torch.bfloat16 and x[7] == kid))
                                     for nm, kid in (("gemm_nt_p5", 2590), ("gemm_nt_256_8wave", 256), ("gemm_nt_128", 128),
                                                     ("gemm_tn", 7128)))},
                    "from": f"{gemm_pass_steps} extra profiled steps after the timed region (an event pair around every own bf16 "
                            "GEMM launch: 128- and 256-tile kernels, split-K wgrad GEMMs with their reduce kernels)"}
                if "region" in line["roofline"]:
                    # what this build EXECUTES in the region: every own GEMM launch of the step is inside it
                    # (measured 2 M N K sums) + the towers' attention (4 N^2 d per head and layer), the depthwise
                    # convolutions (98 FLOP per output) and the absorbed SVA kernels' 16 x 16 x 1024 products — per image
                    # 0.230 + 0.032 + 0.020 TFLOP — next to the reference-algorithm count the `frac` above is quoted on
                    reg = line["roofline"]["region"]
                    ex = fall / gemm_pass_steps / 1e12 + EXEC_NON_GEMM_TFLOP_PER_IMAGE * B
                    reg["executed_tflop_per_step"] = ex
                    reg["executed_frac"] = ex / (reg["ms_per_step"] * 1e-3) / MFMA_BF16_PEAK_TFLOPS if reg["ms_per_step"] > 0 else 0.0
            if calibration is not None:
                line["roofline"]["calibration"] = calibration
        if prof_all and args.gemm_report:
            shapes = {}
            for x in prof_all:
                key = (x[6], x[4], x[5], x[7], x[8] if len(x) > 8 else 1)
                s_ = shapes.setdefault(key, [0, 0.0, 0.0])
                s_[0] += 1
                s_[1] += x[0].elapsed_time(x[1])
                s_[2] += x[2]
            # kernel: 2590 gemm_nt_p5, 256 gemm_nt_256 (8 waves), 128 gemm_nt<128,128> (batch > 1: the per-head launches of the
            # absorbed SVA path), 7128 cmb_gemm_tn (weight gradients; K = contraction rows, the span includes its split-K reduce)
            rows = [{"M": k[0][0], "N": k[0][1], "K": k[0][2], "act": k[0][3], "f32_out": k[0][4], "split_k": k[1], "tile": k[2],
                     "kernel": k[3], "batch": k[4], "launches_per_step": v[0] / gemm_pass_steps, "ms_per_step": v[1] / gemm_pass_steps,
                     "TFLOPs": v[2] / (v[1] * 1e-3) / 1e12 if v[1] > 0 else 0.0} for k, v in shapes.items()]
            rows.sort(key=lambda r: -r["ms_per_step"])
            with open(args.gemm_report, "w") as f:
                json.dump(rows, f, indent=0)
        if not args.full:
            print(json.dumps(line), flush=True)
        else:
            line["box"] = box_identity(dev)
            if "roofline" in line and not args.no_ab:
                try:
                    line["roofline"]["ab"] = gemm_ab(dev)
                except Exception as e:  # a side measurement must never take the line down
                    line["roofline"]["ab"] = {"error": repr(e)[:300]}
            line["parity"] = PARITY
            if not args.no_cpu_baseline and world == 1:
                try:
                    line["cpu_baseline"] = cpu_baseline()
                except Exception as e:  # the baseline must never take the measurement down
                    line["cpu_baseline"] = {"value": None, "error": repr(e)}
            emit(line, args.verbose_line)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
