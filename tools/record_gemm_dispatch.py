#!/usr/bin/env python3
"""Records which kernel every branch of the GEMM dispatch takes, and the bits it produces (GPU).

    python tools/record_gemm_dispatch.py --commit <hash> --out tests/golden/gemm_dispatch_parent.json

For a fixed list of the smallest problems that still reach each branch of cmb_gemm / cmb_gemm_pair / cmb_gemm_tn
(cambrian_amd/csrc/gemm_plan.h) the operands are generated on the CPU from ``torch.Generator().manual_seed(case index)``,
the public ``ops`` launcher is called, and the case's record is: ``cmb_gemm_last_kernel()``, ``cmb_gemm_pair_last()`` (pair
cases), ``cmb_gemm_tail_rows(M, N)`` and the SHA-256 of the output bytes.  Every case runs twice; a case whose two hashes
differ is recorded with ``"hash": null`` (ids only) and listed on stderr.  The file also carries the device's CU count and the
commit it was recorded at: tests/test_gemm_dispatch_golden_gpu.py replays the list on the tree under test and wants the same
ids and bits, tests/test_gemm_plan_sim.py feeds each case's ``plan`` line to the CPU simulation of gemm_plan.h.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BF, F32 = torch.bfloat16, torch.float32
GELU, SWIGLU = 1, 5   # lib.ACT_GELU_ERF, lib.ACT_SWIGLU_PAIRS


def _plan(M, N, K, **kw):
    """One problem as tests/csrc/gemm_plan_sim.cpp reads it: key=value tokens, everything not named is 0 / plain."""
    return " ".join(f"{k}={v}" for k, v in dict(M=M, N=N, K=K, **kw).items())


def _rand(g, *shape, scale=1.0, dt=BF):
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def _gemm(M, N, K, dt=BF, **opt):
    """A k_gemm case: opt = bias / act / residual / pre_out / ln (folded LayerNorm) / out_f32 / beta / split_k / tile / policy."""
    flags = {k: opt[k] for k in ("act", "split_k", "out_f32", "beta") if opt.get(k)}
    flags.update({k: 1 for k in ("bias", "residual", "pre_out", "ln") if opt.get(k)})
    if opt.get("tile"):
        flags["hint"] = opt["tile"]
    if dt == F32:
        flags["es"] = 4
    if opt.get("policy"):
        flags["pol"] = ",".join(str(v) for v in (M, N, K, opt.get("act", 0), opt["policy"]))

    def make(g, dev):
        kw = dict(a=_rand(g, M, K, dt=dt).to(dev), w=_rand(g, N, K, scale=K ** -0.5, dt=dt).to(dev), act=opt.get("act", 0),
                  split_k=opt.get("split_k", 1), tile=opt.get("tile", 0))
        if opt.get("bias") or opt.get("ln"):
            kw["bias"] = torch.randn(N, generator=g).to(dev)
        if opt.get("residual"):
            kw["residual"] = _rand(g, M, N, dt=dt).to(dev)
        if opt.get("pre_out"):
            kw["pre_out"] = torch.zeros(M, N, dtype=dt, device=dev)
        if opt.get("ln"):
            kw["row_stats"] = (torch.randn(M, generator=g).mul(0.1).to(dev), torch.rand(M, generator=g).add(0.5).to(dev))
            kw["col_sum"] = kw["w"].float().sum(1).contiguous()
        if opt.get("out_f32"):
            kw["out"] = torch.randn(M, N, generator=g).to(dev) if opt.get("beta") else torch.zeros(M, N, device=dev)
            kw["beta"] = float(opt.get("beta", 0))
        return kw

    def run(ops, lib, kw):
        if opt.get("policy"):
            assert lib.cmb_gemm_policy_set(M, N, K, opt.get("act", 0), opt["policy"]) == 0
        try:
            out = ops.k_gemm(**kw)
        finally:
            if opt.get("policy"):
                lib.cmb_gemm_policy_clear()
        return [out] + ([kw["pre_out"]] if opt.get("pre_out") else [])

    return dict(M=M, N=N, plan="gemm " + _plan(M, N, K, **flags), make=make, run=run)


def _rowmap(T):
    """test_tail_split_is_the_same_gemm's row-map cases: A rows gathered from a [nb, T + 7, K] buffer, outer period T."""
    M, N, K = 16896, 4096, 256

    def make(g, dev):
        nb = (M + T - 1) // T
        return dict(buf=_rand(g, nb, T + 7, K).to(dev), w=_rand(g, N, K, scale=0.1).to(dev))

    def run(ops, lib, kw):
        from cambrian_amd import lib as L
        return [ops.k_gemm(kw["buf"].view(-1), kw["w"], M=M, a_map=L.make_map(T, T, (T + 7) * K, 0, K))]

    return dict(M=M, N=N, plan="gemm " + _plan(M, N, K, a_n1=T, a_n2=T, a_s0=(T + 7) * K, a_s1=0, a_s2=K), make=make, run=run)


def _batched(batch, M, N, K, residual=False):
    def make(g, dev):
        kw = dict(a=_rand(g, batch, M, K).to(dev), w=_rand(g, batch, N, K, scale=K ** -0.5).to(dev),
                  out=torch.zeros(batch, M, N, dtype=BF, device=dev))
        if residual:
            kw["residual"] = _rand(g, batch * M, N).to(dev)
        return kw

    def run(ops, lib, kw):
        return [ops.k_gemm_batched(kw["a"], kw["w"], kw["out"], batch=batch, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, a_bs=M * K,
                                   b_bs=N * K, c_bs=M * N, residual=kw.get("residual"))]

    return dict(M=M, N=N, plan="gemm " + _plan(M, N, K, batch=batch, c_bs=M * N, **({"residual": 1} if residual else {})),
                make=make, run=run)


def _fp8(M, N, K):
    def make(g, dev):
        return dict(a=_rand(g, M, K).to(dev), w=_rand(g, N, K, scale=K ** -0.5).to(dev))

    def run(ops, lib, kw):
        (aq, ai), (wq, wi) = ops.k_quantize_fp8_rows(kw["a"]), ops.k_quantize_fp8_rows(kw["w"])
        return [ops.k_gemm_fp8(aq, ai, wq, wi)]

    return dict(M=M, N=N, plan="gemm " + _plan(M, N, K, es=1), make=make, run=run)


def _tn(rows, M, N, split_k, batch=1):
    def make(g, dev):
        kw = dict(at=_rand(g, rows, batch * M).to(dev), bt=_rand(g, rows, batch * N).to(dev))
        if batch > 1:
            kw["out"] = torch.zeros(batch, M, N, device=dev)
        return kw

    def run(ops, lib, kw):
        if batch == 1:
            return [ops.k_gemm_tn(kw["at"], kw["bt"], split_k=split_k)]
        return [ops.k_gemm_tn(kw["at"], kw["bt"], out=kw["out"], split_k=split_k, M=M, N=N, batch=batch, a_bs=M, b_bs=N, c_bs=M * N,
                              ldc=N)]

    return dict(M=M, N=N, plan="tn " + _plan(M, N, rows, split_k=split_k, batch=batch), make=make, run=run)


def _pair(p0, p1, pre_out=False):
    """tests/test_gemm_pair_gpu.py's operands: (M, N, K, colscale) per side, bias on both, a residual where N % 256 == 0."""
    def side(g, dev, M, N, K, cs, res):
        kw = dict(a=_rand(g, M, K).to(dev), w=_rand(g, N, K, scale=K ** -0.5).to(dev), act=0,
                  out=torch.zeros(M, N, device=dev, dtype=BF), bias=torch.randn(N, generator=g).to(dev))
        if cs:
            kw["colscale"] = torch.randn(N, generator=g).to(dev)
        if res:
            kw["residual"] = _rand(g, M, N).to(dev)
        return kw

    def make(g, dev):
        k0, k1 = side(g, dev, *p0, True), side(g, dev, *p1, p1[1] % 256 == 0)
        if pre_out:
            k0["pre_out"] = torch.zeros(p0[0], p0[1], device=dev, dtype=BF)
        return dict(k0=k0, k1=k1)

    def run(ops, lib, kw):
        return list(ops.k_gemm_pair(kw["k0"], kw["k1"]))

    def flags(p, res, pre):
        f = dict(bias=1)
        if p[3]:
            f["colscale"] = 1
        if res:
            f["residual"] = 1
        if pre:
            f["pre_out"] = 1
        return _plan(*p[:3], **f)

    return dict(M=p0[0], N=p0[1], pair=True, make=make, run=run,
                plan="pair " + flags(p0, True, pre_out) + " | " + flags(p1, p1[1] % 256 == 0, False))


EPI = dict(bias=True, act=GELU, residual=True, pre_out=True)
CASES = (
    # default dispatch: 4-wave kernel, half column tile, ragged half tile, K = 64, one round, small, tiny
    [("default_%dx%dx%d" % s, _gemm(*s)) for s in [(32768, 2048, 512), (32768, 1152, 512), (32768, 1160, 512), (32768, 2048, 64),
                                                   (8192, 2048, 512), (1536, 2048, 512), (64, 64, 64)]]
    + [("hint_%d" % t, _gemm(1000, 512, 256, tile=t, **EPI)) for t in (128, 256, 2560, 2561, 2590)]
    + [("policy_2560", _gemm(8192, 2048, 512, policy=2560))]
    + [("tail_plain", _gemm(11680, 1536, 128)),
       ("tail_bias_gelu_res", _gemm(11664, 4352, 128, bias=True, act=GELU, residual=True)),
       ("tail_ln_fold", _gemm(11680, 1536, 128, ln=True)),
       ("tail_rowmap_4096", _rowmap(4096)), ("tail_rowmap_4224", _rowmap(4224))]
    + [("splitk8_f32_beta_tile%d" % t, _gemm(1024, 1024, 4096, split_k=8, out_f32=1, beta=1, tile=t)) for t in (128, 2590)]
    + [("splitk8_k128", _gemm(1024, 1024, 128, split_k=8))]
    + [("small_m", _gemm(16, 1024, 1024)), ("small_m_bias", _gemm(16, 1024, 1024, bias=True))]
    + [("batched_k64", _batched(16, 300, 1024, 64)), ("batched_k128", _batched(16, 300, 1024, 128)),
       ("batched_k64_residual", _batched(16, 300, 1024, 64, residual=True))]
    + [("fp32", _gemm(300, 96, 64, dt=F32)), ("fp8", _fp8(512, 1024, 256))]
    + [("swiglu_%d" % t, _gemm(513, 2048, 192, bias=True, act=SWIGLU, tile=t)) for t in (2590, 2560, 128)]
    + [("tn_split1", _tn(1000, 1024, 512, 1)), ("tn_split4", _tn(1000, 1024, 512, 4)), ("tn_batched_split4", _tn(1000, 64, 128, 4, batch=4))]
    + [("pair_yes", _pair((24 * 730, 1536, 1536, True), (24 * 729, 1152, 1152, False))),
       ("pair_whole_rounds", _pair((65536, 2048, 256, False), (65536, 2048, 256, False))),
       ("pair_tiny", _pair((300, 264, 320, False), (257, 8, 64, False))),
       ("pair_pre_out", _pair((24 * 730, 1536, 1536, True), (24 * 729, 1152, 1152, False), pre_out=True))]
)


def device_cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(index: int, dev) -> dict:
    """Launch case ``index`` once on fresh operands: {"kernel", "pair", "tail_rows", "hash"}."""
    from cambrian_amd import lib as L
    from cambrian_amd import ops
    name, case = CASES[index]
    lib = L.load()
    kw = case["make"](torch.Generator().manual_seed(index), dev)
    outs = case["run"](ops, lib, kw)
    kernel = lib.cmb_gemm_last_kernel()
    pair = lib.cmb_gemm_pair_last() if case.get("pair") else None
    torch.cuda.synchronize(dev)
    h = hashlib.sha256()
    for o in outs:
        h.update(o.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return dict(kernel=kernel, pair=pair, tail_rows=lib.cmb_gemm_tail_rows(case["M"], case["N"]), hash=h.hexdigest())


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, unstable = [], []
    for i, (name, case) in enumerate(CASES):
        first, second = run_case(i, dev), run_case(i, dev)
        ids = {k: first[k] for k in ("kernel", "pair", "tail_rows")}
        if ids != {k: second[k] for k in ids}:
            raise SystemExit(f"{name}: the dispatch itself differs between two runs: {first} / {second}")
        if first["hash"] != second["hash"]:
            unstable.append(name)
            first["hash"] = None
        rows.append(dict(name=name, plan=case["plan"], **first))
        print(name, first, flush=True)
    if unstable:
        print("NOT reproducible (ids only):", unstable, file=sys.stderr)
    with open(args.out, "w") as f:
        json.dump(dict(commit=args.commit, cus=device_cus(), cases=rows), f, indent=1)
        f.write("\n")
    return 0 if len(unstable) <= 2 else 1


if __name__ == "__main__":
    sys.exit(main())
