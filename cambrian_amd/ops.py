"""Host-side operators over the C-ABI kernels.

Two layers:
  * ``k_*``  — thin, stateless launchers (no autograd), one per entry point: validate, allocate the outputs, fill the C
    structs, launch through ``lib.call`` (size / id queries through ``lib.load()``).
  * ``*Fn`` / functional wrappers — ``torch.autograd.Function`` objects that pair each forward launcher
    with its backward launchers, so the reference's modules (cambrian/model/vision_sampler.py,
    cambrian_arch.py) can be re-stated on top of them without touching torch's own math kernels.  They hold the autograd
    bookkeeping only (reshapes, what is saved, early returns) and never call the library themselves.
This module imports nothing from ``model/``; ``vit_ops`` holds the tower-only launchers and re-exports the resample pair.

Compute dtype is the dtype of the activation tensor (bf16 for training, fp32 for the parity path);
parameters stay fp32 masters and are cast per call (the cast is itself ``cmb_cast``).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import lib as L
from .lib import RowMap, GemmDesc, SvaDesc


# ================================================================================================
# raw launchers
# ================================================================================================
def _kstep(dtype: torch.dtype) -> int:
    return 64 if dtype == torch.bfloat16 else 32


def pad_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def k_cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Contiguous cast fp32<->bf16 through cmb_cast (returns x itself if nothing to do)."""
    if x.dtype == dtype and x.is_contiguous():
        return x
    L.require_gpu(x)
    xc = x if x.is_contiguous() else x.contiguous()
    if xc.dtype == dtype:
        return xc
    out = torch.empty(xc.shape, dtype=dtype, device=xc.device)
    L.call("cmb_cast", L.dtype_code(xc.dtype), xc.data_ptr(), L.dtype_code(dtype), out.data_ptr(), xc.numel(), device=xc.device)
    return out


def _param_grad(t: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[torch.Tensor]:
    """A parameter's gradient as it leaves the fp32 accumulators, in the parameter's own dtype."""
    return t if t is None or dtype == torch.float32 else t.to(dtype)


def _gemm_desc(dt: int, M: int, N: int, K: int, a: torch.Tensor, a_map: RowMap, w: torch.Tensor, ldb: int, out: torch.Tensor,
               c_map: RowMap, *, bias=None, colscale=None, residual=None, r_map: Optional[RowMap] = None, pre_out=None,
               act: int = L.ACT_NONE, alpha: float = 1.0, beta: float = 0.0, split_k: int = 1, tile: int = 0, slab_rows: int = 0,
               batch: Optional[Tuple[int, int, int, int]] = None, scales=None, ln=None):
    """The ``cmb_gemm_desc`` of every GEMM launcher (the launchers validate, this fills): operands and row maps, the optional
    bias / colscale / residual (through ``r_map``) / contiguous pre_out, the split-K workspace (``split_k`` slabs of
    ``slab_rows`` x N fp32), ``batch`` = (count, a / b / c element strides), ``scales`` = fp8 (a_inv, w_inv), ``ln`` = folded
    LayerNorm (mean, rstd, col_sum).  Returns (descriptor, workspace): the workspace lives as long as the caller holds it."""
    d = GemmDesc()
    d.dtype, d.out_dtype = dt, L.dtype_code(out.dtype)
    d.M, d.N, d.K = M, N, K
    d.A, d.a_map = a.data_ptr(), a_map
    d.B, d.ldb = w.data_ptr(), ldb
    d.C, d.c_map = out.data_ptr(), c_map
    d.bias, d.colscale = L.ptr(bias), L.ptr(colscale)
    d.residual, d.r_map = L.ptr(residual), (r_map if residual is not None else L.identity_map(0))
    d.pre_out, d.p_map = L.ptr(pre_out), L.identity_map(N if pre_out is not None else 0)
    d.act, d.alpha, d.beta, d.split_k, d.tile_hint = act, alpha, beta, split_k, tile
    ws = None
    if split_k > 1:
        ws = torch.empty((split_k * slab_rows * N,), dtype=torch.float32, device=a.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    else:
        d.workspace, d.workspace_bytes = None, 0
    if batch is not None:
        d.batch, d.a_batch_stride, d.b_batch_stride, d.c_batch_stride = batch
    if scales is not None:
        d.a_scale, d.b_scale = scales[0].data_ptr(), scales[1].data_ptr()
    if ln is not None:
        d.row_mean, d.row_rstd, d.col_sum = (t.data_ptr() for t in ln)
    return d, ws


def _gemm_launch(fn: str, descs, device, what: str, prof=None, row=None) -> None:
    """``cmb_<fn>`` on the descriptors; while ``prof`` is a list (GEMM_PROFILE) the launch is bracketed by HIP events on the
    launch stream (bench.py roofline leg) and one row is appended: (start, end) + ``row(lib)``, read after the launch."""
    lib = L.load()
    e0 = _event() if prof is not None else None
    L.check(getattr(lib, fn)(*[C.byref(d) for d in descs], L.stream_ptr(device)), what)
    if prof is not None:
        prof.append((e0, _event()) + row(lib))


def k_gemm(a: torch.Tensor, w: torch.Tensor, *, M: Optional[int] = None, a_map: Optional[RowMap] = None,
           bias: Optional[torch.Tensor] = None, act: int = L.ACT_NONE, colscale: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, r_map: Optional[RowMap] = None,
           out: Optional[torch.Tensor] = None, c_map: Optional[RowMap] = None, out_dtype: Optional[torch.dtype] = None,
           pre_out: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 0.0,
           split_k: int = 1, tile: int = 0, row_stats: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
           col_sum: Optional[torch.Tensor] = None, _collect: Optional[list] = None) -> torch.Tensor:
    """C[M,N] = epilogue(alpha * A[M,K] @ W[N,K]^T).  ``a`` is [M,K] (row stride a.stride(0)) unless an
    explicit ``a_map``/``M`` is given, in which case ``a`` is just the base tensor.  ``row_stats`` = (mean, rstd) [M] fp32
    of ``k_row_stats`` + ``col_sum`` [N]: the LayerNorm in front of this linear folded into its epilogue
    (cmb_gemm_desc.row_mean; ``w`` = W diag(gamma), ``bias`` = b + W beta, ``col_sum`` = rowsum of ``w`` as stored)."""
    L.require_gpu(a, w, bias, colscale, residual, out, pre_out)
    dt = a.dtype
    if w.dtype != dt:
        raise L.CambrianAmdError(f"gemm operand dtypes differ: {dt} vs {w.dtype}")
    N, K = w.shape
    if w.stride(1) != 1:
        raise L.CambrianAmdError("gemm weight must be K-contiguous")
    if a_map is None:
        if a.dim() != 2 or a.stride(1) != 1 or a.shape[1] != K:
            raise L.CambrianAmdError(f"gemm A must be [M,{K}] K-contiguous, got {tuple(a.shape)}")
        M = a.shape[0]
        a_map = L.identity_map(a.stride(0))
    assert M is not None
    odt = out_dtype or (out.dtype if out is not None else dt)
    n_out = N // 2 if act == L.ACT_SWIGLU_PAIRS else N   # gated epilogue: (gate, up) column pairs -> N / 2 outputs
    if out is None:
        out = torch.empty((M, n_out), dtype=odt, device=a.device)
        c_map = L.identity_map(n_out)
    elif c_map is None:
        if out.dim() != 2 or out.stride(1) != 1:
            raise L.CambrianAmdError("gemm out must be 2-D row-major unless c_map is given")
        c_map = L.identity_map(out.stride(0))
    for t in (bias, colscale):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != N):
            raise L.CambrianAmdError("bias / colscale must be contiguous fp32 [N]")
    if residual is not None:
        if residual.dtype != dt:
            raise L.CambrianAmdError("residual dtype must equal the operand dtype")
        if r_map is None:
            if residual.dim() != 2 or residual.stride(1) != 1:
                raise L.CambrianAmdError("residual must be 2-D row-major unless r_map is given")
            r_map = L.identity_map(residual.stride(0))
    if pre_out is not None and (pre_out.dtype != dt or not pre_out.is_contiguous()):
        raise L.CambrianAmdError("pre_out must be contiguous and of the operand dtype")
    ln = None
    if row_stats is not None:
        mean, rstd = row_stats
        L.require_gpu(mean, rstd, col_sum)
        if (col_sum is None or bias is None or any(t.dtype != torch.float32 or not t.is_contiguous() for t in (mean, rstd, col_sum))
                or mean.numel() != M or rstd.numel() != M or col_sum.numel() != N):
            raise L.CambrianAmdError("folded LayerNorm: mean / rstd fp32 [M], col_sum fp32 [N] and a bias are required")
        ln = (mean, rstd, col_sum)
    d, ws = _gemm_desc(L.dtype_code(dt), M, N, K, a, a_map, w, w.stride(0), out, c_map, bias=bias, colscale=colscale,
                       residual=residual, r_map=r_map, pre_out=pre_out, act=act, alpha=alpha, beta=beta, split_k=split_k, tile=tile,
                       slab_rows=M, ln=ln)
    if GEMM_CENSUS is not None and dt == torch.bfloat16 and split_k <= 1 and tile == 0:
        key = (M, N, K, act, pre_out is not None)
        GEMM_CENSUS[key] = GEMM_CENSUS.get(key, 0) + 1
    if _collect is not None:   # k_gemm_pair: the descriptor (and what it points into) instead of the launch
        _collect.append((d, out, (a, w, bias, colscale, residual, pre_out, ws, row_stats, col_sum), (M, N, K, act, dt, split_k, tile)))
        return out
    prof = GEMM_PROFILE
    tile_used = 0
    if prof is not None:
        tile_used = L.load().cmb_gemm_tile(d.dtype, M, N, split_k, tile)
        if GEMM_PROFILE_TILE and tile_used != GEMM_PROFILE_TILE:
            prof = None  # only the dominant kernel is timed: every event pair costs the stream a barrier packet
    _gemm_launch("cmb_gemm", (d,), a.device, f"cmb_gemm(M={M},N={N},K={K},{dt})", prof,
                 lambda lib: (2.0 * M * N * K, dt, split_k, tile_used, (M, N, K, act, out.dtype == torch.float32),
                              lib.cmb_gemm_last_kernel()))
    return out


def k_gemm_pair(kw0: dict, kw1: dict) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two independent ``k_gemm`` calls (keyword dicts with ``a`` and ``w``) through ``cmb_gemm_pair``: ONE launch of the
    persistent 256 x 256 kernel with the workgroups split between the problems when the library's round arithmetic says it pays
    (DINOv2's and SigLIP's same-position linears), else the two launches; the results are bit-identical either way."""
    col: list = []
    k_gemm(_collect=col, **kw0)
    k_gemm(_collect=col, **kw1)
    (d0, o0, _k0, m0), (d1, o1, _k1, m1) = col
    # one profile row for the call: the FLOPs of both problems over the span of the launch (or of the two launches)
    _gemm_launch("cmb_gemm_pair", (d0, d1), o0.device, f"cmb_gemm_pair({m0[:3]}, {m1[:3]})", GEMM_PROFILE,
                 lambda lib: (2.0 * (m0[0] * m0[1] * m0[2] + m1[0] * m1[1] * m1[2]), m0[4], 1, 256,
                              (m0[0], m0[1], m0[2], m0[3], False), lib.cmb_gemm_last_kernel(),
                              ("pair:" if lib.cmb_gemm_pair_last() else "seq:") + f"{m1[0]}x{m1[1]}x{m1[2]}"))
    return o0, o1


def k_quantize_fp8_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [rows, K] (bf16 / fp32, K-contiguous) -> (uint8 e4m3fn bytes [rows, K], fp32 dequantisation factor [rows]):
    each row scaled so that its largest magnitude maps to 448 (cmb_quantize_fp8_rows)."""
    L.require_gpu(x)
    if x.dim() != 2 or x.stride(1) != 1:
        raise L.CambrianAmdError("fp8 quantisation needs a 2-D K-contiguous tensor")
    rows, K = x.shape
    q = torch.empty((rows, K), dtype=torch.uint8, device=x.device)
    inv = torch.empty((rows,), dtype=torch.float32, device=x.device)
    L.call("cmb_quantize_fp8_rows", L.dtype_code(x.dtype), x.data_ptr(), x.stride(0), rows, K, q.data_ptr(), K, inv.data_ptr(),
           device=x.device, what=f"cmb_quantize_fp8_rows({rows}x{K})")
    return q, inv


def k_gemm_fp8(a_q: torch.Tensor, a_inv: torch.Tensor, w_q: torch.Tensor, w_inv: torch.Tensor, *,
               bias: Optional[torch.Tensor] = None, act: int = L.ACT_NONE, colscale: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, r_map: Optional[RowMap] = None,
               pre_out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """C[M,N] = epilogue(a_inv[m] * w_inv[n] * (A_q[M,K] . W_q[N,K]^T)) on v_mfma_f32_32x32x64_f8f6f4; operands are the
    e4m3fn bytes / factors of k_quantize_fp8_rows; residual / pre_out are bf16; C is bf16 or fp32."""
    L.require_gpu(a_q, a_inv, w_q, w_inv, bias, colscale, residual, pre_out)
    M, K = a_q.shape
    N = w_q.shape[0]
    if a_q.dtype != torch.uint8 or w_q.dtype != torch.uint8 or w_q.shape[1] != K or not (a_q.is_contiguous() and w_q.is_contiguous()):
        raise L.CambrianAmdError("fp8 gemm operands must be contiguous uint8 [M,K] / [N,K]")
    out = torch.empty((M, N), dtype=out_dtype, device=a_q.device)
    if residual is not None:
        if residual.dtype != torch.bfloat16:
            raise L.CambrianAmdError("fp8 gemm residual must be bf16")
        r_map = r_map or L.identity_map(residual.stride(0))
    if pre_out is not None and (pre_out.dtype != torch.bfloat16 or not pre_out.is_contiguous()):
        raise L.CambrianAmdError("fp8 gemm pre_out must be contiguous bf16")
    d, _ = _gemm_desc(L.FP8_E4M3, M, N, K, a_q, L.identity_map(K), w_q, K, out, L.identity_map(N), bias=bias, colscale=colscale,
                      residual=residual, r_map=r_map, pre_out=pre_out, act=act, scales=(a_inv, w_inv))
    _gemm_launch("cmb_gemm", (d,), a_q.device, f"cmb_gemm(fp8, M={M},N={N},K={K})")   # (no GEMM_PROFILE row: bf16 / fp32 rooflines only)
    return out


# Forward GEMMs of ops.linear in fp8 (BASELINE configs[4]: "fp8 MFMA projection GEMMs").  The model glue switches it on
# around the SVA-side projections when config.fp8_projections is set; towers and the decoder never see it.
_FP8_LINEAR = False
_FP8_WEIGHT_CACHE: dict = {}


class fp8_projections:
    """Context manager: ``with ops.fp8_projections(True): ...`` — ops.linear(..., heavy=True) quantises x and W row-wise
    to e4m3fn and runs the forward GEMM on the fp8 MFMA; the backward stays bf16 (dX, dW from the saved bf16 operands)."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        global _FP8_LINEAR
        self.prev, _FP8_LINEAR = _FP8_LINEAR, self.on
        return self

    def __exit__(self, *exc):
        global _FP8_LINEAR
        _FP8_LINEAR = self.prev
        return False


def _fp8_weight(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantised copy of a projection weight.  nn.Parameters are cached by identity and re-made when the parameter
    changes (optimizer step => _version bump); anything else (views, weights folded on the fly) is quantised per call —
    a pointer-keyed cache would hand a recycled allocation somebody else's bytes."""
    w2 = weight.detach()
    if w2.stride(1) != 1 or (w2.stride(0) * w2.element_size()) % 16 != 0 or w2.data_ptr() % 16 != 0:
        w2 = w2.contiguous()
    if not isinstance(weight, torch.nn.Parameter):
        return k_quantize_fp8_rows(w2)
    key = id(weight)
    hit = _FP8_WEIGHT_CACHE.get(key)
    if hit is None or hit[0]() is not weight or hit[1] != (weight._version, weight.data_ptr()):
        import weakref
        hit = (weakref.ref(weight, lambda _r, k=key: _FP8_WEIGHT_CACHE.pop(k, None)), (weight._version, weight.data_ptr())) \
            + k_quantize_fp8_rows(w2)
        _FP8_WEIGHT_CACHE[key] = hit
    return hit[2], hit[3]


def fp8_linear_eligible(x: torch.Tensor, weight: torch.Tensor) -> bool:
    return (_FP8_LINEAR and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 128 == 0
            and weight.shape[0] % 8 == 0 and weight.dtype in (torch.bfloat16, torch.float32))


# bench.py sets this to a list to collect (start_event, end_event, flops, dtype, split_k, tile, shape, kernel id) per GEMM launch
GEMM_PROFILE = None
KERNEL_ID_TN = 7128   # the `kernel` field of cmb_gemm_tn launches in GEMM_PROFILE rows (cmb_gemm_last_kernel ids: 128, 256, 2590)
GEMM_PROFILE_TILE = 0  # 0 = time every GEMM launch; 128 / 256 = only launches of that tile configuration
# {(M, N, K, act, has_pre_out): launches} of the bf16 launches that left the kernel choice to the library, while set to a dict
GEMM_CENSUS = None


class gemm_census:
    """``with ops.gemm_census() as c: step()`` — counts the bf16 GEMM problems of one step (no events, no syncs); the
    input of ``calibrate_gemm_dispatch``."""

    def __enter__(self):
        global GEMM_CENSUS
        self.prev, GEMM_CENSUS = GEMM_CENSUS, {}
        self.shapes = GEMM_CENSUS
        return self

    def __exit__(self, *exc):
        global GEMM_CENSUS
        GEMM_CENSUS = self.prev
        return False

    def top(self, n: int = 8, min_tiles: int = 257):
        """The n problems with the most FLOPs per step among those where both 256 x 256 kernels apply: whole tile
        columns, K of at least two 64-deep tiles, no pre-activation copy, at least ``min_tiles`` tiles (257 = more than one
        round of the 256 CUs: where the library's own default is the 4-wave kernel; lower values also put single-round
        problems — the 8-wave kernel's by default — to the test)."""
        rows = []
        for (M, N, K, act, pre), cnt in self.shapes.items():
            tiles = ((M + 255) // 256) * ((N + 255) // 256)
            if pre or N % 128 or K < 128 or K % 64 or tiles < min_tiles:
                continue
            if L.load().cmb_gemm_tail_rows(M, N):
                continue   # launched as 256-tile head + 128-tile tail (gemm_plan.h "tail split"): the policy does not apply
            rows.append((2.0 * M * N * K * cnt, (M, N, K, act)))
        rows.sort(reverse=True)
        return [r[1] for r in rows[:n]]


def calibrate_gemm_dispatch(shapes, iters: int = 3, device=None, candidates=(2590, 2560)):
    """Start-up calibration of the 256 x 256 kernel choice on THIS device (VERDICT r2 #1d): every (M, N, K, act) in
    ``shapes`` is run ``iters`` times (after one untimed launch) with each candidate kernel — interleaved, random bf16
    operands, HIP events on the current stream — and the fastest is registered in the library's per-shape policy
    (``cmb_gemm_policy_set``), which every later ``cmb_gemm`` of that problem without a ``tile_hint`` follows.  The
    candidates (2590 = 4-wave register-buffered kernel, 2560 = 8-wave kernel) give bit-identical results, so this
    changes speed only.  Returns one dict per shape (microseconds per candidate, the choice).  ~1-2 ms per shape."""
    lib = L.load()
    device = device or torch.device("cuda", torch.cuda.current_device())
    report = []
    for (M, N, K, act) in shapes:
        a = torch.randn((M, K), device=device, dtype=torch.bfloat16)
        w = torch.randn((N, K), device=device, dtype=torch.bfloat16)
        out = torch.empty((M, N), device=device, dtype=torch.bfloat16)
        evs = {c: [] for c in candidates}
        for it in range(iters + 1):
            for c in candidates:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                k_gemm(a, w, act=act, out=out, tile=c)
                e1.record()
                if it:
                    evs[c].append((e0, e1))
        torch.cuda.synchronize(device)
        us = {c: min(e0.elapsed_time(e1) for e0, e1 in evs[c]) * 1e3 for c in candidates}
        best = min(us, key=us.get)
        L.check(lib.cmb_gemm_policy_set(M, N, K, act, best), "cmb_gemm_policy_set")
        report.append({"M": M, "N": N, "K": K, "act": act, "us": {str(c): round(v, 1) for c, v in us.items()},
                       "choice": best, "TFLOPs": {str(c): round(2.0 * M * N * K / v / 1e6, 1) for c, v in us.items()}})
        del a, w, out
    return report


# ---- region timing (bench.py ``roofline.region``: the tower + SVA part of the step, forward and backward) -----------
# While REGION_PROFILE is a list, the model glue brackets each piece of the region with HIP events on the launch
# stream: ``region_begin`` / ``region_fwd_end`` in the forward, and identity autograd nodes (``region_mark``) whose
# backward records the events of the matching backward span — the node on the piece's OUTPUT fires when its backward
# starts ("b0"), the node on its INPUT when the gradient leaves the piece ("b1": autograd runs the nodes of the piece,
# created after the input mark, before it).  Spans without an input mark (the first piece: towers have no input
# gradient) are closed by ``region_close`` after ``backward()`` returned.
REGION_PROFILE = None


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


class _RegionMarkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, span, key):
        ctx.span, ctx.key = span, key
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if ctx.key not in ctx.span:
            ctx.span[ctx.key] = _event()
        return g, None, None


def region_begin(tag: str):
    """Forward start of a span (None when nobody profiles)."""
    if REGION_PROFILE is None:
        return None
    span = {"tag": tag, "f0": _event()}
    REGION_PROFILE.append(span)
    return span


def region_mark(x: torch.Tensor, span, key: str) -> torch.Tensor:
    """key "b1" on a piece's input, "b0" on its output (see above)."""
    if span is None or not x.requires_grad:
        return x
    return _RegionMarkFn.apply(x, span, key)


def region_fwd_end(span) -> None:
    if span is not None:
        span["f1"] = _event()


def region_close() -> None:
    """After backward(): spans whose backward started ("b0") but has no input mark end here."""
    if REGION_PROFILE is None:
        return
    e = None
    for span in REGION_PROFILE:
        if "b0" in span and "b1" not in span:
            e = e or _event()
            span["b1"] = e


def region_ms(spans) -> dict:
    """Forward / backward milliseconds of the recorded spans (call after a device synchronise)."""
    fwd = sum(s["f0"].elapsed_time(s["f1"]) for s in spans if "f1" in s)
    bwd = sum(s["b0"].elapsed_time(s["b1"]) for s in spans if "b0" in s and "b1" in s)
    return {"fwd_ms": fwd, "bwd_ms": bwd, "spans": len(spans)}


def k_transpose(x: torch.Tensor, r_pad: Optional[int] = None) -> torch.Tensor:
    """[R,C] -> [C,R_pad] (zero padded)."""
    L.require_gpu(x)
    R, Cc = x.shape
    if x.stride(1) != 1:
        x = x.contiguous()
    r_pad = r_pad or pad_to(R, 8)
    out = torch.empty((Cc, r_pad), dtype=x.dtype, device=x.device)
    L.call("cmb_transpose", L.dtype_code(x.dtype), x.data_ptr(), R, Cc, x.stride(0), out.data_ptr(), r_pad, device=x.device)
    return out


def k_gemm_tn(at: torch.Tensor, bt: torch.Tensor, *, out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32,
              split_k: int = 1, alpha: float = 1.0, beta: float = 0.0, M: Optional[int] = None, N: Optional[int] = None,
              batch: int = 1, a_bs: int = 0, b_bs: int = 0, c_bs: int = 0, ldc: Optional[int] = None) -> torch.Tensor:
    """C[M,N] = alpha * At[K,M]^T @ Bt[K,N] (+ beta C) on cmb_gemm_tn: both operands row-major over the K contraction rows,
    bf16, any K.  ``at`` [K, >=M] / ``bt`` [K, >=N] (row strides taken from the tensors); with ``batch`` > 1 problem z
    reads columns from a_bs*z / b_bs*z on and writes C + c_bs*z (elements).  The weight gradient dW = g^T x without
    transposed copies of g and x."""
    L.require_gpu(at, bt, out)
    if at.dtype != torch.bfloat16 or bt.dtype != torch.bfloat16 or at.dim() != 2 or bt.dim() != 2:
        raise L.CambrianAmdError("gemm_tn operands must be 2-D bf16")
    if at.stride(1) != 1 or bt.stride(1) != 1 or at.shape[0] != bt.shape[0]:
        raise L.CambrianAmdError("gemm_tn operands must be row-major with equal row counts")
    K = at.shape[0]
    M = at.shape[1] if M is None else M
    N = bt.shape[1] if N is None else N
    if out is None:
        if batch > 1:
            raise L.CambrianAmdError("gemm_tn: a batched launch needs the caller's output tensor")
        out = torch.empty((M, N), dtype=out_dtype, device=at.device)
    d, ws = _gemm_desc(L.dtype_code(at.dtype), M, N, K, at, L.identity_map(at.stride(0)), bt, bt.stride(0), out,
                       L.identity_map(ldc if ldc is not None else out.stride(0)), alpha=alpha, beta=beta, split_k=split_k,
                       slab_rows=max(batch, 1) * M, batch=(batch, a_bs, b_bs, c_bs))
    # (the timed region times the dominant kernel only; the span covers the split-K reduce the library launches behind the kernel)
    _gemm_launch("cmb_gemm_tn", (d,), at.device, f"cmb_gemm_tn(M={M}, N={N}, K={K}, batch={batch})",
                 GEMM_PROFILE if not GEMM_PROFILE_TILE else None,
                 lambda lib: (2.0 * max(batch, 1) * M * N * K, at.dtype, split_k, 128, (M, N, K, L.ACT_NONE, out.dtype == torch.float32),
                              KERNEL_ID_TN, max(batch, 1)))
    return out


def k_colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
             group: int = 0) -> torch.Tensor:
    """out[c] (+)= sum_r x[r, c]; with ``row_scale`` [R, C / group] fp32: sum_r row_scale[r, c // group] * x[r, c]."""
    L.require_gpu(x)
    R, Cc = x.shape
    if out is None:
        out = torch.zeros((Cc,), dtype=torch.float32, device=x.device)
    # partial rows of the fixed-order (run-to-run identical) cross-workgroup sum
    ws = torch.empty((max(L.load().cmb_colsum_workspace(R, Cc), 1),), dtype=torch.float32, device=x.device)
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.dim() != 2 or row_scale.stride(1) != 1 or row_scale.shape != (R, Cc // group):
            raise L.CambrianAmdError("colsum row_scale must be fp32 [R, C / group]")
        L.call("cmb_colsum_scaled", L.dtype_code(x.dtype), x.data_ptr(), R, Cc, x.stride(0), row_scale.data_ptr(),
               row_scale.stride(0), group, out.data_ptr(), ws.data_ptr(), ws.numel(), device=x.device)
        return out
    L.call("cmb_colsum", L.dtype_code(x.dtype), x.data_ptr(), R, Cc, x.stride(0), out.data_ptr(), ws.data_ptr(), ws.numel(),
           device=x.device)
    return out


def k_token_mean(x3: torch.Tensor) -> torch.Tensor:
    B, T, D = x3.shape
    out = torch.empty((B, D), dtype=x3.dtype, device=x3.device)
    L.call("cmb_token_mean_fwd", L.dtype_code(x3.dtype), x3.data_ptr(), B, T, D, out.data_ptr(), device=x3.device)
    return out


def k_token_mean_bwd(g: torch.Tensor, B: int, T: int, D: int, acc: torch.Tensor) -> None:
    """acc (fp32 [B*T, D]) += g[b] / T for every token of sample b (cmb_token_mean_bwd)."""
    L.call("cmb_token_mean_bwd", L.dtype_code(g.dtype), g.data_ptr(), B, T, D, acc.data_ptr(), device=g.device)


def k_segment_sum(x: torch.Tensor, rep: int) -> torch.Tensor:
    """[M, D] -> [M/rep, D], summing each run of `rep` consecutive rows (the mean kernel, scaled by rep)."""
    M, D = x.shape
    xc = x if x.is_contiguous() else x.contiguous()
    m = k_token_mean(xc.view(M // rep, rep, D))
    return (m.to(torch.float32) * float(rep)).to(x.dtype)


def k_layernorm_fwd(x, gamma, beta, eps, add=None, side=1, grid_r=1, want_stats=True):
    L.require_gpu(x, gamma, beta, add)
    rows, D = x.shape
    y = torch.empty((rows, D), dtype=x.dtype, device=x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if want_stats else None
    L.call("cmb_layernorm_fwd", L.dtype_code(x.dtype), x.data_ptr(), rows, D, x.stride(0), L.ptr(add), side, grid_r,
           L.ptr(gamma), L.ptr(beta), eps, y.data_ptr(), D, L.ptr(mean), L.ptr(rstd), device=x.device)
    return y, mean, rstd


def k_layernorm_fwd_multi(x: torch.Tensor, adds, eps: float, side: int = 1, grid_r: int = 1):
    """cmb_layernorm_fwd_multi: [(y_l, mean_l, rstd_l)] = the non-affine LayerNorms of x + adds[l][window position] for every
    table of ``adds`` (fp32 [grid_r^2, D] or None) in one pass over x; each triple equals k_layernorm_fwd(x, None, None, eps,
    add=adds[l], ...) bit for bit."""
    L.require_gpu(x, *[a for a in adds if a is not None])
    rows, D = x.shape
    out = []
    for lo in range(0, len(adds), L.LN_MULTI_MAX):
        chunk = adds[lo:lo + L.LN_MULTI_MAX]
        d = L.LnFwdMultiDesc()
        d.dtype, d.layers = L.dtype_code(x.dtype), len(chunk)
        d.x, d.ldx, d.rows, d.D, d.side, d.grid_r, d.eps = x.data_ptr(), x.stride(0), rows, D, side, grid_r, eps
        for i, a in enumerate(chunk):
            if a is not None and (a.dtype != torch.float32 or not a.is_contiguous() or tuple(a.shape) != (grid_r * grid_r, D)):
                raise L.CambrianAmdError("layernorm_fwd_multi: every table must be a dense fp32 [grid_r^2, D] tensor")
            y = torch.empty((rows, D), dtype=x.dtype, device=x.device)
            mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
            rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
            d.add[i] = None if a is None else a.data_ptr()
            d.y[i], d.mean[i], d.rstd[i] = y.data_ptr(), mean.data_ptr(), rstd.data_ptr()
            out.append((y, mean, rstd))
        L.call("cmb_layernorm_fwd_multi", C.byref(d), device=x.device)
    return out


def k_row_stats(x: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, rstd) fp32 [rows] of a LayerNorm over the rows of x — no normalised output (cmb_row_stats)."""
    L.require_gpu(x)
    rows, D = x.shape
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    L.call("cmb_row_stats", L.dtype_code(x.dtype), x.data_ptr(), rows, D, x.stride(0), eps, mean.data_ptr(), rstd.data_ptr(),
           device=x.device)
    return mean, rstd


def k_layernorm_bwd(dy, x, mean, rstd, gamma=None, add=None, side=1, grid_r=1, dx_acc: Optional[torch.Tensor] = None,
                    want_dgamma=True, want_dadd=True):
    """Returns (dx, dgamma, dbeta, dadd).  With ``dx_acc`` (fp32 [rows,D]) dx is accumulated there and the
    returned dx is None."""
    L.require_gpu(dy, x, mean, rstd, gamma, add, dx_acc)
    rows, D = x.shape
    dev = x.device
    if dy.stride(1) != 1:
        dy = dy.contiguous()
    dgamma = torch.zeros((D,), dtype=torch.float32, device=dev) if (gamma is not None and want_dgamma) else None
    dbeta = torch.zeros((D,), dtype=torch.float32, device=dev) if (gamma is not None and want_dgamma) else None
    dadd = torch.zeros_like(add) if (add is not None and want_dadd) else None
    if dx_acc is not None:
        dx, acc = dx_acc, 1
    else:
        dx, acc = torch.empty((rows, D), dtype=x.dtype, device=dev), 0
    # one slab of partial rows per wanted output (fixed-order, run-to-run identical cross-workgroup sums)
    nslab = (dgamma is not None) + (dbeta is not None) + (dadd is not None)
    per = L.load().cmb_layernorm_bwd_workspace(rows, D, grid_r if add is not None else 1) if rows > 0 else 0
    ws = torch.empty((max(nslab * per, 1),), dtype=torch.float32, device=dev)
    L.call("cmb_layernorm_bwd", L.dtype_code(x.dtype), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), rows, D,
           L.ptr(add), side, grid_r, L.ptr(gamma), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), D, acc, L.ptr(dgamma),
           L.ptr(dbeta), L.ptr(dadd), ws.data_ptr(), ws.numel(), device=dev)
    return (None if dx_acc is not None else dx), dgamma, dbeta, dadd


# ---- LLM-side launchers: operands are what the autograd nodes below prepared (2-D, contiguous, one dtype) ----------------
def k_rmsnorm_fwd(x2: torch.Tensor, w32: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, rstd) = (rmsnorm(x2) * w32, fp32 [rows]) of contiguous rows x2 [rows, D] (cmb_rmsnorm_fwd)."""
    rows, D = x2.shape
    y = torch.empty_like(x2)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x2.device)
    L.call("cmb_rmsnorm_fwd", L.dtype_code(x2.dtype), x2.data_ptr(), rows, D, w32.data_ptr(), eps, y.data_ptr(), rstd.data_ptr(),
           device=x2.device)
    return y, rstd


def k_add_rmsnorm_fwd(x2: torch.Tensor, d2: torch.Tensor, w32: torch.Tensor, eps: float):
    """(s, y, rstd) = (x2 + d2, rmsnorm(s) * w32, fp32 [rows]) in one pass (cmb_add_rmsnorm_fwd)."""
    rows, D = x2.shape
    s = torch.empty_like(x2)
    y = torch.empty_like(x2)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x2.device)
    L.call("cmb_add_rmsnorm_fwd", L.dtype_code(x2.dtype), x2.data_ptr(), d2.data_ptr(), rows, D, w32.data_ptr(), eps,
           s.data_ptr(), y.data_ptr(), rstd.data_ptr(), device=x2.device)
    return s, y, rstd


def k_rmsnorm_bwd(gy: torch.Tensor, x2: torch.Tensor, w32: torch.Tensor, rstd: torch.Tensor, add: Optional[torch.Tensor] = None,
                  want_dw: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(dx, dw) of y = rmsnorm(x2) * w32, with ``add`` (a gradient that reaches x2 by another route) summed into dx.
    Trainable weight (``want_dw``): the two-pass cmb_rmsnorm_bwd that also reduces dw (fp32 [D]), then an ATen ``dx + add``.
    Frozen weight: the single-pass cmb_rmsnorm_bwd_add (row kept in registers, ``add`` read in the same pass), dw None."""
    rows, D = x2.shape
    dx = torch.empty_like(x2)
    if not want_dw:
        L.call("cmb_rmsnorm_bwd_add", L.dtype_code(x2.dtype), gy.data_ptr(), x2.data_ptr(), L.ptr(add), rows, D, w32.data_ptr(),
               rstd.data_ptr(), dx.data_ptr(), device=x2.device)
        return dx, None
    dw = torch.zeros((D,), dtype=torch.float32, device=x2.device)
    L.call("cmb_rmsnorm_bwd", L.dtype_code(x2.dtype), gy.data_ptr(), x2.data_ptr(), rows, D, w32.data_ptr(), rstd.data_ptr(),
           dx.data_ptr(), dw.data_ptr(), device=x2.device)
    return (dx if add is None else dx + add), dw


def k_rope_apply(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Rotates the contiguous x [ntok, H, Dh] IN PLACE by the cos / sin rows of ``rope_table`` (``inverse``: back)."""
    ntok, H, Dh = x.shape
    L.call("cmb_rope_apply", L.dtype_code(x.dtype), x.data_ptr(), cos.data_ptr(), sin.data_ptr(), ntok, H, Dh, H * Dh,
           1 if inverse else 0, device=x.device, what="cmb_rope_apply(inverse)" if inverse else None)
    return x


def k_qkv_rope(packed: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
               merge: bool = False) -> None:
    """cmb_qkv_rope over token-major q [B, S, nh, hd], k / v [B, S, nkv, hd] and packed [B, S, (nh + 2 nkv) hd]: split (packed
    -> q, k, v with RoPE on q and k) or ``merge`` (the backward: q, k, v -> packed with the inverse rotation)."""
    B, S, nh, hd = q.shape
    L.call("cmb_qkv_rope", L.dtype_code(packed.dtype), 1 if merge else 0, packed.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, S,
           nh, k.shape[2], hd, q.data_ptr(), k.data_ptr(), v.data_ptr(), device=packed.device,
           what="cmb_qkv_rope(merge)" if merge else "cmb_qkv_rope(split)")


def k_act_bwd(g: torch.Tensor, pre: torch.Tensor, act: int) -> torch.Tensor:
    """g * act'(pre) over dense tensors of one shape and dtype (cmb_act_bwd)."""
    gp = torch.empty_like(pre)
    L.call("cmb_act_bwd", L.dtype_code(g.dtype), act, g.data_ptr(), pre.data_ptr(), pre.numel(), gp.data_ptr(), device=g.device)
    return gp


def k_swiglu_fwd(g2: torch.Tensor, u2: torch.Tensor, cols: Optional[int] = None, u_col: int = 0, what: Optional[str] = None):
    """h [rows, cols] = silu(g2[:, :cols]) * u2[:, u_col:u_col + cols] (cmb_act_mul; row strides taken from the tensors).  The
    packed gate|up form passes the one [rows, 2I] tensor twice with ``cols`` = ``u_col`` = I."""
    rows = g2.shape[0]
    cols = g2.shape[1] if cols is None else cols
    h = torch.empty((rows, cols), dtype=g2.dtype, device=g2.device)
    L.call("cmb_act_mul", L.dtype_code(g2.dtype), L.ACT_SILU, g2.data_ptr(), g2.stride(0), u2.data_ptr() + u_col * u2.element_size(),
           u2.stride(0), rows, cols, h.data_ptr(), cols, device=g2.device, what=what or "cmb_act_mul(silu)")
    return h


def k_swiglu_bwd(dh2: torch.Tensor, g2: torch.Tensor, u2: torch.Tensor, dg: torch.Tensor, du: torch.Tensor,
                 cols: Optional[int] = None, u_col: int = 0, what: Optional[str] = None) -> None:
    """Backward of ``k_swiglu_fwd`` (cmb_swiglu_bwd): dg[:, :cols] and du[:, u_col:u_col + cols] from dh2 [rows, cols]; the packed
    form passes its one [rows, 2I] gradient buffer as both ``dg`` and ``du``."""
    rows = g2.shape[0]
    cols = g2.shape[1] if cols is None else cols
    es = g2.element_size()
    L.call("cmb_swiglu_bwd", L.dtype_code(g2.dtype), dh2.data_ptr(), dh2.stride(0), g2.data_ptr(), g2.stride(0),
           u2.data_ptr() + u_col * es, u2.stride(0), rows, cols, dg.data_ptr(), dg.stride(0), du.data_ptr() + u_col * es,
           du.stride(0), device=g2.device, what=what)


def k_cross_entropy_fwd(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lse, loss_rows) fp32 [T] of row-major logits [T, V] and contiguous int64 labels [T] (cmb_cross_entropy_fwd)."""
    T, V = logits.shape
    lse = torch.empty((T,), dtype=torch.float32, device=logits.device)
    loss_rows = torch.empty((T,), dtype=torch.float32, device=logits.device)
    L.call("cmb_cross_entropy_fwd", L.dtype_code(logits.dtype), logits.data_ptr(), T, V, logits.stride(0), labels.data_ptr(),
           ignore_index, lse.data_ptr(), loss_rows.data_ptr(), device=logits.device)
    return lse, loss_rows


def k_cross_entropy_bwd(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int, lse: torch.Tensor, scale: torch.Tensor,
                        out: torch.Tensor) -> None:
    """out = scale * d(loss rows) / d(logits) (``scale`` an fp32 device scalar; ``out`` may be ``logits`` itself)."""
    T, V = logits.shape
    L.call("cmb_cross_entropy_bwd", L.dtype_code(logits.dtype), logits.data_ptr(), T, V, logits.stride(0), labels.data_ptr(),
           ignore_index, lse.data_ptr(), scale.data_ptr(), out.data_ptr(), out.stride(0), device=logits.device)


def k_flash_attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, causal: int, n: int,
                     key_valid: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, H, S, D], k / v [B, HKV, S, D] as transposed views of token-major storage -> (out [B, S, H, D], lse [B, H, S])."""
    B, H, S, D = q.shape
    HKV = k.shape[1]
    out = torch.empty((B, S, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    L.call("cmb_flash_attn_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, S, H, HKV, D, S * H * D, H * D, D, S * HKV * D,
           HKV * D, D, scale, causal, n, L.ptr(key_valid), out.data_ptr(), lse.data_ptr(), device=q.device)
    return out, lse


def k_flash_attn_bwd(q, k, v, out, dout, lse, scale: float, causal: int, n: int, key_valid: Optional[torch.Tensor]):
    """Operands laid out as in ``k_flash_attn_fwd`` (``out`` / ``dout`` like q, ``lse`` contiguous) -> (dq [B, S, H, D],
    dk, dv [B, S, HKV, D]): the dQ kernel and the dK/dV kernel of flash_bwd.hip."""
    B, H, S, D = q.shape
    HKV = k.shape[1]
    dq = torch.empty((B, S, H, D), dtype=q.dtype, device=q.device)
    dk = torch.empty((B, S, HKV, D), dtype=q.dtype, device=q.device)
    dv = torch.empty((B, S, HKV, D), dtype=q.dtype, device=q.device)
    dvec = torch.empty((2, B, H, S), dtype=torch.float32, device=q.device)   # [0] D, [1] lse * log2 e (flash2.hip)
    L.call("cmb_flash_attn_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), B, S,
           H, HKV, D, S * H * D, H * D, D, S * HKV * D, HKV * D, D, scale, causal, n, L.ptr(key_valid), dvec.data_ptr(),
           dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), device=q.device)
    return dq, dk, dv


def k_embed_splice_fwd(ids: torch.Tensor, table: torch.Tensor, feat: torch.Tensor, newline: torch.Tensor, side: int,
                       image_token: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Contiguous ids [B, S], table [V, H], feat [B, side^2, H], newline [H] of one dtype -> (inputs_embeds [B, S, H], the
    position of each sample's visual span, int32 [B]) (cmb_embed_splice_fwd)."""
    B, S = ids.shape
    V, H = table.shape
    out = torch.empty((B, S, H), dtype=feat.dtype, device=feat.device)
    pos = torch.empty((B,), dtype=torch.int32, device=feat.device)
    L.call("cmb_embed_splice_fwd", L.dtype_code(feat.dtype), ids.data_ptr(), B, S, H, image_token, table.data_ptr(), V,
           feat.data_ptr(), side, newline.data_ptr(), out.data_ptr(), pos.data_ptr(), device=feat.device)
    return out, pos


def k_embed_splice_bwd(dout: torch.Tensor, pos: torch.Tensor, side: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Contiguous d(inputs_embeds) [B, S, H] -> (d feat [B, side^2, H], d newline fp32 [H]) (cmb_embed_splice_bwd)."""
    B, S, H = dout.shape
    dfeat = torch.empty((B, side * side, H), dtype=dout.dtype, device=dout.device)
    dnl = torch.zeros((H,), dtype=torch.float32, device=dout.device)
    ws = torch.empty((max(B * side * H, 1),), dtype=torch.float32, device=dout.device)   # newline partial rows
    L.call("cmb_embed_splice_bwd", L.dtype_code(dout.dtype), dout.data_ptr(), pos.data_ptr(), B, S, H, side, dfeat.data_ptr(),
           dnl.data_ptr(), ws.data_ptr(), ws.numel(), device=dout.device)
    return dfeat, dnl


def k_fold_kv_fwd(ts: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """ts = contiguous fp32 (Wk, gk, bk, Wv, gv, bv) -> ([Wk*gk ; Wv*gv] [2H, K], [Wk@bk ; Wv@bv] [2H]) (cmb_sva_fold_kv_fwd)."""
    H, K = ts[0].shape
    w = torch.empty((2 * H, K), dtype=torch.float32, device=ts[0].device)
    b = torch.empty((2 * H,), dtype=torch.float32, device=ts[0].device)
    L.call("cmb_sva_fold_kv_fwd", *[t.data_ptr() for t in ts], H, K, w.data_ptr(), b.data_ptr(), device=w.device)
    return w, b


def k_fold_kv_bwd(dw: torch.Tensor, db: torch.Tensor, ts: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """Gradients of the six inputs of ``k_fold_kv_fwd`` from contiguous fp32 dw [2H, K], db [2H] (cmb_sva_fold_kv_bwd)."""
    H, K = ts[0].shape
    dev = ts[0].device
    outs = [torch.empty_like(t) for t in ts]
    ws = torch.empty((L.load().cmb_sva_fold_kv_bwd_workspace(H, K) // 4,), dtype=torch.float32, device=dev)
    L.call("cmb_sva_fold_kv_bwd", dw.data_ptr(), db.data_ptr(), *[t.data_ptr() for t in ts], H, K, *[o.data_ptr() for o in outs],
           ws.data_ptr(), ws.numel() * 4, device=dev)
    return outs


def _fill_sva(desc: SvaDesc, q, kvs, masks, r_list, B, qside, heads, hd, window_major=False):
    desc.dtype = L.dtype_code(q.dtype)
    desc.window_major = 1 if window_major else 0
    desc.B, desc.qside, desc.heads, desc.hd, desc.ntowers = B, qside, heads, hd, len(kvs)
    desc.q, desc.ldq = q.data_ptr(), q.stride(0)
    for i, (kv, r) in enumerate(zip(kvs, r_list)):
        G = qside * r
        if kv.dtype != q.dtype or tuple(kv.shape) != (B * G * G, 2 * heads * hd) or kv.stride(1) != 1:
            raise L.CambrianAmdError(f"kv[{i}] must be [{B * G * G},{2 * heads * hd}] of {q.dtype}, got {tuple(kv.shape)}")
        desc.r[i] = r
        desc.kv[i], desc.ldkv[i] = kv.data_ptr(), kv.stride(0)
        m = masks[i] if masks is not None else None
        if m is not None:
            if m.dtype != torch.uint8 or not m.is_contiguous() or m.numel() != B * qside * qside * r * r:
                raise L.CambrianAmdError(f"mask[{i}] must be contiguous uint8 [{B * qside * qside},{r * r}]")
            desc.mask[i] = m.data_ptr()
        else:
            desc.mask[i] = None


def k_sva_attn_fwd(q, kvs, masks, r_list, B, qside, heads, hd, window_major=False):
    L.require_gpu(q, *kvs)
    d = SvaDesc()
    _fill_sva(d, q, kvs, masks, r_list, B, qside, heads, hd, window_major)
    Bq = B * qside * qside
    out = torch.empty((Bq, heads * hd), dtype=q.dtype, device=q.device)
    lse = torch.empty((Bq, heads), dtype=torch.float32, device=q.device)
    d.out, d.ldo, d.lse = out.data_ptr(), out.stride(0), lse.data_ptr()
    L.call("cmb_sva_attn_fwd", C.byref(d), device=q.device)
    return out, lse


def k_sva_attn_bwd(dout, q, kvs, masks, r_list, out, lse, B, qside, heads, hd, window_major=False):
    d = SvaDesc()
    _fill_sva(d, q, kvs, masks, r_list, B, qside, heads, hd, window_major)
    if dout.stride(1) != 1:
        dout = dout.contiguous()
    dq = torch.empty_like(q)
    dkvs = [torch.empty_like(kv) for kv in kvs]
    d.out, d.ldo, d.lse = out.data_ptr(), out.stride(0), lse.data_ptr()
    d.dout, d.lddo = dout.data_ptr(), dout.stride(0)
    d.dq, d.lddq = dq.data_ptr(), dq.stride(0)
    for i, t in enumerate(dkvs):
        d.dkv[i] = t.data_ptr()
    L.call("cmb_sva_attn_bwd", C.byref(d), device=q.device)
    return dq, dkvs


# ================================================================================================
# prepared weights: bf16 copy + transposed bf16 copy of the trainable 2-D weights, refreshed in ONE launch per step
# ================================================================================================
# Round 5 cast every fp32 master per use (cmb_cast in LinearFn.forward: 171 launches per step) and transposed it again per
# backward (cmb_transpose for dx = g W: 166 launches) — 3.1 ms of 5-12 us kernels per step.  The model now opens a window per
# training forward (weight_step_begin / weight_step_end): begin() refreshes the copies of every weight registered so far with
# one cmb_weight_prep launch (one pass over the masters), the linears inside the window take them from the cache (a weight
# seen for the first time is prepared on the spot and registered), the backward uses what the forward captured.  Outside a
# window (direct calls of a layer, the re-computation forward of activation checkpointing, eval) nothing is cached: weights
# may have changed in ways no version counter shows (ZeRO-2 writes the all-gathered shards straight into the flat buckets).
# CAMBRIAN_AMD_PREP_WEIGHTS=0 restores the per-use launches (A/B runs).
PREP_WEIGHTS = L.env_flag("CAMBRIAN_AMD_PREP_WEIGHTS", True)
_PREP: dict = {}
_PREP_EPOCH = 0
_PREP_ACTIVE = False
_PREP_TABLE = None   # (signature, device job table, n_jobs, total_tiles)
_PREP_TMP: dict = {}   # id(tensor) -> (weakref, w_c, w_t): per-step weights made inside a window (the folded K|V weights)


class _PrepEntry:
    __slots__ = ("ref", "off", "shape", "stride", "w_c", "w_t", "rows_pad", "epoch", "src_ptr")


def _prep_src_ptr(base: torch.Tensor, e: "_PrepEntry") -> int:
    return base.data_ptr() + (e.off - base.storage_offset()) * base.element_size()


def _prep_job(e: "_PrepEntry", base: torch.Tensor, tile0: int) -> "L.PrepJob":
    j = L.PrepJob()
    j.src, j.dst, j.dst_t = _prep_src_ptr(base, e), e.w_c.data_ptr(), e.w_t.data_ptr()
    j.ld_src, j.src_dtype = e.stride[0], L.dtype_code(base.dtype)
    j.rows, j.cols, j.rows_pad, j.tile0, j.reserved = e.shape[0], e.shape[1], e.rows_pad, tile0, 0
    return j


def weight_step_begin() -> None:
    """Open the prepared-weight window of a training forward and refresh every registered weight's copies in one launch."""
    global _PREP_EPOCH, _PREP_ACTIVE, _PREP_TABLE
    if not PREP_WEIGHTS:
        return
    _PREP_EPOCH += 1
    _PREP_ACTIVE = True
    _PREP_TMP.clear()
    live = []
    for key in list(_PREP):
        e = _PREP[key]
        base = e.ref()
        if base is None or not base.is_cuda:
            del _PREP[key]
            continue
        live.append((key, e, base))
    if not live:
        return
    dev = live[0][2].device
    sig = (dev, tuple((key, _prep_src_ptr(base, e), e.w_c.data_ptr()) for key, e, base in live))
    if _PREP_TABLE is None or _PREP_TABLE[0] != sig:
        jobs = (L.PrepJob * len(live))()
        tile0 = 0
        lib = L.load()
        for i, (key, e, base) in enumerate(live):
            jobs[i] = _prep_job(e, base, tile0)
            tile0 += lib.cmb_weight_prep_tiles(e.rows_pad, e.shape[1])
        table = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
        _PREP_TABLE = (sig, table, len(live), tile0)
    _, table, n, tiles = _PREP_TABLE
    L.call("cmb_weight_prep", table.data_ptr(), n, tiles, device=dev)
    for key, e, base in live:
        e.epoch, e.src_ptr = _PREP_EPOCH, _prep_src_ptr(base, e)


def weight_step_end() -> None:
    global _PREP_ACTIVE
    _PREP_ACTIVE = False
    _PREP_TMP.clear()


def prepare_step_weight(w: torch.Tensor) -> None:
    """A weight computed inside the window (fp32 [N, K], e.g. the folded K|V projection): its bf16 copy and transposed copy in
    one launch, found by ``prepared_weight`` for ``w`` itself and for row slices of it (the absorbed tower's K / V halves)."""
    if not (_PREP_ACTIVE and w.is_cuda and w.dim() == 2 and w.is_contiguous() and w.dtype == torch.float32 and w.shape[1] % 8 == 0):
        return
    import weakref
    N, K = w.shape
    w_c = torch.empty((N, K), dtype=torch.bfloat16, device=w.device)
    w_t = torch.empty((K, pad_to(N, 64)), dtype=torch.bfloat16, device=w.device)
    j = L.PrepJob()
    j.src, j.dst, j.dst_t, j.ld_src, j.src_dtype = w.data_ptr(), w_c.data_ptr(), w_t.data_ptr(), K, L.F32
    j.rows, j.cols, j.rows_pad, j.tile0, j.reserved = N, K, w_t.shape[1], 0, 0
    L.call("cmb_weight_prep_one", C.byref(j), device=w.device)
    _PREP_TMP[id(w)] = (weakref.ref(w), w_c, w_t)


def prepared_weight(weight: torch.Tensor, dt: torch.dtype):
    """(bf16 copy [N, K], transposed bf16 copy [K, pad64(N)]) of a trainable weight inside a prepared-weight window, else None.
    Only nn.Parameters (or views of one) qualify: their identity is what the cache is keyed on."""
    if not (_PREP_ACTIVE and dt == torch.bfloat16 and weight.is_cuda and weight.dim() == 2 and weight.stride(1) == 1):
        return None
    base = weight._base if weight._base is not None else weight
    tmp = _PREP_TMP.get(id(base))
    if tmp is not None and tmp[0]() is base:   # a weight made inside this window, or rows [r0, r1) of it
        ldw = base.shape[1]
        if weight is base:
            return tmp[1], tmp[2]
        off = weight.storage_offset() - base.storage_offset()
        if weight.shape[1] == ldw and weight.stride(0) == ldw and off % ldw == 0:
            r0 = off // ldw
            return tmp[1][r0:r0 + weight.shape[0]], tmp[2][:, r0:r0 + weight.shape[0]]
        return None
    if not isinstance(base, torch.nn.Parameter) or base.dtype not in (torch.float32, torch.bfloat16):
        return None
    N, K = weight.shape
    if K % 8 or weight.stride(0) % 8 or weight.data_ptr() % 16:
        return None
    key = (id(base), weight.storage_offset(), (N, K), tuple(weight.stride()))
    e = _PREP.get(key)
    if e is not None and e.ref() is not base:
        e = None   # the id was recycled
    if e is None:
        import weakref
        e = _PrepEntry()
        e.ref = weakref.ref(base)
        e.off, e.shape, e.stride, e.rows_pad, e.epoch, e.src_ptr = weight.storage_offset(), (N, K), tuple(weight.stride()), pad_to(N, 64), -1, 0
        e.w_c = torch.empty((N, K), dtype=torch.bfloat16, device=weight.device)
        e.w_t = torch.empty((K, e.rows_pad), dtype=torch.bfloat16, device=weight.device)
        _PREP[key] = e
    if e.epoch != _PREP_EPOCH or e.src_ptr != weight.data_ptr():   # first sight in this window: prepare it on the spot
        j = _prep_job(e, base, 0)
        L.call("cmb_weight_prep_one", C.byref(j), device=weight.device)
        e.epoch, e.src_ptr = _PREP_EPOCH, weight.data_ptr()
    return e.w_c, e.w_t


# ================================================================================================
# autograd: linear
# ================================================================================================
# CAMBRIAN_AMD_TN_WGRAD=0: weight gradients through transposed copies + the NT kernels (A/B runs, tests of the old path)
TN_WGRAD = L.env_flag("CAMBRIAN_AMD_TN_WGRAD", True)


def _tn_wgrad_wins(rows: int, n_out: int, k_in: int) -> bool:
    """Where dW = g^T x on cmb_gemm_tn beats transposed copies + the 256-tile NT kernels (tools/bench_tn.py,
    profiles/r03c_wgrad_tn_vs_nt.md): every weight of up to 256 output tiles (4096 x 1024), with one exception — the
    ConvNeXt-side projector's 1024 x 3072 at 147456 rows (192 tiles: two row slices of 74 k rows each run 1.5 rounds; 1556
    vs 1323 us).  The 4096 x 4096 mm_projector weight (1024 tiles, no split) stays on the 4-wave NT kernel (341 vs 303 us)."""
    tiles = ((n_out + 127) // 128) * ((k_in + 127) // 128)
    return tiles <= 256 and not (rows > 65536 and tiles > 128)


def _tn_splits(m_cols: int, n_cols: int, rows: int, batch: int = 1) -> int:
    """Split-K factor of a cmb_gemm_tn weight gradient: as many row slices as fill ONE round of the kernel's two workgroups
    per CU (512 on the 256-CU part).  Measured (13824 x 1024 x 1024: 2 / 4 / 8 / 12 / 16 slices = 112 / 67 / 52 / 65 / 67 us;
    2048 x 1024: best at 4; 1024 x 1152: best at 6): one full round beats 1.5 rounds with smaller slabs."""
    tiles = batch * ((m_cols + 127) // 128) * ((n_cols + 127) // 128)
    return max(1, min(512 // max(tiles, 1), rows // 128, 64))


def _wgrad_splits(n_out: int, k_in: int, m_pad: int, kstep: int) -> int:
    tiles = ((n_out + 127) // 128) * ((k_in + 127) // 128)
    want = max(1, 768 // tiles)
    return max(1, min(want, m_pad // kstep // 4, 64))


def _as_dtype_contig(t: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    if t.dtype == dt and t.is_contiguous():
        return t
    return k_cast(t.contiguous(), dt)


def _wgrad_into(g: torch.Tensor, x: torch.Tensor, out: torch.Tensor) -> None:
    """out[N, K] (fp32: a whole weight gradient or a column slice of one, row stride out.stride(0)) = g[R, N]^T x[R, K], the one
    place that picks the route of a weight gradient."""
    R, N = g.shape
    K = x.shape[1]
    dt = g.dtype
    if (dt == torch.bfloat16 and R > 0 and N % 8 == 0 and K % 8 == 0 and x.stride(1) == 1 and x.stride(0) % 8 == 0
            and x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and g.stride(1) == 1 and g.stride(0) % 8 == 0
            and TN_WGRAD and _tn_wgrad_wins(R, N, K)):  # everything cmb_gemm_tn checks (gemm_tn_dispatch)
        # dW = g^T x with g and x as they lie (cmb_gemm_tn: transposing LDS reads, rows beyond R contribute zero)
        k_gemm_tn(g, x, out=out, split_k=_tn_splits(N, K, R), M=N, N=K, ldc=out.stride(0))
    else:  # fp32 parity path / odd widths: transposed copies for the NT kernel
        ks = _kstep(dt)
        m_pad = pad_to(R, ks)
        k_gemm(k_transpose(g, m_pad), k_transpose(x, m_pad), out=out, split_k=_wgrad_splits(N, K, m_pad, ks))


def _wgrad(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """g[R, N]^T x[R, K] as a new fp32 [N, K] tensor."""
    out = torch.empty((g.shape[1], x.shape[1]), dtype=torch.float32, device=g.device)
    _wgrad_into(g, x, out)
    return out


class LinearFn(torch.autograd.Function):
    """y = act(x @ W^T + b) (* colscale) (+ residual).  x: [M,K] compute dtype; W: [N,K] fp32 master (or
    compute dtype); gradients for W / b come out in fp32 straight from the fp32 accumulators.
    ``res_rep`` > 0 means residual is [M/res_rep, N] and output row r adds residual[r // res_rep]
    (the per-image context term of proj_in, vision_sampler.py:279-292, never materialised per query)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act: int, residual, res_rep: int, colscale, heavy: bool = False, link=None, role: int = 0):
        dt = x.dtype
        # ``link`` (a dict private to one block) joins the two uses of a block's input t — y1 = linear(t, ...) (role 1, the
        # "sink") ... out = linear(h, ..., residual=t) (role 2, the "source"): autograd would sum d(t) = g1 W1 + d(out) with an
        # ATen add over [rows, width]; the source's backward (it always runs first: its input descends from the sink's output)
        # parks d(out) in the link instead of returning it and the sink's d(x) GEMM adds it in its epilogue.
        ctx.link = None
        if link is not None and LINK_RESIDUAL_GRADS:
            if role == 1 and ctx.needs_input_grad[0]:
                link["armed"] = (x.data_ptr(), tuple(x.shape))
                ctx.link = link
            elif role == 2 and residual is not None and res_rep == 0 and ctx.needs_input_grad[4] and residual.dtype == dt \
                    and residual.is_contiguous() and link.get("armed") == (residual.data_ptr(), tuple(residual.shape)):
                ctx.link = link
        ctx.role = role
        prep = prepared_weight(weight, dt)
        w_c, ctx.w_t = prep if prep is not None else (k_cast(weight, dt), None)
        b_c = None if bias is None else k_cast(bias, torch.float32)
        need_pre = act != L.ACT_NONE and (x.requires_grad or weight.requires_grad
                                          or (bias is not None and bias.requires_grad))
        pre = torch.empty((x.shape[0], weight.shape[0]), dtype=dt, device=x.device) if need_pre else None
        r_map = None
        if residual is not None:
            residual = _as_dtype_contig(residual, dt)
            if res_rep > 0:
                if residual.dim() != 2 or residual.shape[0] * res_rep != x.shape[0]:
                    raise L.CambrianAmdError("broadcast residual must be [M/res_rep, N]")
                r_map = L.make_map(res_rep, 1, residual.stride(0), 0, 0)
        if heavy and fp8_linear_eligible(x, weight):
            xq, xinv = k_quantize_fp8_rows(x if x.is_contiguous() else x.contiguous())
            wq, winv = _fp8_weight(weight)
            y = k_gemm_fp8(xq, xinv, wq, winv, bias=b_c, act=act, residual=residual, r_map=r_map, colscale=colscale,
                           pre_out=pre)
        else:
            y = k_gemm(x, w_c, bias=b_c, act=act, residual=residual, r_map=r_map, colscale=colscale, pre_out=pre)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.res_rep = res_rep
        ctx.save_for_backward(x, w_c, pre, colscale)
        ctx.w_dtype = weight.dtype
        ctx.b_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_c, pre, colscale = ctx.saved_tensors
        dt = x.dtype
        dy = _as_dtype_contig(dy, dt)
        need_x, need_w, need_b, _, need_res = ctx.needs_input_grad[:5]
        M, N = x.shape[0], w_c.shape[0]
        dres = None
        if need_res:
            if ctx.link is not None and ctx.role == 2:
                ctx.link["g"] = dy                      # handed to the sink's d(x) GEMM (see forward)
            else:
                dres = k_segment_sum(dy, ctx.res_rep) if ctx.res_rep > 0 else dy
        g = dy
        if colscale is not None:
            g = dy * colscale.to(dt)  # LayerScale belongs to the frozen towers; kept for completeness
        if ctx.act != L.ACT_NONE:
            g = k_act_bwd(g, pre, ctx.act)
        dx = dw = db = None
        ks = _kstep(dt)
        if need_x:
            n_pad = pad_to(N, ks)
            w_t = ctx.w_t if (ctx.w_t is not None and ctx.w_t.shape[1] == n_pad) else k_transpose(w_c, n_pad)  # [K, N_pad]
            parked = ctx.link.pop("g", None) if (ctx.link is not None and ctx.role == 1) else None
            if n_pad != N:
                gpad = torch.zeros((M, n_pad), dtype=dt, device=g.device)
                gpad[:, :N] = g
                dx = k_gemm(gpad, w_t, residual=parked)
            else:
                dx = k_gemm(g, w_t, residual=parked)
        elif ctx.link is not None and ctx.role == 1 and "g" in ctx.link:
            dx = ctx.link.pop("g")                       # (never expected: the sink was armed because x requires grad)
        if need_w:
            dw = _param_grad(_wgrad(g, x), ctx.w_dtype)
        if need_b and ctx.has_bias:
            db = _param_grad(k_colsum(g), ctx.b_dtype)
        return dx, dw, db, None, dres, None, None, None, None, None


# CAMBRIAN_AMD_LINK_RESIDUAL_GRADS=0: autograd sums the two gradients of a block's input itself (A/B runs)
LINK_RESIDUAL_GRADS = L.env_flag("CAMBRIAN_AMD_LINK_RESIDUAL_GRADS", True)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = L.ACT_NONE,
           residual: Optional[torch.Tensor] = None, res_rep: int = 0,
           colscale: Optional[torch.Tensor] = None, heavy: bool = False, link: Optional[dict] = None, role: int = 0) -> torch.Tensor:
    """2-D linear on the HIP GEMM.  x [M,K] -> [M,N].  ``heavy`` marks the KV-side projections (aux projectors, SVA
    K/V projections: M = every tower token, >85 % of the SVA-side FLOPs) — the ones ``fp8_projections`` moves to the
    fp8 MFMA; the query-side GEMMs (M = 576 per image) stay bf16.  ``link`` / ``role``: see LinearFn.forward."""
    return LinearFn.apply(x, weight, bias, act, residual, res_rep, colscale, heavy, link, role)


# ================================================================================================
# autograd: LayerNorm (affine) and the SVA "normalise-only, shared input" variant
# ================================================================================================
class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float):
        g32 = k_cast(gamma, torch.float32)
        b32 = k_cast(beta, torch.float32)
        y, mean, rstd = k_layernorm_fwd(x, g32, b32, eps)
        ctx.save_for_backward(x, g32, mean, rstd)
        ctx.p_dtype = gamma.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g32, mean, rstd = ctx.saved_tensors
        dy = _as_dtype_contig(dy, x.dtype)
        dx, dgamma, dbeta, _ = k_layernorm_bwd(dy, x, mean, rstd, gamma=g32)
        return dx, _param_grad(dgamma, ctx.p_dtype), _param_grad(dbeta, ctx.p_dtype), None


def layernorm(x, gamma, beta, eps: float = 1e-5):
    return LayerNormFn.apply(x, gamma, beta, eps)


DEFER_LN_BWD = L.env_flag("CAMBRIAN_AMD_DEFER_LN_BWD", True)   # (A/B runs: 0 = one LayerNorm backward per SVA layer)
# parked layers per flush (= the 5-layer launches of cmb_layernorm_bwd_multi, CMB_KNOB_LN_MULTI_CHUNK; 0 = only when the
# shared-gradient node runs)
DEFER_LN_FLUSH = int(os.environ.get("CAMBRIAN_AMD_DEFER_LN_FLUSH", "5"))


# the last multi-layer launch of a tower's deferred LayerNorm backward writes d(x) in x's dtype (no separate cast of the fp32
# accumulator); CAMBRIAN_AMD_LN_BWD_FINAL_CAST=0: accumulator + cmb_cast as before (A/B runs)
LN_BWD_FINAL_CAST = L.env_flag("CAMBRIAN_AMD_LN_BWD_FINAL_CAST", True)


class GradAccumulator:
    """fp32 side buffer that the 13 SVA layers' LayerNorm backwards accumulate into (all layers read the
    same aux feature tensor; SURVEY.md §7 "hard parts").

    Round 4: the layers' LayerNorm backwards can be DEFERRED — each SvaNormFn.backward parks (d xh_l, mean_l, rstd_l, pos_l)
    here instead of running, and SharedGradFn.backward (which autograd runs after all of them) does them in ONE pass over x
    (cmb_layernorm_bwd_multi: 32 instead of 156 bytes per element for 13 layers).  The gradients of the position tables come
    out of that pass, so they are returned by SharedGradFn.backward: the tables are formally inputs of shared_grad()
    (``pos_params``) and SvaNormFn returns no gradient for them.  A layer whose table was not announced runs the immediate
    path."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.shape = None
        self.defer = False
        self.pos_index = {}     # id() of an announced position table (the Parameter object) -> its slot in SharedGradFn's inputs
        self.deferred = []      # (dn, x, mean, rstd, add fp32 | None, side, grid_r, slot | -1)
        self.pos_meta = []      # (shape, dtype, needs grad) per announced table
        self.dpos = []          # fp32 table gradients filled by flush()
        self.pos_params = ()    # the announced tables themselves (SvaNormFn.forward: all layers' normalisations in one pass)
        self.fwd_key = None     # (x identity, side, grid_r, eps) of the one multi-layer forward this holder has run
        self.fwd_cache = {}     # slot -> (n, mean, rstd, add) not yet handed to its layer; "nopos" -> the table-less result

    def get(self, rows: int, D: int, device) -> torch.Tensor:
        if self.buf is None:
            self.buf = torch.zeros((rows, D), dtype=torch.float32, device=device)
        return self.buf

    def flush(self, final_dtype: Optional[torch.dtype] = None) -> Optional[torch.Tensor]:
        """Run the parked LayerNorm backwards (one cmb_layernorm_bwd_multi call per window geometry) into the shared fp32
        buffer and release their gradient tensors.  Called by SvaNormFn.backward whenever DEFER_LN_FLUSH layers are parked
        (= the kernel's 5-layer launches: same launches as one call at the end, but at most 5 layers' d(x-hat) — 2.3 GB at
        24 images instead of 5.9 GB — are alive at a time) and by SharedGradFn.backward for the rest."""
        items, self.deferred = self.deferred, []
        if not items:
            return None
        x = items[0][1]
        groups = {}
        for dn, _x, mean, rstd, add, side, grid_r, slot in items:
            if slot >= 0 and self.dpos[slot] is None and self.pos_meta[slot][2]:
                self.dpos[slot] = torch.zeros(self.pos_meta[slot][0], dtype=torch.float32, device=x.device)
            groups.setdefault((side, grid_r) if add is not None else (1, 1), []).append((dn, mean, rstd, add, slot))
        have = self.buf is not None
        if self.buf is None:
            self.buf = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        # ``final_dtype`` (SharedGradFn.backward's last flush): the kernel's last launch writes the finished sum in that dtype —
        # the fp32 accumulator's cast (906 MB read + 453 MB written for the 9216-token tower at 24 images) and the launch's own
        # fp32 write are gone.  Returns that tensor (the accumulator is then stale), else None.
        out = None
        if final_dtype is not None and final_dtype == x.dtype and final_dtype != torch.float32 and len(groups) == 1:
            out = torch.empty((x.shape[0], x.shape[1]), dtype=final_dtype, device=x.device)
        for (side, grid_r), its in groups.items():
            k_layernorm_bwd_multi(x, its, side, grid_r, self.buf, have, self.dpos, dx_out=out)
            have = True
        return out


def k_layernorm_bwd_multi(x: torch.Tensor, items, side: int, grid_r: int, dx: torch.Tensor, accumulate: bool, dadd_out,
                          dx_out: Optional[torch.Tensor] = None):
    """cmb_layernorm_bwd_multi over ``items`` = [(dn, mean, rstd, add | None, slot)]: dx (fp32 [rows, D]) (+)= the summed
    LayerNorm backwards; ``dadd_out[slot]`` (fp32, zero-filled, same shape as the table) receives each layer's table gradient.
    ``dx_out`` (x's dtype, dense [rows, D]): the last launch writes the finished sum THERE instead of updating dx."""
    L.require_gpu(x, dx, dx_out)
    rows, D = x.shape
    if dx_out is not None and (dx_out.dtype != x.dtype or not dx_out.is_contiguous() or tuple(dx_out.shape) != (rows, D)):
        raise L.CambrianAmdError("layernorm_bwd_multi: dx_out must be a dense [rows, D] tensor of x's dtype")
    for lo in range(0, len(items), L.LN_MULTI_MAX):
        chunk = items[lo:lo + L.LN_MULTI_MAX]
        d = L.LnMultiDesc()
        d.dtype, d.layers = L.dtype_code(x.dtype), len(chunk)
        d.x, d.ldx, d.rows, d.D, d.side, d.grid_r = x.data_ptr(), x.stride(0), rows, D, side, grid_r
        for i, (dn, mean, rstd, add, slot) in enumerate(chunk):
            if dn.dtype != x.dtype or not dn.is_contiguous() or tuple(dn.shape) != (rows, D):
                raise L.CambrianAmdError("layernorm_bwd_multi: every gradient must be a dense [rows, D] tensor of x's dtype")
            d.dy[i], d.mean[i], d.rstd[i] = dn.data_ptr(), mean.data_ptr(), rstd.data_ptr()
            d.add[i] = None if add is None else add.data_ptr()
            d.dadd[i] = None if (add is None or slot < 0 or dadd_out[slot] is None) else dadd_out[slot].data_ptr()
        d.dx, d.lddx, d.accumulate = dx.data_ptr(), dx.stride(0), 1 if (accumulate or lo > 0) else 0
        d.dx_out = dx_out.data_ptr() if (dx_out is not None and lo + L.LN_MULTI_MAX >= len(items)) else None
        ws = torch.empty((max(L.load().cmb_layernorm_bwd_multi_workspace(C.byref(d)), 1),), dtype=torch.float32,
                         device=x.device)   # partial rows of the fixed-order table-gradient sums
        d.workspace, d.workspace_floats = ws.data_ptr(), ws.numel()
        L.call("cmb_layernorm_bwd_multi", C.byref(d), device=x.device)


class SharedGradFn(torch.autograd.Function):
    """Identity whose backward hands out the accumulator filled by the consumers (which themselves return
    no gradient for this tensor).  Autograd runs this node only after every consumer node has run, because
    dependencies are counted on graph edges, not on defined gradients.  ``pos_params``: the position tables of the SVA
    layers that will normalise this tensor (GradAccumulator: deferred LayerNorm backwards)."""

    @staticmethod
    def forward(ctx, x, holder: GradAccumulator, *pos_params):
        ctx.holder = holder
        holder.shape = x.shape
        holder.defer = DEFER_LN_BWD
        holder.deferred = []
        holder.pos_meta = [(tuple(p.shape), p.dtype, bool(ctx.needs_input_grad[2 + i])) for i, p in enumerate(pos_params)]
        holder.dpos = [None] * len(pos_params)
        ctx.x_dtype = x.dtype
        ctx.n_pos = len(pos_params)
        ctx.set_materialize_grads(False)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        h = ctx.holder
        done = h.flush(final_dtype=ctx.x_dtype if (g is None and LN_BWD_FINAL_CAST) else None)
        buf, h.buf = h.buf, None
        dpos = [None if t is None else (t if h.pos_meta[i][1] == torch.float32 else t.to(h.pos_meta[i][1]))
                for i, t in enumerate(h.dpos)] + [None] * (ctx.n_pos - len(h.dpos))
        h.dpos = [None] * ctx.n_pos
        if done is not None:     # the last multi-layer launch already wrote d(x) in x's dtype
            return (done.view(h.shape), None, *dpos)
        if buf is None:
            return (g, None, *dpos)
        if g is not None:
            buf = buf + g.to(torch.float32).reshape(buf.shape)
        return (k_cast(buf, ctx.x_dtype).view(h.shape), None, *dpos)


def shared_grad(x: torch.Tensor, holder: GradAccumulator, pos_params=()) -> torch.Tensor:
    # tables are recognised by the IDENTITY of the tensor object handed to sva_norm(), not by their storage address: a
    # sharded / re-materialised parameter (ZeRO-3: storage.resize_(0), every released table at data_ptr 0) keeps its id but
    # not its address, and two tables must never alias
    pos_params = tuple(pos_params)
    index = {id(p): i for i, p in enumerate(pos_params)}
    if len(index) != len(pos_params):
        raise L.CambrianAmdError("shared_grad: the same position table was announced twice")
    holder.pos_index = index
    holder.pos_params = pos_params
    holder.fwd_key, holder.fwd_cache = None, {}
    return SharedGradFn.apply(x, holder, *pos_params)


# The 13 SVA layers normalise the SAME aux features; only the position table differs (vision_sampler.py:304-309), and a one-key
# tower has no table at all: its 13 normalisations are one and the same tensor.  Round 6: the first layer that asks runs
# cmb_layernorm_fwd_multi over every table announced to shared_grad() (x read once instead of 13 times) and parks the other
# layers' results in the holder; a table-less result is computed once per holder and shared.  Bit-identical to the per-layer
# launches.  A slot is served from the multi-layer pass at most once per holder: re-computation forwards (activation
# checkpointing) and geometries that differ from the first request's take the per-layer kernel.  The normalised tensors were
# alive until the backward anyway (the attention core saves them).  CAMBRIAN_AMD_LN_FWD_MULTI=0: per-layer launches (A/B runs).
LN_FWD_MULTI = L.env_flag("CAMBRIAN_AMD_LN_FWD_MULTI", True)


def _materialised(p: torch.Tensor) -> bool:
    return p.is_cuda and p.numel() > 0 and p.untyped_storage().size() >= (p.storage_offset() + p.numel()) * p.element_size()


def _sva_norm_forward(x, add, holder: "GradAccumulator", side: int, grid_r: int, eps: float, pos_key):
    if not (LN_FWD_MULTI and x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.shape[1] <= 1024 and holder.pos_index is not None):
        return k_layernorm_fwd(x, None, None, eps, add=add, side=side, grid_r=grid_r)
    xid = (x.data_ptr(), x._version, tuple(x.shape), x.dtype)
    if add is None:   # every layer's normalisation of a table-less tower is the same tensor: one launch per holder
        hit = holder.fwd_cache.get("nopos")
        if hit is None or hit[0] != (xid, eps):
            hit = ((xid, eps), k_layernorm_fwd(x, None, None, eps))
            holder.fwd_cache["nopos"] = hit
        n, mean, rstd = hit[1]
        return n.detach(), mean, rstd          # a fresh tensor object per autograd node, the same storage
    slot = holder.pos_index.get(pos_key, -1)
    key = (xid, side, grid_r, eps)
    if slot >= 0 and holder.fwd_key is None and len(holder.pos_params) > 1 and all(_materialised(p) for p in holder.pos_params):
        adds = [k_cast(p.detach(), torch.float32) for p in holder.pos_params]
        if all(tuple(a.shape) == (grid_r * grid_r, x.shape[1]) for a in adds):
            holder.fwd_key = key
            for i, res in enumerate(k_layernorm_fwd_multi(x, adds, eps, side, grid_r)):
                holder.fwd_cache[i] = res
    if slot >= 0 and holder.fwd_key == key:
        hit = holder.fwd_cache.pop(slot, None)
        if hit is not None:
            return hit
    return k_layernorm_fwd(x, None, None, eps, add=add, side=side, grid_r=grid_r)


class SvaNormFn(torch.autograd.Function):
    """n = (x + pos[window_pos]) normalised without affine (the K- and V-LayerNorm affines of
    vision_sampler.py:173-174 are folded into the projection weights).  The gradient w.r.t. x goes into
    the shared fp32 accumulator instead of being returned."""

    @staticmethod
    def forward(ctx, x, pos, holder: GradAccumulator, side: int, grid_r: int, eps: float, pos_key=None):
        add = None if pos is None else k_cast(pos, torch.float32)
        n, mean, rstd = _sva_norm_forward(x, add, holder, side, grid_r, eps, pos_key)
        ctx.holder, ctx.side, ctx.grid_r = holder, side, grid_r
        ctx.pos_key = pos_key          # id() of the table object the caller passed (sva_norm)
        ctx.pos_dtype = None if pos is None else pos.dtype
        ctx.has_pos = pos is not None
        if pos is None:
            ctx.save_for_backward(x, mean, rstd)
        else:
            ctx.save_for_backward(x, mean, rstd, add)
        return n

    @staticmethod
    def backward(ctx, dn):
        if ctx.has_pos:
            x, mean, rstd, add = ctx.saved_tensors
        else:
            (x, mean, rstd), add = ctx.saved_tensors, None
        dn = _as_dtype_contig(dn, x.dtype)
        need_x, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        h = ctx.holder
        if need_x and h.defer and x.is_contiguous() and x.shape[1] <= 1024:
            slot = -1 if add is None else h.pos_index.get(ctx.pos_key, -2)
            if slot != -2 and not (h.deferred and h.deferred[0][1].data_ptr() != x.data_ptr()):
                # parked: SharedGradFn.backward runs every layer's LayerNorm backward in one pass and returns d(pos)
                h.deferred.append((dn, x, mean, rstd, add, ctx.side, ctx.grid_r, slot))
                if DEFER_LN_FLUSH > 0 and len(h.deferred) >= DEFER_LN_FLUSH:
                    h.flush()
                return None, None, None, None, None, None, None
        dpos = None
        if need_x:
            acc = h.get(x.shape[0], x.shape[1], x.device)
            _, _, _, dpos = k_layernorm_bwd(dn, x, mean, rstd, add=add, side=ctx.side, grid_r=ctx.grid_r, dx_acc=acc,
                                            want_dadd=need_pos)
        elif need_pos and add is not None:
            _, _, _, dpos = k_layernorm_bwd(dn, x, mean, rstd, add=add, side=ctx.side, grid_r=ctx.grid_r)
        return None, _param_grad(dpos, ctx.pos_dtype), None, None, None, None, None


def sva_norm(x, pos, holder, side, grid_r, eps=1e-5):
    return SvaNormFn.apply(x, pos, holder, side, grid_r, eps, None if pos is None else id(pos))


# ================================================================================================
# autograd: K|V weight folding of one tower (vision_sampler.py:173-174,188-189)
# ================================================================================================
class FoldKVFn(torch.autograd.Function):
    """(Wk, gk, bk, Wv, gv, bv) -> ([Wk*gk ; Wv*gv] [2H, K], [Wk@bk ; Wv@bv] [2H]) in fp32, two HIP launches per step."""

    @staticmethod
    def forward(ctx, wk, gk, bk, wv, gv, bv):
        ts = [t.detach().contiguous() for t in (wk, gk, bk, wv, gv, bv)]
        for t in ts:
            L.require_gpu(t)
            if t.dtype != torch.float32:
                raise L.CambrianAmdError("fold_kv: fp32 tensors expected (ops.fold_kv up-casts other parameter dtypes)")
        w, b = k_fold_kv_fwd(ts)
        ctx.save_for_backward(*ts)
        return w, b

    @staticmethod
    def backward(ctx, dw, db):
        ts = ctx.saved_tensors
        H, K = ts[0].shape
        dev = ts[0].device
        dw = torch.zeros((2 * H, K), dtype=torch.float32, device=dev) if dw is None else dw.contiguous().float()
        db = torch.zeros((2 * H,), dtype=torch.float32, device=dev) if db is None else db.contiguous().float()
        return tuple(k_fold_kv_bwd(dw, db, ts))


def fold_kv(wk, gk, bk, wv, gv, bv):
    """Folded K|V weight / bias in fp32.  Parameters that are not fp32 masters (a module moved with ``.to(bfloat16)`` /
    ``.half()``) are up-cast by autograd-tracked ``.float()`` first, as the torch expression this replaces did."""
    ts = [t if t.dtype == torch.float32 else t.float() for t in (wk, gk, bk, wv, gv, bv)]
    w, b = FoldKVFn.apply(*ts)
    prepare_step_weight(w)   # (inside a training window: the bf16 copies the consuming linears would otherwise make per use)
    return w, b


# ================================================================================================
# autograd: SVA attention core
# ================================================================================================
class SvaAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, B: int, qside: int, heads: int, hd: int, r_list, masks, window_major: bool, *kvs):
        out, lse = k_sva_attn_fwd(q, list(kvs), masks, r_list, B, qside, heads, hd, window_major)
        ctx.cfg = (B, qside, heads, hd, tuple(r_list), window_major)
        ctx.masks = masks
        ctx.save_for_backward(q, out, lse, *kvs)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, out, lse, *kvs = ctx.saved_tensors
        B, qside, heads, hd, r_list, window_major = ctx.cfg
        dout = _as_dtype_contig(dout, q.dtype)
        dq, dkvs = k_sva_attn_bwd(dout, q, kvs, ctx.masks, list(r_list), out, lse, B, qside, heads, hd, window_major)
        return (dq, None, None, None, None, None, None, None, *dkvs)


def sva_attention(q, kvs: Sequence[torch.Tensor], masks, r_list, B, qside, heads=16, hd=64, window_major=False):
    return SvaAttnFn.apply(q, B, qside, heads, hd, list(r_list), masks, window_major, *kvs)


# ================================================================================================
# absorbed K / V projections of the windowed tower (csrc/sva_absorbed.hip)
# ================================================================================================
def k_gemm_batched(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, batch: int, M: int, N: int, K: int, lda: int,
                   ldb: int, ldc: int, a_bs: int, b_bs: int, c_bs: int, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``batch`` independent C_z[M,N] = A_z[M,K] @ B_z[N,K]^T in one launch (cmb_gemm, 128 x 128 tile): problem z reads
    A + z*a_bs (row stride lda), B + z*b_bs (row stride ldb) and writes C + z*c_bs (row stride ldc), all in elements of
    the tensors' dtype (``out`` may be fp32 for bf16 operands).  The per-head GEMMs of the absorbed SVA projections."""
    L.require_gpu(a, w, out)
    if a.dtype != w.dtype:
        raise L.CambrianAmdError("batched gemm operand dtypes differ")
    if residual is not None:   # laid out as ``out`` (row stride ldc, batch stride c_bs), the operands' dtype
        L.require_gpu(residual)
        if residual.dtype != a.dtype or out.dtype != a.dtype or residual.stride(-1) != 1 or residual.stride(0) != ldc \
                or residual.data_ptr() % 16:
            raise L.CambrianAmdError("batched gemm residual must have the operands' dtype and the output's layout")
    d, _ = _gemm_desc(L.dtype_code(a.dtype), M, N, K, a, L.identity_map(lda), w, ldb, out, L.identity_map(ldc), residual=residual,
                      r_map=L.identity_map(ldc), batch=(batch, a_bs, b_bs, c_bs))
    _gemm_launch("cmb_gemm", (d,), a.device, f"cmb_gemm(batch={batch}, M={M}, N={N}, K={K})",
                 GEMM_PROFILE if not GEMM_PROFILE_TILE else None,
                 lambda lib: (2.0 * batch * M * N * K, a.dtype, 1, 128, (M, N, K, L.ACT_NONE, out.dtype == torch.float32),
                              lib.cmb_gemm_last_kernel(), batch))
    return out


def _per_head_wgrad(x: torch.Tensor, dy: torch.Tensor, heads: int, hd: int, Cin: int) -> torch.Tensor:
    """dW[h*hd + j, :] = sum_q x[q, h*hd + j] dy[q, h, :]  ([heads*hd, Cin], fp32) — the weight gradient of the per-head
    projections.  bf16: one batched split-K cmb_gemm_tn on the operands as they lie; other dtypes (the fp32 parity path):
    transposed copies and one NT GEMM per head (cmb_gemm_tn is a bf16 kernel)."""
    Bq = x.shape[0]
    dw = torch.empty((heads * hd, Cin), dtype=torch.float32, device=x.device)
    if x.dtype == torch.bfloat16:
        k_gemm_tn(x, dy.view(Bq, heads * Cin), out=dw, M=hd, N=Cin, batch=heads, a_bs=hd, b_bs=Cin, c_bs=hd * Cin, ldc=Cin,
                  split_k=_tn_splits(hd, Cin, Bq, heads))
        return dw
    m_pad = pad_to(Bq, _kstep(x.dtype))
    x_t = k_transpose(x, m_pad)                                      # [heads*hd, m_pad]
    dy_t = k_transpose(dy.view(Bq, heads * Cin), m_pad)              # [heads*Cin, m_pad]
    for h in range(heads):
        k_gemm(x_t[h * hd:(h + 1) * hd], dy_t[h * Cin:(h + 1) * Cin], out=dw[h * hd:(h + 1) * hd])
    return dw


class HeadExpandFn(torch.autograd.Function):
    """U[q, h, :] = x[q, h*hd:(h+1)*hd] @ W[h*hd:(h+1)*hd, :]   (x [Bq, H*hd], W [H*hd, Cin] -> U [Bq, H, Cin]): the K
    projection of the windowed tower applied to the QUERY (U = W_k,h^T q_h) and, with x = d(o), the V projection's backward
    (d Xb = W_v,h^T d o_h).  H GEMMs with K = hd = 64 in one batched launch; backward: dx_h = dU_h W_h^T (N = 64),
    dW_h = x_h^T dU_h (M = 64, contraction over the queries: cmb_gemm_tn, batched)."""

    @staticmethod
    def forward(ctx, x, w, heads: int):
        Bq, C = x.shape
        hd, Cin = C // heads, w.shape[1]
        prep = prepared_weight(w, x.dtype)
        if prep is not None and prep[1].shape[1] == C:
            w_c, w_t = prep
        else:
            w_c = k_cast(w, x.dtype)
            w_t = k_transpose(w_c, C)                                # [Cin, C]: rows c, the head's 64 inputs contiguous
        U = torch.empty((Bq, heads, Cin), dtype=x.dtype, device=x.device)
        xc = x if x.is_contiguous() else x.contiguous()
        k_gemm_batched(xc, w_t, U, batch=heads, M=Bq, N=Cin, K=hd, lda=C, ldb=w_t.stride(0), ldc=heads * Cin, a_bs=hd, b_bs=hd,
                       c_bs=Cin)
        ctx.save_for_backward(xc, w_c)
        ctx.heads, ctx.w_dtype = heads, w.dtype
        return U

    @staticmethod
    def backward(ctx, dU):
        x, w_c = ctx.saved_tensors
        heads = ctx.heads
        Bq, C = x.shape
        hd, Cin = C // heads, w_c.shape[1]
        dU = _as_dtype_contig(dU, x.dtype)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((Bq, C), dtype=x.dtype, device=x.device)
            k_gemm_batched(dU, w_c, dx, batch=heads, M=Bq, N=hd, K=Cin, lda=heads * Cin, ldb=Cin, ldc=C, a_bs=Cin,
                           b_bs=hd * Cin, c_bs=hd)
        if ctx.needs_input_grad[1]:
            dw = _param_grad(_per_head_wgrad(x, dU, heads, hd, Cin), ctx.w_dtype)
        return dx, dw, None


class HeadContractFn(torch.autograd.Function):
    """y[q, h*hd + j] = Xb[q, h, :] . W[h*hd + j, :]   (Xb [Bq, H, Cin], W [H*hd, Cin] -> y [Bq, H*hd]): the V projection of
    the windowed tower applied to the attention-weighted token mix (o_h = W_v,h Xb_h).  H GEMMs with N = hd = 64 in one
    batched launch; backward: dXb_h = dy_h W_h (K = 64), dW_h = dy_h^T Xb_h."""

    @staticmethod
    def forward(ctx, xb, w, heads: int, addend=None):
        """``addend`` [Bq, C] (optional): y = addend + the per-head products, added in the GEMM's epilogue (the one-key towers'
        part of the attention output: no separate add over [Bq, C])."""
        Bq, H, Cin = xb.shape
        C = w.shape[0]
        hd = C // heads
        prep = prepared_weight(w, xb.dtype)
        w_c, ctx.w_t = prep if (prep is not None and prep[1].shape[1] == C) else (k_cast(w, xb.dtype), None)
        xbc = xb if xb.is_contiguous() else xb.contiguous()
        y = torch.empty((Bq, C), dtype=xb.dtype, device=xb.device)
        if addend is not None:
            addend = _as_dtype_contig(addend, xb.dtype)
        k_gemm_batched(xbc, w_c, y, batch=heads, M=Bq, N=hd, K=Cin, lda=heads * Cin, ldb=Cin, ldc=C, a_bs=Cin,
                       b_bs=hd * Cin, c_bs=hd, residual=addend)
        ctx.save_for_backward(xbc, w_c)
        ctx.heads, ctx.w_dtype = heads, w.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, w_c = ctx.saved_tensors
        heads = ctx.heads
        Bq, H, Cin = xb.shape
        C = w_c.shape[0]
        hd = C // heads
        dy = _as_dtype_contig(dy, xb.dtype)
        dxb = dw = None
        if ctx.needs_input_grad[0]:
            w_t = ctx.w_t if ctx.w_t is not None else k_transpose(w_c, C)   # [Cin, C]
            dxb = torch.empty((Bq, heads, Cin), dtype=xb.dtype, device=xb.device)
            k_gemm_batched(dy, w_t, dxb, batch=heads, M=Bq, N=Cin, K=hd, lda=C, ldb=w_t.stride(0), ldc=heads * Cin, a_bs=hd,
                           b_bs=hd, c_bs=Cin)
        if ctx.needs_input_grad[1]:
            dw = _param_grad(_per_head_wgrad(dy, xb, heads, hd, Cin), ctx.w_dtype)
        if len(ctx.needs_input_grad) < 4:     # called without an addend
            return dxb, dw, None
        return dxb, dw, None, (dy if ctx.needs_input_grad[3] else None)


def _fill_sva_abs(d, q, kvs, masks, xhat, mask_a, ra, U, bk, bv, B, qside, window_major):
    d.B, d.qside, d.heads, d.hd = B, qside, 16, 64
    d.dtype = L.dtype_code(q.dtype)
    d.ntowers, d.window_major, d.ra = len(kvs), 1 if window_major else 0, ra
    d.q, d.ldq = q.data_ptr(), q.stride(0)
    for i, kv in enumerate(kvs):
        d.r[i] = 1
        d.kv[i], d.ldkv[i] = kv.data_ptr(), kv.stride(0)
        d.mask[i] = None if masks[i] is None else masks[i].data_ptr()
    d.xhat, d.ldx = xhat.data_ptr(), xhat.stride(0)
    d.mask_a = None if mask_a is None else mask_a.data_ptr()
    d.U, d.bk, d.bv = U.data_ptr(), bk.data_ptr(), bv.data_ptr()


def k_sva_abs_fwd(q, kvs, masks, xhat, mask_a, ra, U, bk, bv, B, qside, window_major):
    """cmb_sva_abs_fwd -> (out [Bq, 1024], xbar [Bq, 16, 1024], m3 fp32 [Bq, 16], P fp32 [Bq, 16, 20])."""
    Bq = q.shape[0]
    out = torch.empty((Bq, 1024), dtype=q.dtype, device=q.device)
    xbar = torch.empty((Bq, 16, 1024), dtype=q.dtype, device=q.device)
    m3 = torch.empty((Bq, 16), dtype=torch.float32, device=q.device)
    P = torch.empty((Bq, 16, 20), dtype=torch.float32, device=q.device)   # [0, 4) direct keys, [4, 20) window tokens
    d = L.SvaAbsDesc()
    _fill_sva_abs(d, q, kvs, masks, xhat, mask_a, ra, U, bk, bv, B, qside, window_major)
    d.out, d.ldo, d.xbar, d.m3, d.P = out.data_ptr(), out.stride(0), xbar.data_ptr(), m3.data_ptr(), P.data_ptr()
    L.call("cmb_sva_abs_fwd", C.byref(d), device=q.device)
    return out, xbar, m3, P


def k_sva_abs_bwd(dout, dxbar, q, kvs, masks, xhat, mask_a, ra, U, bk, bv, P, B, qside, window_major):
    """cmb_sva_abs_bwd -> (dq, [dK|dV rows per direct tower], dU, d(cb) fp32 [Bq, 16], d xhat)."""
    Bq, dev = q.shape[0], q.device
    dq = torch.empty_like(q)
    dkvs = [torch.empty_like(kv) for kv in kvs]
    dU = torch.empty_like(U)
    dcb = torch.empty((Bq, 16), dtype=torch.float32, device=dev)
    dxhat = torch.empty((xhat.shape[0], 1024), dtype=q.dtype, device=dev)
    d = L.SvaAbsDesc()
    _fill_sva_abs(d, q, kvs, masks, xhat, mask_a, ra, U, bk, bv, B, qside, window_major)
    # (the forward outputs are not read by the backward kernel, but the descriptor's forward fields must be set)
    d.out, d.ldo, d.xbar, d.m3, d.P = dq.data_ptr(), dq.stride(0), dU.data_ptr(), dcb.data_ptr(), P.data_ptr()
    d.dout, d.lddo, d.dxbar = dout.data_ptr(), dout.stride(0), dxbar.data_ptr()
    d.dq, d.lddq = dq.data_ptr(), dq.stride(0)
    for i, t in enumerate(dkvs):
        d.dkv[i] = t.data_ptr()
    d.dU, d.dcb, d.dxhat, d.lddx = dU.data_ptr(), dcb.data_ptr(), dxhat.data_ptr(), dxhat.stride(0)
    L.call("cmb_sva_abs_bwd", C.byref(d), device=dev)
    return dq, dkvs, dU, dcb, dxhat


class SvaAbsorbedFn(torch.autograd.Function):
    """cmb_sva_abs_fwd / _bwd: per query the joint softmax over the one-key towers' projected K|V rows and the windowed
    tower's tokens (scored against U, plus b_k . q), returning (the direct towers' part of the output + m3 b_v [Bq, 1024],
    Xb [Bq, 16, 1024])."""

    @staticmethod
    def forward(ctx, q, U, bk, bv, xhat, B: int, qside: int, ra: int, masks, mask_a, window_major: bool, *kvs):
        L.require_gpu(q, U, bk, bv, xhat, *kvs)
        Bq = B * qside * qside
        if q.dtype not in (torch.bfloat16, torch.float32) or tuple(q.shape) != (Bq, 1024) or tuple(U.shape) != (Bq, 16, 1024):
            raise L.CambrianAmdError("absorbed SVA attention: bf16 / fp32, 16 heads x 64, 1024-wide features")
        if any(t.dtype != q.dtype for t in (U, xhat, *kvs)):
            raise L.CambrianAmdError("absorbed SVA attention: q, U, xhat and the K|V rows must share one dtype")
        if xhat.shape[0] != B * (qside * ra) ** 2 or xhat.shape[1] != 1024 or xhat.stride(1) != 1:
            raise L.CambrianAmdError("absorbed SVA attention: xhat must be [B*(qside*ra)^2, 1024]")
        # dense rows: the backward kernel writes dK|dV with the K|V row stride (cmb_sva_abs_desc has no separate lddkv) into
        # torch.empty_like(kv), which is contiguous whatever kv's strides were
        kvs = [kv.contiguous() for kv in kvs]
        Uc = U.contiguous()
        bkc, bvc = bk.detach().to(torch.float32).contiguous(), bv.detach().to(torch.float32).contiguous()
        out, xbar, m3, P = k_sva_abs_fwd(q, kvs, masks, xhat, mask_a, ra, Uc, bkc, bvc, B, qside, window_major)
        ctx.cfg = (B, qside, ra, window_major)
        ctx.masks, ctx.mask_a = masks, mask_a
        ctx.b_dtypes = (bk.dtype, bv.dtype)
        ctx.save_for_backward(q, Uc, bkc, bvc, xhat, P, m3, *kvs)
        ctx.mark_non_differentiable(m3)
        return out, xbar, m3

    @staticmethod
    def backward(ctx, dout, dxbar, _dm3):
        q, U, bk, bv, xhat, P, m3, *kvs = ctx.saved_tensors
        B, qside, ra, window_major = ctx.cfg
        dout = torch.zeros_like(q) if dout is None else _as_dtype_contig(dout, q.dtype)
        dxbar = torch.zeros_like(U) if dxbar is None else _as_dtype_contig(dxbar, q.dtype)
        dq, dkvs, dU, dcb, dxhat = k_sva_abs_bwd(dout, dxbar, q, kvs, ctx.masks, xhat, ctx.mask_a, ra, U, bk, bv, P, B, qside,
                                                 window_major)
        dbk = dbv = None
        if ctx.needs_input_grad[2]:   # d b_k[c] = sum_q d(cb)[q, h(c)] q[q, c]
            dbk = k_colsum(q, row_scale=dcb, group=64).to(ctx.b_dtypes[0])
        if ctx.needs_input_grad[3]:   # d b_v[c] = sum_q m3[q, h(c)] d out[q, c]
            dbv = k_colsum(dout, row_scale=m3, group=64).to(ctx.b_dtypes[1])
        return (dq, dU, dbk, dbv, dxhat, None, None, None, None, None, None, *dkvs)


# CAMBRIAN_AMD_FUSE_CONTRACT_ADD=1: the one-key towers' output is added to the windowed tower's W_v Xb inside the per-head GEMM's
# epilogue (a batched residual) instead of by an ATen add over [Bq, 1024].  Measured neutral (profiles/r06_lab.md section 25): off.
FUSE_CONTRACT_ADD = L.env_flag("CAMBRIAN_AMD_FUSE_CONTRACT_ADD", False)


def sva_absorbed_attention(qh, kvs_direct, masks_direct, xhat, mask_a, ra: int, wk, bk, wv, bv, B: int, qside: int,
                           window_major: bool = False) -> torch.Tensor:
    """The SVA attention core with the windowed tower's K / V projections absorbed (csrc/sva_absorbed.hip): ``qh`` [Bq, 1024]
    projected queries; ``kvs_direct`` K|V rows [Bq, 2048] of the one-key towers with their uint8 masks [Bq] (or None);
    ``xhat`` the windowed tower's normalised tokens; (wk, bk, wv, bv) its folded projection [1024, 1024] / [1024] (fp32,
    autograd-tracked).  Returns the attention output [Bq, 1024] (before o_proj), identical to ``sva_attention`` on the K|V
    rows ``xhat @ [wk; wv]^T + [bk; bv]``."""
    U = HeadExpandFn.apply(qh, wk, 16)                                           # [Bq, 16, 1024]
    out_d, xbar, _ = SvaAbsorbedFn.apply(qh, U, bk, bv, xhat, B, qside, ra, list(masks_direct), mask_a, window_major, *kvs_direct)
    if FUSE_CONTRACT_ADD:
        return HeadContractFn.apply(xbar, wv, 16, out_d)                          # out_d + W_v,h Xb, added in the GEMM's epilogue
    return out_d + HeadContractFn.apply(xbar, wv, 16)                             # + W_v,h Xb


# ================================================================================================
# autograd: token mean, embedding splice
# ================================================================================================
class TokenMeanFn(torch.autograd.Function):
    """[B,T,D] -> [B,D] mean over tokens (cambrian_arch.py:377).  If ``holder`` is given the gradient is
    accumulated into the shared fp32 buffer of the aux feature instead of being returned."""

    @staticmethod
    def forward(ctx, x, holder: Optional[GradAccumulator]):
        B, T, D = x.shape
        xc = x if x.is_contiguous() else x.contiguous()
        out = k_token_mean(xc)
        ctx.shape = (B, T, D)
        ctx.holder = holder
        ctx.x_dtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        B, T, D = ctx.shape
        g = _as_dtype_contig(g, ctx.x_dtype)
        if ctx.holder is not None:
            acc = ctx.holder.get(B * T, D, g.device)
        else:
            acc = torch.zeros((B * T, D), dtype=torch.float32, device=g.device)
        k_token_mean_bwd(g, B, T, D, acc)
        if ctx.holder is not None:
            return None, None
        return k_cast(acc, ctx.x_dtype).view(B, T, D), None


def token_mean(x, holder=None):
    return TokenMeanFn.apply(x, holder)


class EmbedSpliceFn(torch.autograd.Function):
    """inputs_embeds of the static path: embedding gather + newline column + visual splice in one kernel
    (cambrian_arch.py:413-420,457-490).  Gradients flow to feat and newline, and — finetune stage — to the embedding table
    (frozen in the pre-training stage: train_fsdp.py:1677-1685)."""

    @staticmethod
    def forward(ctx, ids, table, feat, newline, side: int, image_token: int):
        B, S = ids.shape
        V, H = table.shape
        dt = feat.dtype
        tab = k_cast(table, dt)
        nl = k_cast(newline, dt)
        featc = feat if feat.is_contiguous() else feat.contiguous()
        idc = ids if ids.is_contiguous() else ids.contiguous()
        out, pos = k_embed_splice_fwd(idc, tab, featc, nl, side, image_token)
        ctx.cfg = (B, S, H, side, dt, newline.dtype, V, table.dtype, image_token)
        ctx.save_for_backward(pos, idc)
        ctx.mark_non_differentiable(pos)
        return out, pos

    @staticmethod
    def backward(ctx, dout, _dpos):
        pos, ids = ctx.saved_tensors
        B, S, H, side, dt, nl_dtype, V, tab_dtype, image_token = ctx.cfg
        dout = _as_dtype_contig(dout, dt)
        dtable = None
        if ctx.needs_input_grad[1]:
            # finetune stage (the embedding table trains): nn.Embedding's backward for the TEXT rows — every position outside
            # the visual span [p_b, p_b + side (side + 1)) gathers table[ids'] (stock index_add_, fp32 accumulation)
            t = torch.arange(S, device=dout.device)[None]
            p_b = pos.to(torch.int64)[:, None]
            text = (p_b < 0) | (t < p_b) | (t >= p_b + side * (side + 1))
            # the same id map as embed_splice_fwd_kernel: the image token -> row 0, everything else clamped into the table
            # (a pad / ignore id such as -100 reads row 0 in the forward; it must add to row 0 here, not assert)
            idx = torch.where(ids == image_token, torch.zeros_like(ids), ids).clamp_(0, V - 1)[text]
            dtable = torch.zeros((V, H), dtype=torch.float32, device=dout.device)
            dtable.index_add_(0, idx, dout[text].float())
            dtable = dtable.to(tab_dtype)
        dfeat, dnl = k_embed_splice_bwd(dout, pos, side)
        return None, dtable, dfeat, dnl.to(nl_dtype), None, None


def embed_splice(ids, table, feat, newline, side: int, image_token: int = -200):
    return EmbedSpliceFn.apply(ids, table, feat, newline, side, image_token)


# ================================================================================================
# autograd: RMSNorm / RoPE (LLM side)
# ================================================================================================
class RmsNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps: float):
        shape = x.shape
        D = shape[-1]
        x2 = x.reshape(-1, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        w32 = k_cast(weight, torch.float32)
        y, rstd = k_rmsnorm_fwd(x2, w32, eps)
        ctx.save_for_backward(x2, w32, rstd)
        ctx.shape, ctx.w_dtype = shape, weight.dtype
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w32, rstd = ctx.saved_tensors
        rows, D = x2.shape
        dy2 = _as_dtype_contig(dy.reshape(rows, D), x2.dtype)
        dx, dw = k_rmsnorm_bwd(dy2, x2, w32, rstd, want_dw=ctx.needs_input_grad[1])
        return dx.view(ctx.shape), _param_grad(dw, ctx.w_dtype), None


def rmsnorm(x, weight, eps: float = 1e-6):
    return RmsNormFn.apply(x, weight, eps)


class RmsNormForkFn(torch.autograd.Function):
    """(x, rmsnorm(x) * w): the decoder layer's "normalise for the attention branch AND keep x for the skip connection" as
    ONE autograd node.  With two consumers of x (RmsNormFn and the later residual add) autograd sums their two dense
    [tokens, hidden] gradients with an extra elementwise pass per layer (33 x 131 us per step at 16 x 2048 tokens); here
    the skip path's gradient enters the RMSNorm backward kernel as its additive term (cmb_rmsnorm_bwd_add): one pass."""

    @staticmethod
    def forward(ctx, x, weight, eps: float):
        # RmsNormFn's forward on this node's ctx (same launch, same saved tensors); x returned as is: autograd hands out an alias
        return x, RmsNormFn.forward(ctx, x, weight, eps)

    @staticmethod
    def backward(ctx, g_x, g_y):
        x2, w32, rstd = ctx.saved_tensors
        rows, D = x2.shape
        if g_y is None:
            return g_x, None, None
        gy = _as_dtype_contig(g_y.reshape(rows, D), x2.dtype)
        gs = None if g_x is None else _as_dtype_contig(g_x.reshape(rows, D), x2.dtype)
        # (a trainable norm weight — finetune stage — takes the two-pass kernel that also reduces dw: k_rmsnorm_bwd)
        dx, dw = k_rmsnorm_bwd(gy, x2, w32, rstd, add=gs, want_dw=ctx.needs_input_grad[1])
        out = dx.view(ctx.shape)
        # a buffer this call allocated and hands to exactly one receiver: whoever gets THIS object as its incoming gradient may
        # write into it (ScatterQueryRowsFn.backward: no 400 MB clone per in-LLM SVA layer).  Autograd's own sums of several
        # gradients are new tensors without the mark.
        out._cmb_exclusive = True
        return out, _param_grad(dw, ctx.w_dtype), None


def rmsnorm_fork(x, weight, eps: float = 1e-6):
    """(x, rmsnorm(x) * weight) — see RmsNormForkFn.  Use the RETURNED x for the skip connection."""
    return RmsNormForkFn.apply(x, weight, eps)


def rope_table(position_ids: torch.Tensor, head_dim: int, base: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin [ntok, head_dim/2] fp32 for position_ids [B,S] (built once per forward)."""
    L.require_gpu(position_ids)
    pid = position_ids.reshape(-1).to(torch.int64).contiguous()
    ntok = pid.numel()
    cos = torch.empty((ntok, head_dim // 2), dtype=torch.float32, device=pid.device)
    sin = torch.empty_like(cos)
    L.call("cmb_rope_table", pid.data_ptr(), ntok, head_dim, base, cos.data_ptr(), sin.data_ptr(), device=pid.device)
    return cos, sin


class RopeFn(torch.autograd.Function):
    """x [ntok, H, Dh] (contiguous) rotated out of place; the backward is the inverse rotation."""

    @staticmethod
    def forward(ctx, x, cos, sin):
        ctx.save_for_backward(cos, sin)
        return k_rope_apply(x.contiguous().clone(), cos, sin)

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        return k_rope_apply(dy.contiguous().clone(), cos, sin, inverse=True), None, None


def rope(x, cos, sin):
    return RopeFn.apply(x, cos, sin)


# ================================================================================================
# autograd: row gather / scatter of the in-LLM SVA hook (cambrian_llama.py:181-207)
# ================================================================================================
def k_copy_rows(src: Optional[torch.Tensor], src_map: Optional[RowMap], dst: torch.Tensor, dst_map: RowMap, rows: int,
                D: int) -> None:
    L.require_gpu(src, dst)
    L.call("cmb_copy_rows", L.dtype_code(dst.dtype), L.ptr(src), None if src_map is None else C.byref(src_map), dst.data_ptr(),
           C.byref(dst_map), rows, D, device=dst.device)


def hook_row_map(S: int, H: int, side: int) -> RowMap:
    """query row (b, i, j) -> element offset of hidden[b, i*(side+1)+j, :] relative to hidden[0, image_position]."""
    return L.make_map(side * side, side, S * H, (side + 1) * H, H)


class GatherQueryRowsFn(torch.autograd.Function):
    """hidden [B,S,H] -> the side*side latent-query rows [B*side*side, H] starting at ``pos`` (newline column
    skipped): ``hidden[:, pos:pos+side*(side+1)].view(B,side,side+1,H)[:, :, :side]`` as one strided copy.

    ``link`` (a dict shared with the ScatterQueryRowsFn of the same hook, or None): the hook reads these rows of
    ``hidden`` and then overwrites exactly them, so d(hidden) = [text / newline rows: the scatter's incoming gradient;
    query rows: this gather's].  Returned as two dense tensors autograd would zero-fill one, clone the other and add
    them (4 extra passes over [B,S,H] per hook).  With a link the scatter's backward — which always runs first: this
    node's incoming gradient is computed from the scatter's d(rows) — HANDS its dense result over in ``link["dh"]`` and
    returns no gradient for ``hidden`` itself; this backward writes its rows into that buffer and returns it as THE
    gradient of ``hidden``.  Autograd therefore sees one ordinary contribution (no assumption about which buffer it
    keeps, views / CopySlices and further consumers of ``hidden`` included: ADVICE r3)."""

    @staticmethod
    def forward(ctx, hidden, pos: int, side: int, link=None):
        B, S, H = hidden.shape
        assert hidden.is_contiguous()
        out = torch.empty((B * side * side, H), dtype=hidden.dtype, device=hidden.device)
        k_copy_rows(hidden.view(-1)[pos * H:], hook_row_map(S, H, side), out, L.identity_map(H), B * side * side, H)
        ctx.cfg = (B, S, H, pos, side)
        ctx.link = link
        if link is not None:
            link["armed"] = bool(ctx.needs_input_grad[0])  # this node's backward will run iff the scatter's does
        return out

    @staticmethod
    def backward(ctx, g):
        B, S, H, pos, side = ctx.cfg
        g = g.contiguous()
        dh = ctx.link.pop("dh", None) if ctx.link is not None else None
        if dh is None:
            dh = torch.zeros((B, S, H), dtype=g.dtype, device=g.device)
        elif dh.dtype != g.dtype:
            g = g.to(dh.dtype)
        k_copy_rows(g, L.identity_map(H), dh.view(-1)[pos * H:], hook_row_map(S, H, side), B * side * side, H)
        return dh, None, None, None


class ScatterQueryRowsFn(torch.autograd.Function):
    """In-place write-back of the updated latent queries into ``hidden`` (the reference's
    ``hidden_states[:, a:b] = latent_query_with_newline``, cambrian_llama.py:207); the newline column and all
    text rows are untouched.  ``link``: see GatherQueryRowsFn."""

    @staticmethod
    def forward(ctx, hidden, rows, pos: int, side: int, link=None):
        B, S, H = hidden.shape
        assert hidden.is_contiguous() and rows.is_contiguous()
        k_copy_rows(rows, L.identity_map(H), hidden.view(-1)[pos * H:], hook_row_map(S, H, side), B * side * side, H)
        ctx.mark_dirty(hidden)
        ctx.cfg = (B, S, H, pos, side)
        ctx.link = link
        return hidden

    @staticmethod
    def backward(ctx, g):
        B, S, H, pos, side = ctx.cfg
        g = g.contiguous()
        drows = torch.empty((B * side * side, H), dtype=g.dtype, device=g.device)
        k_copy_rows(g.view(-1)[pos * H:], hook_row_map(S, H, side), drows, L.identity_map(H), B * side * side, H)
        # d(hidden) = g with the overwritten rows zeroed: in place when g is a buffer its producer marked as handed to this node
        # alone (RmsNormForkFn.backward: the decoder layer that follows), else on a copy (round 6: the copy was 400 MB x 10 layers)
        dh = g if getattr(g, "_cmb_exclusive", False) else g.clone()
        k_copy_rows(None, None, dh.view(-1)[pos * H:], hook_row_map(S, H, side), B * side * side, H)  # zero the rows
        if ctx.link is not None and ctx.link.get("armed") and ctx.needs_input_grad[0]:
            ctx.link["dh"] = dh  # the paired gather's backward completes it and returns it for `hidden`
            return None, drows, None, None, None
        return dh, drows, None, None, None


def gather_query_rows(hidden, pos: int, side: int, link=None):
    return GatherQueryRowsFn.apply(hidden, pos, side, link)


def scatter_query_rows(hidden, rows, pos: int, side: int, link=None):
    return ScatterQueryRowsFn.apply(hidden, rows, pos, side, link)


# ================================================================================================
# autograd: fused shifted cross-entropy and SwiGLU (LLM side; cambrian_llama.py:402-422, Llama MLP)
# ================================================================================================
class CrossEntropyFn(torch.autograd.Function):
    """mean_{labels != ignore} ( logsumexp(logits[t]) - logits[t, labels[t]] ) over [T, V] logits kept in their
    compute dtype (the reference's ``logits.float()`` + ``CrossEntropyLoss``, cambrian_llama.py:409-422: fp32 math on
    the same bf16-rounded values).  The backward overwrites ``logits`` with dlogits when ``inplace`` (the tensor that
    lm_head produced is not needed by anybody else's backward)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index: int, inplace: bool):
        L.require_gpu(logits, labels)
        if logits.stride(1) != 1:
            raise L.CambrianAmdError("logits must be row-major")
        labels = labels.to(torch.int64).contiguous()
        lse, loss_rows = k_cross_entropy_fwd(logits, labels, ignore_index)
        n_valid = (labels != ignore_index).sum().to(torch.float32)
        ctx.save_for_backward(logits, labels, lse, n_valid)
        ctx.ignore_index, ctx.inplace = ignore_index, inplace
        return loss_rows.sum() / n_valid

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse, n_valid = ctx.saved_tensors
        scale = (g.to(torch.float32) / n_valid).reshape(1).contiguous()
        out = logits if ctx.inplace else torch.empty_like(logits)
        k_cross_entropy_bwd(logits, labels, ctx.ignore_index, lse, scale, out)
        return out, None, None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100, inplace: bool = False):
    return CrossEntropyFn.apply(logits, labels, ignore_index, inplace)


class SwiGLUFn(torch.autograd.Function):
    """h = silu(g) * u in one pass; backward (dg, du) in one pass (Llama MLP: down_proj(silu(gate) * up))."""

    @staticmethod
    def forward(ctx, g, u):
        L.require_gpu(g, u)
        shape = g.shape
        D = shape[-1]
        g2, u2 = g.reshape(-1, D), u.reshape(-1, D)
        if g2.stride(1) != 1 or u2.stride(1) != 1:
            g2, u2 = g2.contiguous(), u2.contiguous()
        h = k_swiglu_fwd(g2, u2)
        ctx.save_for_backward(g2, u2)
        ctx.shape = shape
        return h.view(shape)

    @staticmethod
    def backward(ctx, dh):
        g2, u2 = ctx.saved_tensors
        rows, D = g2.shape
        dh2 = dh.reshape(rows, D)
        if dh2.stride(1) != 1:
            dh2 = dh2.contiguous()
        dg = torch.empty((rows, D), dtype=g2.dtype, device=g2.device)
        du = torch.empty((rows, D), dtype=g2.dtype, device=g2.device)
        k_swiglu_bwd(dh2, g2, u2, dg, du)
        return dg.view(ctx.shape), du.view(ctx.shape)


def swiglu(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    return SwiGLUFn.apply(g, u)


class QkvRopeFn(torch.autograd.Function):
    """packed QKV projection [B,S,(nh+2nkv)*Dh] -> q [B,nh,S,Dh], k, v [B,nkv,S,Dh] (transposed VIEWS of token-major
    buffers) with RoPE on q and k, one kernel;
    the backward merges (dq, dk, dv) into one d(packed) with the inverse rotation (no slice-backward zero fills)."""

    @staticmethod
    def forward(ctx, packed, cos, sin, nh: int, nkv: int, hd: int):
        L.require_gpu(packed, cos, sin)
        B, S, W = packed.shape
        if W != (nh + 2 * nkv) * hd or not packed.is_contiguous():
            raise L.CambrianAmdError("packed QKV must be contiguous [B,S,(nh+2*nkv)*hd]")
        dt, dev = packed.dtype, packed.device
        q = torch.empty((B, S, nh, hd), dtype=dt, device=dev)
        k = torch.empty((B, S, nkv, hd), dtype=dt, device=dev)
        v = torch.empty((B, S, nkv, hd), dtype=dt, device=dev)
        k_qkv_rope(packed, cos, sin, q, k, v)
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (B, S, nh, nkv, hd)
        return q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)  # [B,H,S,hd] views of token-major storage

    @staticmethod
    def backward(ctx, dq, dk, dv):
        cos, sin = ctx.saved_tensors
        B, S, nh, nkv, hd = ctx.cfg
        # token-major storage; free when the attention backward returns grads laid out like its inputs
        dq, dk, dv = (t.transpose(1, 2).contiguous() for t in (dq, dk, dv))
        dp = torch.empty((B, S, (nh + 2 * nkv) * hd), dtype=dq.dtype, device=dq.device)
        k_qkv_rope(dp, cos, sin, dq, dk, dv, merge=True)
        return dp, None, None, None, None, None


def qkv_rope(packed, cos, sin, nh: int, nkv: int, hd: int):
    return QkvRopeFn.apply(packed, cos, sin, nh, nkv, hd)


class SwiGLUPackedFn(torch.autograd.Function):
    """h = silu(gu[:, :I]) * gu[:, I:] for the packed output of a fused gate|up projection [T, 2I]; the backward
    writes both halves of d(gu) straight into one [T, 2I] buffer."""

    @staticmethod
    def forward(ctx, gu):
        L.require_gpu(gu)
        shape = gu.shape
        I2 = shape[-1]
        I = I2 // 2
        g2 = gu.reshape(-1, I2)
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        h = k_swiglu_fwd(g2, g2, cols=I, u_col=I, what="cmb_act_mul(silu, packed)")
        ctx.save_for_backward(g2)
        ctx.shape = shape
        return h.view(*shape[:-1], I)

    @staticmethod
    def backward(ctx, dh):
        (g2,) = ctx.saved_tensors
        rows, I2 = g2.shape
        I = I2 // 2
        dh2 = dh.reshape(rows, I)
        if dh2.stride(1) != 1:
            dh2 = dh2.contiguous()
        dgu = torch.empty((rows, I2), dtype=g2.dtype, device=g2.device)
        k_swiglu_bwd(dh2, g2, g2, dgu, dgu, cols=I, u_col=I, what="cmb_swiglu_bwd(packed)")
        return dgu.view(ctx.shape)


def swiglu_packed(gu: torch.Tensor) -> torch.Tensor:
    return SwiGLUPackedFn.apply(gu)


# ================================================================================================
# autograd: causal self-attention of the decoder — stock forward, HIP backward
# ================================================================================================
def _token_major(t: torch.Tensor) -> torch.Tensor:
    """[B,H,S,D] tensor whose storage is [B,S,H,D]-contiguous (a transposed view); copies only if it is not."""
    tm = t.transpose(1, 2)
    return t if tm.is_contiguous() else tm.contiguous().transpose(1, 2)


class CausalAttnFn(torch.autograd.Function):
    """GQA attention, head_dim 128, on flash_bwd.hip: forward kernel (online softmax, writes the log-sum-exp),
    backward = dQ kernel + dK/dV kernel (no atomics).  K/V are read un-expanded (grouped heads): no
    repeat_interleave copies of K and V per layer as F.scaled_dot_product_attention(enable_gqa=True) makes.
    ``kv_len`` None: causal (the decoder).  ``kv_len`` = n: bidirectional over keys [0, n), rows [n, S) are padding
    (trainable vision towers, see ``vit_attention``).  ``key_valid`` (causal only): uint8 / bool [B, S] key-padding mask of
    the collator; query q sees key k iff k <= q and (key_valid[b, k] or k == q)."""

    @staticmethod
    def forward(ctx, q, k, v, scale=None, kv_len=None, key_valid=None):
        L.require_gpu(q, k, v, key_valid)
        B, _, S, D = q.shape
        scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
        causal, n = (1, S) if kv_len is None else (0, int(kv_len))
        q, k, v = _token_major(q), _token_major(k), _token_major(v)
        if key_valid is not None:
            if not causal or key_valid.shape != (B, S):
                raise L.CambrianAmdError("key_valid is a [B, S] mask of the causal form")
            key_valid = key_valid.view(torch.uint8) if key_valid.dtype == torch.bool else key_valid.to(torch.uint8)
            key_valid = key_valid.contiguous()
        out, lse = k_flash_attn_fwd(q, k, v, scale, causal, n, key_valid)
        out = out.transpose(1, 2)  # [B,H,S,D] view of token-major storage: the o_proj input needs no copy
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.key_valid = key_valid
        ctx.cfg = (scale, causal, n)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        scale, causal, n = ctx.cfg
        q, out, dout = _token_major(q), _token_major(out), _token_major(dout)
        k, v = _token_major(k), _token_major(v)
        dq, dk, dv = k_flash_attn_bwd(q, k, v, out, dout, lse.contiguous(), scale, causal, n, ctx.key_valid)
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None


def vit_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """Bidirectional self-attention WITH a backward, for towers that train: q, k, v [B,H,N,hd] bf16
    with any N and hd <= 128.  Runs on the decoder's flash kernels: tokens zero-padded to a multiple of 128 and masked
    through ``kv_len``, head_dim zero-padded to 128 (zero columns change neither q.k nor the first hd output columns);
    the padding and the final slice are ordinary autograd ops, so padded rows receive zero gradients."""
    B, H, N, hd = q.shape
    if hd > 128 or q.dtype != torch.bfloat16:
        raise L.CambrianAmdError("vit_attention: bf16 and head_dim <= 128 only")
    S = (N + 127) // 128 * 128
    pad = (0, 128 - hd, 0, S - N)
    qp, kp, vp = (F.pad(t, pad) for t in (q, k, v))
    return CausalAttnFn.apply(qp, kp, vp, scale, N)[:, :, :N, :hd]


def causal_attention_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    return (q.is_cuda and q.dtype == torch.bfloat16 and q.shape[-1] == 128 and q.shape[2] % 128 == 0
            and q.shape[2] == k.shape[2] and q.shape[1] % k.shape[1] == 0)


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B,H,S,128], k / v [B,HKV,S,128] (any strides with a contiguous last dim) -> [B,H,S,128].  ``key_valid``: optional
    bool / uint8 [B,S] key-padding mask (the collator's ``attention_mask``); the diagonal stays open."""
    return CausalAttnFn.apply(q, k, v, None, None, key_valid)


# ================================================================================================
# decode step of generate(): attention of one new token per sequence against the K/V cache (decode_attn.hip)
# ================================================================================================
_DECODE_WS: dict = {}   # device -> fp32 workspace of the split partials, grown on demand and reused by every layer and step


def decode_attention_supported(dtype: torch.dtype, nh: int, nkv: int, hd: int) -> bool:
    """The geometries ``cmb_decode_attn`` takes: bf16 / fp32, head_dim 64 / 96 / 128, at most 8 query heads per KV head."""
    return (dtype in (torch.bfloat16, torch.float32) and hd in (64, 96, 128) and nkv > 0 and nh > 0 and nh % nkv == 0
            and nh // nkv <= 8)


def decode_attention_plan(B: int, nkv: int, t: int, splits: int = 0) -> Tuple[int, int]:
    """(splits, chunk) of a decode step over cache keys 0..t: the key range is cut into ``splits`` chunks of ``chunk`` keys
    (the last one shorter), ``splits * chunk >= t + 1 > (splits - 1) * chunk``.  ``splits`` = 0 asks for the library's
    choice, a pure function of (B, nkv, t, CU count); a forced count is reduced when t + 1 is short."""
    s, ch = C.c_int32(0), C.c_int64(0)
    L.check(L.load().cmb_decode_attn_plan(B, nkv, t, splits, C.byref(s), C.byref(ch), None), "cmb_decode_attn_plan")
    return s.value, ch.value


def decode_attention_max_splits() -> int:
    mx = C.c_int32(0)
    L.load().cmb_decode_attn_plan(1, 1, 0, 0, None, None, C.byref(mx))
    return mx.value


def _decode_attention_launch(name: str, symbol: str, ws_symbol: str, supported, q, k, v, cos, sin, kc, vc, factors: tuple,
                             multi: bool, t0: int, key_valid, scale, splits: int) -> torch.Tensor:
    """The one body of ``decode_attention``, ``decode_attention_multi`` and ``decode_attention_kv8``: every check in its
    order, the device's workspace and the launch of ``symbol``.  ``name`` heads the messages, ``supported`` is the caller's
    geometry test and ``ws_symbol`` its workspace query.  ``kc`` / ``vc``: the cache tensors [B, nkv, Lmax, hd]; of e4m3
    caches the bytes, their fp32 factors being ``factors`` = (k, v), else ().  ``multi``: q holds Q rows per sequence, the
    tokens of slots t0 .. t0 + Q - 1; else one row, slot t0."""
    L.require_gpu(q, k, v, cos, sin, kc, vc, *factors, key_valid)
    if torch.is_grad_enabled() and any(x.requires_grad for x in (q, k, v, kc, vc)):     # e4m3 caches: bytes, which never do
        raise L.CambrianAmdError(f"{name} has no backward: call it under torch.no_grad()")
    B, nkv, Lmax, hd = kc.shape
    nh = q.shape[1] // hd
    Q = 1 if not multi else q.shape[0] // B if B > 0 else 0
    rows, dt = B * Q, q.dtype
    if not (supported(dt, nh, nkv, hd, Q) if multi else supported(dt, nh, nkv, hd)) or q.shape != (rows, nh * hd) \
            or k.shape != (rows, nkv * hd) or v.shape != k.shape or vc.shape != kc.shape \
            or not (k.dtype == v.dtype == dt and kc.dtype == vc.dtype == (torch.uint8 if factors else dt)):
        raise L.CambrianAmdError(
            f"{name}: unsupported geometry q {tuple(q.shape)} {dt} k {tuple(k.shape)} cache {tuple(kc.shape)}" if factors else
            f"{name}: unsupported geometry q {tuple(q.shape)} k {tuple(k.shape)} cache {tuple(kc.shape)} {dt}")
    if not 0 <= t0 or t0 + Q > Lmax or key_valid.dim() != 2 or key_valid.shape[0] != B or key_valid.shape[1] < t0 + Q:
        raise L.CambrianAmdError(f"{name}: {'slots t0 .. t0 + Q - 1' if multi else 'slot t'} outside the cache or the key mask")
    if q.stride(1) != 1 or k.stride(1) != 1 or v.stride(1) != 1 or kc.stride(3) != 1 or vc.stride() != kc.stride() \
            or (factors and factors[1].stride() != factors[0].stride()) or key_valid.stride(1) != 1:
        raise L.CambrianAmdError(
            f"{name}: rows of q / k / v and the key mask must be contiguous, and the two caches of one layout" if factors else
            f"{name}: rows of q / k / v, the caches and the key mask must be contiguous")
    if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape != (rows, hd // 2) or sin.shape != cos.shape \
            or not cos.is_contiguous() or not sin.is_contiguous():
        raise L.CambrianAmdError(f"{name}: cos / sin are the contiguous fp32 [{'B*Q' if multi else 'B'}, hd/2] tables of rope_table")
    if key_valid.dtype == torch.bool:
        key_valid = key_valid.view(torch.uint8)
    elif key_valid.dtype != torch.uint8:
        raise L.CambrianAmdError(f"{name}: key_valid is a bool / uint8 mask")
    scale = 1.0 / math.sqrt(hd) if scale is None else float(scale)
    slots = (Q, t0) if multi else (t0,)
    need = getattr(L.load(), ws_symbol)(B, nh, nkv, hd, *slots, splits)
    if need < 0:
        L.check(int(need), ws_symbol)
    ws = _DECODE_WS.get(q.device)
    if need > 0 and (ws is None or ws.numel() < need):
        ws = _DECODE_WS[q.device] = torch.empty(int(need), dtype=torch.float32, device=q.device)
    out = torch.empty((rows, nh * hd), dtype=dt, device=q.device)
    lead = () if multi or factors else (L.dtype_code(dt),)           # the two bf16-only entry points take no dtype code
    fac = (factors[0].data_ptr(), factors[1].data_ptr(), factors[0].stride(0), factors[0].stride(1)) if factors else ()
    L.call(symbol, *lead, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), cos.data_ptr(),
           sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), kc.stride(0), kc.stride(1), kc.stride(2), *fac, B, nh, nkv, hd, *slots,
           key_valid.data_ptr(), key_valid.stride(0), scale, splits, L.ptr(ws) if need > 0 else None, int(need),
           out.data_ptr(), device=q.device)
    return out


def decode_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                     kcache: torch.Tensor, vcache: torch.Tensor, t: int, key_valid: torch.Tensor,
                     scale: Optional[float] = None, splits: int = 0) -> torch.Tensor:
    """One new token per sequence: q [B, nh*hd], k / v [B, nkv*hd] (rows of the projections, un-roped; views into one
    packed row are fine), cos / sin fp32 [B, hd/2], k / v caches [B, nkv, Lmax, hd] -> out [B, nh*hd].  Ropes q and k, stores
    roped k and v into cache slot ``t`` and attends to slots 0..t under ``key_valid`` (bool / uint8 [B, >= t+1], slot t
    always open).  Inference only: there is no backward."""
    return _decode_attention_launch("decode_attention", "cmb_decode_attn", "cmb_decode_attn_ws", decode_attention_supported,
                                    q, k, v, cos, sin, kcache, vcache, (), False, t, key_valid, scale, splits)


def decode_attention_enabled() -> bool:
    """``CAMBRIAN_AMD_DECODE_ATTN=0`` in the environment: decode steps take the stock SDPA branch (A/B runs)."""
    return L.env_flag("CAMBRIAN_AMD_DECODE_ATTN", True)


# ------------------------------------------------------------------------------------------------
# the same step for Q consecutive new tokens per sequence (decode_attn_multi.hip): the verify step of prompt-lookup decoding
# ------------------------------------------------------------------------------------------------
DECODE_LOOKUP_MAX_ROWS = 16     # rows of a multi-token step: the last token plus at most 15 drafts


def decode_attention_multi_supported(dtype: torch.dtype, nh: int, nkv: int, hd: int, Q: int) -> bool:
    """The geometries ``cmb_decode_attn_multi`` takes: bf16, head_dim 64 / 96 / 128, G = nh / nkv <= 8, 1 <= Q <= 16 and
    Q * G <= 64."""
    return (dtype == torch.bfloat16 and decode_attention_supported(dtype, nh, nkv, hd)
            and 1 <= Q <= DECODE_LOOKUP_MAX_ROWS and Q * (nh // nkv) <= 64)


def decode_attention_multi_plan(B: int, nkv: int, t0: int, Q: int, splits: int = 0) -> Tuple[int, int]:
    """(splits, chunk) of a Q-token step over cache slots 0 .. t0 + Q - 1, ``splits * chunk >= t0 + Q > (splits - 1) * chunk``;
    the last chunk holds the step's own slots.  ``splits`` = 0: the library's choice, a pure function of (B, nkv, t0 + Q, CU
    count)."""
    s, ch = C.c_int32(0), C.c_int64(0)
    L.check(L.load().cmb_decode_attn_multi_plan(B, nkv, t0, Q, splits, C.byref(s), C.byref(ch), None),
            "cmb_decode_attn_multi_plan")
    return s.value, ch.value


def decode_attention_multi(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                           kcache: torch.Tensor, vcache: torch.Tensor, t0: int, key_valid: torch.Tensor,
                           scale: Optional[float] = None, splits: int = 0) -> torch.Tensor:
    """Q consecutive new tokens per sequence: bf16 q [B*Q, nh*hd], k / v [B*Q, nkv*hd] (un-roped rows of the projections, row
    b*Q + j = token j of sequence b; views into one packed row are fine), cos / sin fp32 [B*Q, hd/2], k / v caches
    [B, nkv, Lmax, hd] -> out [B*Q, nh*hd].  Ropes q and k, stores roped k and v of token j into cache slot ``t0 + j`` and lets
    token j attend to slots 0 .. t0 + j: cached slots under ``key_valid`` (bool / uint8 [B, >= t0+Q], columns >= t0 are not
    read), the step's own slots always.  Inference only: there is no backward."""
    return _decode_attention_launch("decode_attention_multi", "cmb_decode_attn_multi", "cmb_decode_attn_multi_ws",
                                    decode_attention_multi_supported, q, k, v, cos, sin, kcache, vcache, (), True, t0,
                                    key_valid, scale, splits)


# ------------------------------------------------------------------------------------------------
# a chunk of Q new tokens per sequence against the cache (extend_attn.hip): the suffix of a prompt over a cached prefix
# ------------------------------------------------------------------------------------------------
EXTEND_MAX_ROWS = 4096          # tokens of a chunk


def extend_attention_supported(dtype: torch.dtype, nh: int, nkv: int, hd: int, Q: int) -> bool:
    """The geometries ``cmb_extend_attn`` takes: bf16, head_dim 64 / 96 / 128, G = nh / nkv <= 8, 1 <= Q <= 4096."""
    return dtype == torch.bfloat16 and decode_attention_supported(dtype, nh, nkv, hd) and 1 <= Q <= EXTEND_MAX_ROWS


def extend_attention_plan(B: int, nkv: int, t0: int, Q: int, splits: int = 0) -> Tuple[int, int]:
    """(splits, chunk) of a Q-token chunk over cache slots 0 .. t0 + Q - 1, ``splits * chunk >= t0 + Q > (splits - 1) * chunk``.
    ``splits`` = 0: the library's choice, a pure function of (B, nkv, t0, Q, CU count) that counts the chunk's row blocks as
    batch rows, so long chunks split little or not at all."""
    s, ch = C.c_int32(0), C.c_int64(0)
    L.check(L.load().cmb_extend_attn_plan(B, nkv, t0, Q, splits, C.byref(s), C.byref(ch), None), "cmb_extend_attn_plan")
    return s.value, ch.value


def extend_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                     kcache: torch.Tensor, vcache: torch.Tensor, t0: int, key_valid: torch.Tensor,
                     scale: Optional[float] = None, splits: int = 0) -> torch.Tensor:
    """A chunk of Q consecutive new tokens per sequence: ``decode_attention_multi``'s arguments and stores (bf16 q [B*Q, nh*hd],
    k / v [B*Q, nkv*hd] un-roped, cos / sin fp32 [B*Q, hd/2], caches [B, nkv, Lmax, hd] -> out [B*Q, nh*hd]; roped k and v of
    token j into cache slot ``t0 + j``) for any 1 <= Q <= 4096, under ONE mask rule for cached and new slots: token j attends
    slot s iff s <= t0 + j and (``key_valid[b, s]`` or s == t0 + j) — ``extend_mask``.  ``key_valid`` (bool / uint8
    [B, >= t0+Q]) is read for slots 0 .. t0 + Q - 1, so suffixes left-padded inside the chunk are legal.  Inference only."""
    return _decode_attention_launch("extend_attention", "cmb_extend_attn", "cmb_extend_attn_ws", extend_attention_supported,
                                    q, k, v, cos, sin, kcache, vcache, (), True, t0, key_valid, scale, splits)


def extend_mask(key_mask: torch.Tensor, t0: int, Q: int) -> torch.Tensor:
    """bool [B, Q, t0 + Q]: what token j of a chunk may attend (``cmb_extend_attn``'s rule) — slot s iff s <= t0 + j and
    (``key_mask[b, s]`` or s == t0 + j).  For the torch bodies of ``extend`` and the tests."""
    S = t0 + Q
    s = torch.arange(S, device=key_mask.device)
    limit = t0 + torch.arange(Q, device=key_mask.device)[:, None]
    return (s[None, :] <= limit)[None] & (key_mask[:, None, :S].bool() | (s[None, :] == limit)[None])


# ------------------------------------------------------------------------------------------------
# the same step on an e4m3 K / V cache (decode_attn_kv8.hip): one byte per element plus one fp32 factor per cache row, about
# half the cache's memory and stream.  Opt-in (``config.decode_kv_fp8`` / CAMBRIAN_AMD_DECODE_KV_FP8): it changes numerics
# (profiles/decode_kv8.md has what was measured).
# ------------------------------------------------------------------------------------------------
def _config_switch(env_name: str, config_flag: bool, strict: bool = False) -> bool:
    """The opt-in ``decode_*_enabled(config_flag)`` switches: ``env_name`` in the environment overrides, unset (or empty) it
    is ``config_flag``.  ``strict``: only ``1`` / ``0`` are taken and anything else raises; else everything but ``0`` is on."""
    v = os.environ.get(env_name)
    if v is None or v == "":
        return bool(config_flag)
    if strict and v not in ("0", "1"):
        raise ValueError(f"{env_name}={v!r}: the switch takes 1 or 0")
    return v != "0"


def decode_kv_fp8_enabled(config_flag: bool = False) -> bool:
    """Whether ``generate()`` keeps its K / V cache in e4m3: ``CAMBRIAN_AMD_DECODE_KV_FP8`` = ``1`` / ``0`` in the environment
    overrides, unset (or empty) it is ``config_flag`` (the model's ``config.decode_kv_fp8``, absent = off)."""
    return _config_switch("CAMBRIAN_AMD_DECODE_KV_FP8", config_flag)


class KvCacheE4M3:
    """One tensor (K or V) of a layer's cache in the format of ``cmb_decode_attn_kv8``: ``q`` uint8 [B, nkv, Lmax, hd] (OCP
    e4m3fn bytes, rows of hd contiguous bytes) and ``inv`` fp32 [B, nkv, Lmax] (slot stride 1); an entry's value is
    ``e4m3(q) * inv``."""
    __slots__ = ("q", "inv")

    def __init__(self, q: torch.Tensor, inv: torch.Tensor):
        if q.dtype != torch.uint8 or inv.dtype != torch.float32 or q.dim() != 4 or inv.shape != q.shape[:3] \
                or q.stride(3) != 1 or inv.stride(2) != 1 or q.device != inv.device:
            raise L.CambrianAmdError("KvCacheE4M3: q is uint8 [B, nkv, Lmax, hd] with contiguous rows, inv fp32 [B, nkv, Lmax] "
                                     "with contiguous slots, on one device")
        self.q, self.inv = q, inv

    @classmethod
    def empty(cls, B: int, nkv: int, Lmax: int, hd: int, device) -> "KvCacheE4M3":
        """Zero bytes (the value 0) and zero factors."""
        return cls(torch.zeros(B, nkv, Lmax, hd, dtype=torch.uint8, device=device),
                   torch.zeros(B, nkv, Lmax, dtype=torch.float32, device=device))

    @property
    def shape(self):
        return self.q.shape

    def dequantize(self) -> torch.Tensor:
        """fp32 [B, nkv, Lmax, hd]: what the kernel reads (tests and tools; not on a hot path)."""
        return self.q.view(torch.float8_e4m3fn).float() * self.inv[..., None]


def decode_attention_kv8_supported(dtype: torch.dtype, nh: int, nkv: int, hd: int) -> bool:
    """The geometries ``cmb_decode_attn_kv8`` takes: ``decode_attention_supported``'s with bf16 activations only."""
    return dtype == torch.bfloat16 and decode_attention_supported(dtype, nh, nkv, hd)


def kv_quantize_e4m3(src: torch.Tensor, cache: KvCacheE4M3, L_: Optional[int] = None) -> KvCacheE4M3:
    """The prefill's K or V, bf16 [B, nkv, L, hd] (the ``kv_out`` tensors as they lie: any strides the kernel's 16-byte loads can take, else a contiguous copy
    is made first), into slots 0 .. L-1 of ``cache``: bytes and factors of ``k_quantize_fp8_rows`` on the same rows.  Nothing else of
    the cache is touched.  One launch."""
    L.require_gpu(src, cache.q, cache.inv)
    B, nkv, Ls, hd = src.shape
    n = Ls if L_ is None else int(L_)
    if src.dtype != torch.bfloat16 or cache.q.shape[:2] != (B, nkv) or cache.q.shape[3] != hd \
            or not 0 <= n <= min(Ls, cache.q.shape[2]):
        raise L.CambrianAmdError(f"kv_quantize_e4m3: src {tuple(src.shape)} {src.dtype} does not fit the cache "
                                 f"{tuple(cache.q.shape)} at L = {n}")
    if src.stride(3) != 1 or src.data_ptr() % 16 or any(src.stride(i) % 8 for i in range(3)):      # the kernel loads 16 bytes at a time
        src = src.contiguous()
    L.call("cmb_kv_quantize_e4m3", src.data_ptr(), src.stride(0), src.stride(1), src.stride(2), B, nkv, n, hd, cache.q.data_ptr(),
           cache.q.stride(0), cache.q.stride(1), cache.q.stride(2), cache.inv.data_ptr(), cache.inv.stride(0), cache.inv.stride(1),
           device=src.device)
    return cache


def decode_attention_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                         kcache: KvCacheE4M3, vcache: KvCacheE4M3, t: int, key_valid: torch.Tensor,
                         scale: Optional[float] = None, splits: int = 0) -> torch.Tensor:
    """``decode_attention`` on e4m3 caches: bf16 q [B, nh*hd], k / v [B, nkv*hd], the caches ``KvCacheE4M3`` of one shape and
    stride -> out bf16 [B, nh*hd].  Ropes q and k, quantises roped k (rounded to bf16 first) and raw v into slot ``t`` (bytes
    and factors) and attends to slots 0..t as stored.  Inference only."""
    return _decode_attention_launch("decode_attention_kv8", "cmb_decode_attn_kv8", "cmb_decode_attn_ws",
                                    decode_attention_kv8_supported, q, k, v, cos, sin, kcache.q, vcache.q,
                                    (kcache.inv, vcache.inv), False, t, key_valid, scale, splits)


def decode_attention_any(q, k, v, cos, sin, kcache, vcache, t: int, key_valid) -> torch.Tensor:
    """``decode_attention`` or, for ``KvCacheE4M3`` caches, ``decode_attention_kv8``: the one line the decode call sites share."""
    if isinstance(kcache, KvCacheE4M3):
        return decode_attention_kv8(q, k, v, cos, sin, kcache, vcache, t, key_valid)
    return decode_attention(q, k, v, cos, sin, kcache, vcache, t, key_valid)


# ================================================================================================
# decode step of generate(): the layer's linears and the lm_head at M <= 16 rows as weight streams (decode_linear.hip)
# ================================================================================================
DECODE_LINEAR_MAX_ROWS = 16
# Largest batch at which decode steps take the kernel by default; 0 = nowhere (the kernel stays behind the switch).  Set from
# the measured table of profiles/decode_linear.md (tools/bench_decode_linear.py): at batch 1 / 4 / 16 on the Llama-3-8B, Yi-34B
# and Phi-3-mini geometries the five-launch layer's median is below the stock sequence's fastest window, so it is on throughout.
DECODE_LINEAR_DEFAULT_MAX_ROWS = 16


def decode_linear_enabled(rows: int = 1) -> bool:
    """Whether a decode step of ``rows`` sequences runs its linears on ``decode_linear``: ``CAMBRIAN_AMD_DECODE_LINEAR=0``
    is the stock BLAS sequence and ``=1`` the kernel wherever it applies (A/B runs); unset, the default the measured table
    led to."""
    v = os.environ.get("CAMBRIAN_AMD_DECODE_LINEAR")
    if v is None:
        return rows <= DECODE_LINEAR_DEFAULT_MAX_ROWS
    return v != "0"


def decode_linear_plan(M: int, N: int, K: int, act: Optional[str] = None, cus: int = 0) -> Tuple[int, int]:
    """(weight rows per workgroup, workgroups) of a ``decode_linear`` call: a pure function of (M, N, K, act, CU count);
    ``cus`` = 0 takes the current device's count."""
    return _decode_plan("cmb_decode_linear_plan", M, N, K, act, cus)


def _decode_plan(symbol: str, M: int, N: int, K: int, act, cus: int) -> Tuple[int, int]:
    rows, wgs = C.c_int32(0), C.c_int64(0)
    L.check(getattr(L.load(), symbol)(M, N, K, _decode_linear_act(act), cus, C.byref(rows), C.byref(wgs)), symbol)
    return rows.value, wgs.value


def _decode_linear_act(act) -> int:
    if act in (None, "none", 0):
        return 0
    if act in ("swiglu", 1):
        return 1
    raise L.CambrianAmdError(f"decode_linear: act is None or 'swiglu', got {act!r}")


def _decode_linear_rows_ok(t: torch.Tensor, K: int) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.shape[1] == K and t.stride(1) == 1
            and t.stride(0) % 8 == 0 and t.stride(0) >= K and t.data_ptr() % 16 == 0)


def decode_linear_weight_supported(M: int, w: torch.Tensor, act: Optional[str] = None) -> bool:
    """The weight's side of ``decode_linear_supported``, for ``M`` rows of x that are yet to be computed."""
    return (w.dim() == 2 and _decode_linear_rows_ok(w, w.shape[1])
            and bool(L.load().cmb_decode_linear_supported(M, w.shape[0], w.shape[1], _decode_linear_act(act))))


def decode_linear_supported(x: torch.Tensor, w: torch.Tensor, act: Optional[str] = None) -> bool:
    """Whether ``decode_linear(x, w, act=act)`` takes these operands: bf16 GPU tensors, x [M <= 16, K] and w [N, K] with
    contiguous rows, 16-byte aligned with row strides that are multiples of 8, K % 8 == 0, N even for SwiGLU."""
    return (w.dim() == 2 and x.dim() == 2 and x.shape[0] >= 1 and _decode_linear_rows_ok(x, w.shape[1])
            and decode_linear_weight_supported(x.shape[0], w, act))


def _decode_linear_launch(name: str, supported, x: torch.Tensor, weights: tuple, grad_weights: tuple, describe, norm_weight,
                          eps, act, residual, out_dtype, out) -> torch.Tensor:
    """The one body of the four decode linears.  ``supported``: the caller's own ``*_supported`` test, put to (x, *weights,
    act); ``describe()``: the weights' part of its message; ``grad_weights``: the weights a backward would flow to.  The
    arguments of ``cmb_<name>`` differ in the weights alone: per tensor its pointer and, for a matrix, its row stride."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, *grad_weights, norm_weight, residual)):
        raise L.CambrianAmdError(f"{name} has no backward: call it under torch.no_grad()")
    L.require_gpu(x, *weights, norm_weight, residual, out)
    code = _decode_linear_act(act)
    if not supported(x, *weights, act):
        raise L.CambrianAmdError(f"{name}: unsupported operands x {tuple(x.shape)} {x.dtype} strides {x.stride()}, "
                                 f"{describe()}, act {act!r}")
    (M, K), N = x.shape, weights[0].shape[0]
    cols = N // 2 if code else N
    if norm_weight is not None and (norm_weight.dtype != torch.bfloat16 or norm_weight.shape != (K,)
                                    or not norm_weight.is_contiguous()):
        raise L.CambrianAmdError(f"{name}: norm_weight is a contiguous bf16 [K] vector")
    if residual is not None and (code or residual.dtype != torch.bfloat16 or residual.shape != (M, cols)
                                 or residual.stride(1) != 1):
        raise L.CambrianAmdError(f"{name}: residual is bf16 [M, N] with contiguous rows, and not combined with act")
    out_dtype = out_dtype or (torch.bfloat16 if out is None else out.dtype)
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise L.CambrianAmdError(f"{name}: out_dtype {out_dtype} (bf16 or fp32)")
    if out is None:
        out = torch.empty((M, (cols + 7) // 8 * 8), dtype=out_dtype, device=x.device)[:, :cols]
    elif not out.is_cuda or out.dtype != out_dtype or out.shape != (M, cols) or out.stride(1) != 1:
        raise L.CambrianAmdError(f"{name}: out must be a {out_dtype} GPU tensor [{M}, {cols}] with contiguous rows")
    w_args = []
    for t in weights:
        w_args += (t.data_ptr(), t.stride(0)) if t.dim() == 2 else (t.data_ptr(),)
    L.call("cmb_" + name, x.data_ptr(), x.stride(0), M, L.ptr(norm_weight), float(eps), *w_args, N, K, code,
           L.ptr(residual), 0 if residual is None else residual.stride(0), out.data_ptr(), out.stride(0),
           int(out_dtype == torch.float32), device=x.device)
    return out


def decode_linear(x: torch.Tensor, w: torch.Tensor, *, norm_weight: Optional[torch.Tensor] = None, eps: float = 0.0,
                  act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
                  out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``epilogue(prologue(x) @ w.T)`` for bf16 x [M <= 16, K] and w [N, K] (row views are fine), one launch that reads the
    weights once.  ``norm_weight`` [K]: RMSNorm(x; norm_weight, eps) is the operand (with the default
    ``eps`` = 0 an all-zero row gives NaN, as the stock norm does: pass the model's eps); ``act="swiglu"``: w is packed
    [gate; up] and the result is ``silu(gate) * up`` [M, N / 2] (``swiglu_packed``'s convention); ``residual`` [M, N]: added
    in fp32 before the rounding; ``out_dtype``: bf16 (default) or fp32; ``out``: write into this [M, N'] tensor or row view
    (16-byte aligned, row stride a multiple of 8) instead of a new one.  Inference only: there is no backward."""
    return _decode_linear_launch("decode_linear", decode_linear_supported, x, (w,), (w,),
                                 lambda: f"w {tuple(w.shape)} {w.dtype} strides {w.stride()}",
                                 norm_weight, eps, act, residual, out_dtype, out)


# ------------------------------------------------------------------------------------------------
# the same linears at up to 64 rows (decode_linear_wide.hip): decode steps of 17-64 sequences, or beams.  Opt-in
# (config.decode_linear_wide / CAMBRIAN_AMD_DECODE_LINEAR_WIDE): profiles/decode_linear_wide.md has what was measured.
# ------------------------------------------------------------------------------------------------
DECODE_LINEAR_WIDE_MAX_ROWS = 64


def decode_linear_wide_enabled(config_flag: bool = False) -> bool:
    """Whether decode steps of 17-64 rows run their linears on ``decode_linear_wide`` (five launches per layer) instead of the
    stock sequence: ``CAMBRIAN_AMD_DECODE_LINEAR_WIDE`` = ``1`` / ``0`` in the environment overrides, unset it is
    ``config_flag`` (the model's ``config.decode_linear_wide``, absent = off).  Any other value raises: a typo must not
    silently pick a side.  ``CAMBRIAN_AMD_DECODE_LINEAR=0`` (the stock sequence everywhere) wins over this switch at the
    dispatch sites."""
    return _config_switch("CAMBRIAN_AMD_DECODE_LINEAR_WIDE", config_flag, strict=True)


def decode_linear_wide_rows(rows: int, config_flag: bool = False) -> bool:
    """The dispatch sites' question: do ``rows`` rows of a decode step go to ``decode_linear_wide``?  17-64 rows, the wide
    switch on, and ``CAMBRIAN_AMD_DECODE_LINEAR`` not ``0``."""
    return (DECODE_LINEAR_MAX_ROWS < rows <= DECODE_LINEAR_WIDE_MAX_ROWS and decode_linear_wide_enabled(config_flag)
            and os.environ.get("CAMBRIAN_AMD_DECODE_LINEAR") != "0")


def decode_linear_wide_plan(M: int, N: int, K: int, act: Optional[str] = None, cus: int = 0) -> Tuple[int, int]:
    """(weight rows per workgroup, workgroups) of a ``decode_linear_wide`` call: a pure function of (N, act, CU count);
    ``cus`` = 0 takes the current device's count."""
    return _decode_plan("cmb_decode_linear_wide_plan", M, N, K, act, cus)


def decode_linear_wide_weight_supported(M: int, w: torch.Tensor, act: Optional[str] = None) -> bool:
    """The weight's side of ``decode_linear_wide_supported``, for ``M`` rows of x that are yet to be computed."""
    return (w.dim() == 2 and _decode_linear_rows_ok(w, w.shape[1])
            and bool(L.load().cmb_decode_linear_wide_supported(M, w.shape[0], w.shape[1], _decode_linear_act(act))))


def decode_linear_wide_supported(x: torch.Tensor, w: torch.Tensor, act: Optional[str] = None) -> bool:
    """Whether ``decode_linear_wide(x, w, act=act)`` takes these operands: ``decode_linear_supported``'s conditions with
    x [M <= 64, K]."""
    return (w.dim() == 2 and x.dim() == 2 and x.shape[0] >= 1 and _decode_linear_rows_ok(x, w.shape[1])
            and decode_linear_wide_weight_supported(x.shape[0], w, act))


def decode_linear_wide(x: torch.Tensor, w: torch.Tensor, *, norm_weight: Optional[torch.Tensor] = None, eps: float = 0.0,
                       act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
                       out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``decode_linear`` for bf16 x [M <= 64, K]: the same function, arguments and checks, one launch that reads the weights
    once.  The same inputs give the same bits, and a row's bits depend neither on M nor on the other rows; they are not
    ``decode_linear``'s bits (another order of the same fp32 sum).  Inference only: there is no backward."""
    return _decode_linear_launch("decode_linear_wide", decode_linear_wide_supported, x, (w,), (w,),
                                 lambda: f"w {tuple(w.shape)} {w.dtype} strides {w.stride()}",
                                 norm_weight, eps, act, residual, out_dtype, out)


# ------------------------------------------------------------------------------------------------
# the same linears on weight-only e4m3 weights (decode_linear_fp8.hip): half the weight stream of a decode step.  Opt-in
# (``config.decode_fp8_weights`` / CAMBRIAN_AMD_DECODE_FP8): it changes numerics — row-wise e4m3 weights are about 2.5–2.7 %
# relative L2 error per product on Gaussian weights — and keeps a 1-byte copy of every decoder weight beside the bf16 one.
# ------------------------------------------------------------------------------------------------
DECODE_FP8_MAX_K = 16384       # cmb_quantize_fp8_rows holds a row in registers: K <= 256 threads x 16 x 4 pieces (fp8.hip)


def decode_fp8_enabled(config_flag: bool = False) -> bool:
    """Whether decode steps stream e4m3 weights: ``CAMBRIAN_AMD_DECODE_FP8`` = ``1`` / ``0`` in the environment overrides,
    unset it is ``config_flag`` (the model's ``config.decode_fp8_weights``, absent = off)."""
    return _config_switch("CAMBRIAN_AMD_DECODE_FP8", config_flag)


def decode_linear_fp8_plan(M: int, N: int, K: int, act: Optional[str] = None, cus: int = 0) -> Tuple[int, int]:
    """(weight rows per workgroup, workgroups) of a ``decode_linear_fp8`` call: a pure function of (M, N, K, act, CU
    count); ``cus`` = 0 takes the current device's count."""
    return _decode_plan("cmb_decode_linear_fp8_plan", M, N, K, act, cus)


def decode_linear_fp8_weight_supported(M: int, w: torch.Tensor, act: Optional[str] = None) -> bool:
    """Whether the bf16 weight ``w`` [N, K] can be served by ``decode_fp8_weight`` + ``decode_linear_fp8`` for ``M`` rows of
    x: a GPU bf16 matrix with contiguous, 16-byte aligned rows, K % 16 == 0, K within the quantiser's reach
    (``DECODE_FP8_MAX_K``), and the kernel's shape rule."""
    return (w.dim() == 2 and _decode_linear_rows_ok(w, w.shape[1]) and w.shape[1] <= DECODE_FP8_MAX_K
            and bool(L.load().cmb_decode_linear_fp8_supported(M, w.shape[0], w.shape[1], _decode_linear_act(act))))


def _decode_fp8_q_ok(q: torch.Tensor, inv_scale: torch.Tensor) -> bool:
    return (q.is_cuda and q.dtype == torch.uint8 and q.dim() == 2 and q.stride(1) == 1 and q.stride(0) >= q.shape[1]
            and q.stride(0) % 16 == 0 and q.data_ptr() % 16 == 0 and inv_scale.is_cuda and inv_scale.device == q.device
            and inv_scale.dtype == torch.float32 and inv_scale.shape == (q.shape[0],) and inv_scale.is_contiguous())


def decode_linear_fp8_supported(x: torch.Tensor, q: torch.Tensor, inv_scale: torch.Tensor, act: Optional[str] = None) -> bool:
    """Whether ``decode_linear_fp8(x, q, inv_scale, act=act)`` takes these operands: bf16 GPU x [M <= 16, K], uint8 GPU q
    [N, K] with contiguous 16-byte aligned rows (row stride a multiple of 16), contiguous fp32 inv_scale [N], K % 16 == 0,
    N even for SwiGLU."""
    return (x.dim() == 2 and q.dim() == 2 and x.shape[0] >= 1 and _decode_linear_rows_ok(x, q.shape[1])
            and _decode_fp8_q_ok(q, inv_scale)
            and bool(L.load().cmb_decode_linear_fp8_supported(x.shape[0], q.shape[0], q.shape[1], _decode_linear_act(act))))


def decode_fp8_weight(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """A frozen bf16 GPU weight [N, K] -> (e4m3fn bytes uint8 [N, K], fp32 dequantisation factor [N]) for
    ``decode_linear_fp8``: every row scaled so that its largest magnitude maps to 448 (``k_quantize_fp8_rows``; a zero row
    gets the factor 1).  K % 16 == 0 and K <= ``DECODE_FP8_MAX_K``, the quantiser's limit."""
    L.require_gpu(w)
    if w.requires_grad:
        raise L.CambrianAmdError("decode_fp8_weight: the weight is trainable; quantised copies are for frozen weights")
    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.stride(1) != 1 or w.shape[0] < 1 or w.shape[1] < 16 \
            or w.shape[1] % 16 or w.shape[1] > DECODE_FP8_MAX_K or w.stride(0) % 8 or w.data_ptr() % 16:
        raise L.CambrianAmdError(f"decode_fp8_weight: needs a bf16 [N, K] matrix with contiguous 16-byte aligned rows, "
                                 f"K % 16 == 0 and 16 <= K <= {DECODE_FP8_MAX_K}; got {tuple(w.shape)} {w.dtype} "
                                 f"strides {w.stride()}")
    return k_quantize_fp8_rows(w.detach())


def decode_linear_fp8(x: torch.Tensor, q: torch.Tensor, inv_scale: torch.Tensor, *, norm_weight: Optional[torch.Tensor] = None,
                      eps: float = 0.0, act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
                      out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``decode_linear`` on weight-only e4m3 weights: ``epilogue(inv_scale * (prologue(x) @ e4m3(q).T))`` for bf16 x
    [M <= 16, K], q the uint8 e4m3fn bytes [N, K] (finite: never the NaN codes 0x7F / 0xFF) and inv_scale the fp32 row factors [N] of
    ``decode_fp8_weight``; one
    launch that reads one byte per weight.  ``norm_weight`` / ``eps`` / ``act`` / ``residual`` / ``out_dtype`` / ``out``
    mean what they mean in ``decode_linear``.  Inference only: there is no backward and no CPU path."""
    return _decode_linear_launch("decode_linear_fp8", decode_linear_fp8_supported, x, (q, inv_scale), (inv_scale,),
                                 lambda: f"q {tuple(q.shape)} {q.dtype} strides {q.stride()}, inv_scale "
                                         f"{tuple(inv_scale.shape)} {inv_scale.dtype}",
                                 norm_weight, eps, act, residual, out_dtype, out)


# ------------------------------------------------------------------------------------------------
# the same linears on MXFP4 weights (decode_linear_fp4.hip, mxfp4.hip): OCP e2m1 nibbles with one e8m0 power-of-two scale per
# 32 elements, 4.25 bits per weight — a quarter of the bf16 stream, and 0.53 byte per decoder parameter beside the bf16 weights
# (the e4m3 mode adds 1).  Opt-in (``config.decode_fp4_weights`` / CAMBRIAN_AMD_DECODE_FP4) and COARSE: about 11 % relative L2
# error per weight on Gaussian weights (e4m3 rows: 2.5–2.7 %); task quality on real checkpoints is unmeasured.  Block scales
# need no row in registers, so K has no upper reach (Yi-34B's down_proj, K = 20480, is taken).  Not bitsandbytes' NF4:
# ``load_4bit`` stays refused.
# ------------------------------------------------------------------------------------------------
DECODE_FP4_BLOCK = 32


def decode_fp4_enabled(config_flag: bool = False) -> bool:
    """Whether decode steps stream MXFP4 weights: ``CAMBRIAN_AMD_DECODE_FP4`` = ``1`` / ``0`` in the environment overrides,
    unset it is ``config_flag`` (the model's ``config.decode_fp4_weights``, absent = off)."""
    return _config_switch("CAMBRIAN_AMD_DECODE_FP4", config_flag)


def decode_weight_format(config) -> Optional[str]:
    """The reduced weight format of the decode steps as the two switches resolve it: None (bf16), ``"fp8"`` (e4m3 rows,
    ``config.decode_fp8_weights`` / CAMBRIAN_AMD_DECODE_FP8) or ``"fp4"`` (MXFP4, ``config.decode_fp4_weights`` /
    CAMBRIAN_AMD_DECODE_FP4).  Both on is an error, not a silent pick."""
    fp8 = decode_fp8_enabled(getattr(config, "decode_fp8_weights", False))
    fp4 = decode_fp4_enabled(getattr(config, "decode_fp4_weights", False))
    if fp8 and fp4:
        raise L.CambrianAmdError("decode steps can stream one reduced weight format: both the e4m3 mode (config.decode_fp8_weights / "
                                 "CAMBRIAN_AMD_DECODE_FP8) and the MXFP4 mode (config.decode_fp4_weights / CAMBRIAN_AMD_DECODE_FP4) "
                                 "are switched on; switch one off")
    return "fp8" if fp8 else ("fp4" if fp4 else None)


def decode_linear_fp4_plan(M: int, N: int, K: int, act: Optional[str] = None, cus: int = 0) -> Tuple[int, int]:
    """(weight rows per workgroup, workgroups) of a ``decode_linear_fp4`` call: a pure function of (M, N, K, act, CU
    count); ``cus`` = 0 takes the current device's count."""
    return _decode_plan("cmb_decode_linear_fp4_plan", M, N, K, act, cus)


def decode_linear_fp4_weight_supported(M: int, w: torch.Tensor, act: Optional[str] = None) -> bool:
    """Whether the bf16 weight ``w`` [N, K] can be served by ``decode_fp4_weight`` + ``decode_linear_fp4`` for ``M`` rows of
    x: a GPU bf16 matrix with contiguous, 16-byte aligned rows, K % 32 == 0 (any such K), and the kernel's shape rule."""
    return (w.dim() == 2 and _decode_linear_rows_ok(w, w.shape[1])
            and bool(L.load().cmb_decode_linear_fp4_supported(M, w.shape[0], w.shape[1], _decode_linear_act(act))))


def _decode_fp4_q_ok(q: torch.Tensor, scales: torch.Tensor) -> bool:
    return (q.is_cuda and q.dtype == torch.uint8 and q.dim() == 2 and q.shape[1] >= 16 and q.shape[1] % 16 == 0
            and q.stride(1) == 1 and q.stride(0) >= q.shape[1] and q.stride(0) % 16 == 0 and q.data_ptr() % 16 == 0
            and scales.is_cuda and scales.device == q.device and scales.dtype == torch.uint8 and scales.dim() == 2
            and scales.shape == (q.shape[0], q.shape[1] // 16) and scales.stride(1) == 1 and scales.stride(0) >= scales.shape[1])


def decode_linear_fp4_supported(x: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, act: Optional[str] = None) -> bool:
    """Whether ``decode_linear_fp4(x, q, scales, act=act)`` takes these operands: bf16 GPU x [M <= 16, K], uint8 GPU q
    [N, K / 2] with contiguous 16-byte aligned rows (row stride a multiple of 16), uint8 scales [N, K / 32] with contiguous
    rows, K % 32 == 0, N even for SwiGLU."""
    return (x.dim() == 2 and q.dim() == 2 and x.shape[0] >= 1 and _decode_linear_rows_ok(x, 2 * q.shape[1])
            and _decode_fp4_q_ok(q, scales)
            and bool(L.load().cmb_decode_linear_fp4_supported(x.shape[0], q.shape[0], 2 * q.shape[1], _decode_linear_act(act))))


def k_quantize_mxfp4_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [rows, K] bf16 | fp32 GPU tensor with contiguous rows, finite, K % 32 == 0 -> (uint8 nibbles [rows, K / 2], uint8 e8m0
    scales [rows, K / 32]): MXFP4 under the OCP scale rule (cmb_quantize_mxfp4_rows)."""
    L.require_gpu(x)
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype not in (torch.bfloat16, torch.float32) or x.shape[1] < DECODE_FP4_BLOCK \
            or x.shape[1] % DECODE_FP4_BLOCK:
        raise L.CambrianAmdError("MXFP4 quantisation needs a 2-D K-contiguous bf16 / fp32 tensor with K a multiple of 32")
    rows, K = x.shape
    q = torch.empty(rows, K // 2, dtype=torch.uint8, device=x.device)
    scales = torch.empty(rows, K // DECODE_FP4_BLOCK, dtype=torch.uint8, device=x.device)
    L.call("cmb_quantize_mxfp4_rows", L.dtype_code(x.dtype), x.data_ptr(), x.stride(0), rows, K, q.data_ptr(), K // 2,
           scales.data_ptr(), K // DECODE_FP4_BLOCK, device=x.device, what=f"cmb_quantize_mxfp4_rows({rows}x{K})")
    return q, scales


def decode_fp4_weight(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """A frozen bf16 GPU weight [N, K] -> (e2m1 nibbles uint8 [N, K / 2], e8m0 scales uint8 [N, K / 32]) for
    ``decode_linear_fp4`` (``k_quantize_mxfp4_rows``).  K % 32 == 0; no upper limit on K."""
    L.require_gpu(w)
    if w.requires_grad:
        raise L.CambrianAmdError("decode_fp4_weight: the weight is trainable; quantised copies are for frozen weights")
    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.stride(1) != 1 or w.shape[0] < 1 or w.shape[1] < DECODE_FP4_BLOCK \
            or w.shape[1] % DECODE_FP4_BLOCK or w.stride(0) % 8 or w.data_ptr() % 16:
        raise L.CambrianAmdError(f"decode_fp4_weight: needs a bf16 [N, K] matrix with contiguous 16-byte aligned rows and "
                                 f"K % 32 == 0, K >= 32; got {tuple(w.shape)} {w.dtype} strides {w.stride()}")
    return k_quantize_mxfp4_rows(w.detach())


def decode_linear_fp4(x: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, *, norm_weight: Optional[torch.Tensor] = None,
                      eps: float = 0.0, act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
                      out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``decode_linear`` on MXFP4 weights: ``epilogue(prologue(x) @ (e2m1(q) * 2^(scales - 127)).T)`` for bf16 x [M <= 16, K],
    q the packed nibbles [N, K / 2] and scales the e8m0 bytes [N, K / 32] of ``decode_fp4_weight`` (codes 1 .. 254, never 0 or
    255); one launch that reads 4.25 bits per weight.  ``norm_weight`` / ``eps`` / ``act`` / ``residual`` / ``out_dtype`` /
    ``out`` mean what they mean in ``decode_linear``.  Inference only: there is no backward and no CPU path."""
    return _decode_linear_launch("decode_linear_fp4", decode_linear_fp4_supported, x, (q, scales), (),
                                 lambda: f"q {tuple(q.shape)} {q.dtype} strides {q.stride()}, scales {tuple(scales.shape)} "
                                         f"{scales.dtype} strides {scales.stride()}",
                                 norm_weight, eps, act, residual, out_dtype, out)


# ------------------------------------------------------------------------------------------------
# the whole decode step as one library call (decode_step.hip) and the greedy selection between two steps as another
# (decode_next.hip; decode_sample.hip for sampled decoding, behind a switch of its own: ``config.decode_sample_device`` /
# CAMBRIAN_AMD_DECODE_SAMPLE).  Opt-in (``config.decode_step_fused`` / CAMBRIAN_AMD_DECODE_STEP), off by default: the kernels and
# their arguments are those of the five-launch path, what changes is who issues them.  The wrappers are thin on purpose
# (the point is the host's time per token): the caller — ``cambrian_llama`` — establishes every condition once per
# ``generate()`` call, and the library checks every argument rule again before it launches anything.
# ------------------------------------------------------------------------------------------------
DECODE_STEP_POLL = 8           # with an eos id the host reads ``done`` at most every this many steps
_DECODE_STEP_WS: dict = {}     # device -> fp32 workspace of cmb_decode_step, grown on demand and reused (like _DECODE_WS)


def decode_step_enabled(config_flag: bool = False) -> bool:
    """Whether decode steps of ``generate()`` are issued as one library call per token: ``CAMBRIAN_AMD_DECODE_STEP`` =
    ``1`` / ``0`` in the environment overrides, unset it is ``config_flag`` (the model's ``config.decode_step_fused``,
    absent = off)."""
    return _config_switch("CAMBRIAN_AMD_DECODE_STEP", config_flag)


def decode_step_ws_floats(B: int, H: int, I: int, nh: int, nkv: int, hd: int, t_max: int) -> int:
    """fp32 elements of the workspace ``decode_step`` needs for steps up to cache slot ``t_max``."""
    need = int(L.load().cmb_decode_step_ws(B, H, I, nh, nkv, hd, t_max))
    if need < 0:
        L.check(need, "cmb_decode_step_ws")
    return need


def decode_step_workspace(device, floats: int) -> torch.Tensor:
    """The device's shared workspace, at least ``floats`` long."""
    ws = _DECODE_STEP_WS.get(device)
    if ws is None or ws.numel() < floats:
        ws = _DECODE_STEP_WS[device] = torch.empty(max(int(floats), 4), dtype=torch.float32, device=device)
    return ws


def decode_step(desc, layers, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, t: int, key_valid: torch.Tensor,
                ws: torch.Tensor, logits: torch.Tensor, kv8=None) -> torch.Tensor:
    """One token through every decoder layer and the lm_head: ``desc`` (``lib.DecodeStepDesc``) and ``layers`` (a ctypes
    array of ``lib.DecodeLayer``) describe the model, x bf16 [B, H], cos / sin the fp32 tables of ``rope_table``, ``t`` the
    cache slot, key_valid bool / uint8 [B, >= t+1], ``ws`` from ``decode_step_workspace``; fp32 logits [B, V] are written
    into ``logits`` (row stride a multiple of 8) and returned.  ``kv8``: None, or (a ctypes array of ``lib.DecodeKv8Factors``,
    i_sb, i_sh) when ``layers`` hold e4m3 caches and ``desc`` their byte strides (``cmb_decode_step_kv8``).  Inference only."""
    if kv8 is not None:
        factors, i_sb, i_sh = kv8
        L.call("cmb_decode_step_kv8", C.byref(desc), layers, factors, i_sb, i_sh, x.data_ptr(), x.stride(0), cos.data_ptr(),
               sin.data_ptr(), t, key_valid.data_ptr(), key_valid.stride(0), ws.data_ptr(), ws.numel(), logits.data_ptr(),
               logits.stride(0), device=x.device)
        return logits
    L.call("cmb_decode_step", C.byref(desc), layers, x.data_ptr(), x.stride(0), cos.data_ptr(), sin.data_ptr(), t,
           key_valid.data_ptr(), key_valid.stride(0), ws.data_ptr(), ws.numel(), logits.data_ptr(), logits.stride(0),
           device=x.device)
    return logits


def decode_next(logits: torch.Tensor, eos: int, done: Optional[torch.Tensor], out_ids: torch.Tensor, step: int,
                n_tok: torch.Tensor, pos: torch.Tensor, key_valid: torch.Tensor, t: int, embed: torch.Tensor, x: torch.Tensor,
                hd: int, rope_base: float, cos: torch.Tensor, sin: torch.Tensor) -> None:
    """Greedy selection and the next step's inputs in one launch (+ the RoPE-table launch): per row ``nxt = argmax(logits)``
    (fp32 [B, V], any row stride; torch.argmax's tie and NaN rules), with ``eos`` >= 0 (-1: none) ``nxt = done ? eos : nxt;
    done |= nxt == eos``; writes ``out_ids[:, step] = nxt`` (int64), ``pos = n_tok + step`` (int64 [B]), ``key_valid[:, t] =
    1``, ``x = embed[nxt]`` (bf16 rows) and cos / sin = ``rope_table(pos)``.  Every tensor is the caller's, on one GPU."""
    B, V = logits.shape
    L.call("cmb_decode_next", logits.data_ptr(), logits.stride(0), B, V, eos, L.ptr(done), out_ids.data_ptr(), out_ids.stride(0),
           step, n_tok.data_ptr(), pos.data_ptr(), key_valid.data_ptr(), key_valid.stride(0), t, embed.data_ptr(),
           embed.stride(0), embed.shape[0], embed.shape[1], x.data_ptr(), x.stride(0), hd, rope_base, cos.data_ptr(),
           sin.data_ptr(), device=logits.device)


def decode_sample_enabled(config_flag: bool = False) -> bool:
    """Whether sampled decoding of ``generate()`` selects its tokens on the device (``decode_sample``) where the one-call decode
    step runs: ``CAMBRIAN_AMD_DECODE_SAMPLE`` = ``1`` / ``0`` in the environment overrides, unset it is ``config_flag`` (the
    model's ``config.decode_sample_device``, absent = off)."""
    return _config_switch("CAMBRIAN_AMD_DECODE_SAMPLE", config_flag)


def decode_sample(logits: torch.Tensor, inv_temperature: float, top_k: int, top_p: float, seed: torch.Tensor, eos: int,
                  done: Optional[torch.Tensor], out_ids: torch.Tensor, step: int, n_tok: torch.Tensor, pos: torch.Tensor,
                  key_valid: torch.Tensor, t: int, embed: torch.Tensor, x: torch.Tensor, hd: int, rope_base: float,
                  cos: torch.Tensor, sin: torch.Tensor, thr: Optional[torch.Tensor] = None,
                  n_keep: Optional[torch.Tensor] = None) -> None:
    """``decode_next`` with the argmax replaced by a filtered random draw, in one launch (+ the RoPE-table launch): per row
    ``z = logits * inv_temperature``, top-k (``top_k`` 0 = off; ties at the k-th value kept), top-p over what top-k kept
    (``top_p`` 1 = off; equal values kept or dropped together), then Gumbel-max with Philox4x32-10 noise keyed by ``seed`` (one
    int64 in DEVICE memory) and counted by (element, row, ``step``).  A row whose maximum is not finite takes its argmax.
    ``thr`` fp32 [B] / ``n_keep`` int32 [B]: optional outputs, the threshold and how many elements passed it.  Everything else
    as ``decode_next``; the semantics are spelled out at ``cmb_decode_sample`` in include/cambrian_amd.h."""
    B, V = logits.shape
    L.call("cmb_decode_sample", logits.data_ptr(), logits.stride(0), B, V, inv_temperature, top_k, top_p, seed.data_ptr(), eos,
           L.ptr(done), out_ids.data_ptr(), out_ids.stride(0), step, n_tok.data_ptr(), pos.data_ptr(), key_valid.data_ptr(),
           key_valid.stride(0), t, embed.data_ptr(), embed.stride(0), embed.shape[0], embed.shape[1], x.data_ptr(), x.stride(0),
           hd, rope_base, cos.data_ptr(), sin.data_ptr(), L.ptr(thr), L.ptr(n_keep), device=logits.device)


def decode_process_enabled(config_flag: bool = False) -> bool:
    """Whether ``generate()`` takes the logits processors that read the generated ids (``repetition_penalty``,
    ``no_repeat_ngram_size``, ``min_new_tokens``, ``bad_words_ids``, ``suppress_tokens``) and a list ``eos_token_id``, and runs
    them on the device (``decode_process``): ``CAMBRIAN_AMD_DECODE_PROCESS`` = ``1`` / ``0`` in the environment overrides, unset
    it is ``config_flag`` (the model's ``config.decode_logits_processors``, absent = off).  Any other value raises."""
    return _config_switch("CAMBRIAN_AMD_DECODE_PROCESS", config_flag, strict=True)


class DecodeProcess:
    """One ``generate()`` call's processors on the device: the ``processors.ProcessSpec`` and its lists (eos ids, single-id
    bans, the word table), uploaded once."""

    def __init__(self, spec, device):
        self.spec = spec
        self.eos, self.bans, self.word_ids, self.word_off = spec.device_lists(device)
        self.n_eos, self.n_bans, self.n_words = len(spec.eos), len(spec.bans), len(spec.words)
        self.n_word_ids = 0 if self.word_ids is None else self.word_ids.numel()


def decode_process(logits: torch.Tensor, hist: Optional[torch.Tensor], n_hist: int, proc: DecodeProcess,
                   done: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The logits processors of ``proc`` on fp32 ``logits`` [B, V] (unit column stride, any row stride and alignment) IN PLACE,
    in one launch: ``hist`` int64 [B, >= n_hist] holds each row's generated ids (None with ``n_hist`` 0), ``done`` bool / uint8
    [B] is set where the row's last id is in the eos set.  Run it before ``decode_next`` / ``decode_sample`` or the argmax of
    the same step; the rule is spelled out at ``cmb_decode_process`` in include/cambrian_amd.h and restated in
    ``processors.apply_torch``.  Returns ``logits``."""
    L.require_gpu(logits, hist, done)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise L.CambrianAmdError("decode_process: logits is an fp32 [B, V] tensor with unit column stride")
    if hist is not None and (hist.dtype != torch.int64 or hist.dim() != 2 or hist.stride(1) != 1 or hist.shape[0] != logits.shape[0]):
        raise L.CambrianAmdError("decode_process: hist is an int64 [B, n] tensor with unit column stride")
    if done is not None and (done.dtype not in (torch.bool, torch.uint8) or done.shape != (logits.shape[0],) or not done.is_contiguous()):
        raise L.CambrianAmdError("decode_process: done is a contiguous bool / uint8 [B] tensor")
    B, V = logits.shape
    s = proc.spec
    L.call("cmb_decode_process", logits.data_ptr(), logits.stride(0), B, V, L.ptr(hist), 0 if hist is None else hist.stride(0),
           n_hist, s.penalty, s.ngram, s.min_new, L.ptr(proc.eos), proc.n_eos, L.ptr(proc.bans), proc.n_bans,
           L.ptr(proc.word_ids), proc.n_word_ids, L.ptr(proc.word_off), proc.n_words, L.ptr(done), device=logits.device)
    return logits


def trim_after_all_done_set(ids: torch.Tensor, eos: Sequence[int]) -> torch.Tensor:
    """``trim_after_all_done`` for an eos SET: a row is done from its first id that is in ``eos`` on.  The fused loops mark a
    row that ends on a secondary eos one step late, so the columns are searched for ids of the set, not for ``eos[0]``."""
    if ids.shape[1] == 0:
        return ids
    from .model.language_model.processors import first_in_set
    hit = torch.nonzero(first_in_set(ids, eos).all(dim=0))
    return ids if hit.numel() == 0 else ids[:, :int(hit[0, 0]) + 1]


def decode_beam_enabled(config_flag: bool = False) -> bool:
    """Whether ``generate(num_beams > 1)`` runs beam search (on the device, ``decode_beam``, where the one-call decode step
    runs; else on the per-launch loop around model/language_model/beam.py) instead of raising: ``CAMBRIAN_AMD_DECODE_BEAM`` =
    ``1`` / ``0`` in the environment overrides, unset it is ``config_flag`` (the model's ``config.decode_beam_search``, absent =
    off).  Any other value raises: a typo must not silently pick a side."""
    return _config_switch("CAMBRIAN_AMD_DECODE_BEAM", config_flag, strict=True)


DECODE_BEAM_MAX = 16           # CMB_BEAM_MAX of csrc/decode_beam_core.h: beams of one prompt, and rows of a fused decode step


class DecodeBeamState:
    """The state block of ``decode_beam`` (``cmb_decode_beam`` in include/cambrian_amd.h documents the layout): one zeroed
    uint8 tensor ``buf`` per ``generate()`` call, every section a view into it, plus the ``unfinished`` byte.  ``view(n)`` gives
    the state after ``n`` steps in the shape of ``beam.BeamState`` ([prompts, num_beams, ...]) for ``beam.beam_result``."""

    def __init__(self, prompts: int, num_beams: int, max_new: int, device):
        need = int(L.load().cmb_decode_beam_state_bytes(prompts, num_beams, max_new))
        if need < 0:
            L.check(need, "cmb_decode_beam_state_bytes")
        self.prompts, self.num_beams, self.max_new = prompts, num_beams, max_new
        self.buf = torch.zeros(need + 16, dtype=torch.uint8, device=device)     # the last 16 bytes: the `unfinished` byte
        R, K, f32, i32, u8 = prompts * num_beams, 2 * num_beams, torch.float32, torch.int32, torch.uint8
        at = 0
        for name, dtype, shape in (("run_score", f32, (R,)), ("fin_score", f32, (R,)), ("fin_len", i32, (R,)), ("parent", i32, (R,)),
                                   ("tok", i32, (R,)), ("cand_lp", f32, (R, K)), ("cand_tok", i32, (R, K)), ("fin_ok", u8, (R,)),
                                   ("unsat", u8, (prompts,)), ("all_hit", u8, (prompts,)),
                                   ("run_ids2", torch.int64, (2, R, max_new)), ("fin_ids", torch.int64, (R, max_new))):
            n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()      # cmb_beam_make_layout's order and rounding
            setattr(self, name, self.buf[at:at + n].view(dtype).view(shape))
            at += (n + 15) // 16 * 16
        if at != need:
            raise L.CambrianAmdError(f"decode_beam: the state block's layout ({at} bytes) is not the library's ({need})")
        self.bytes = need
        self.unfinished = self.buf[need:need + 1]

    def view(self, steps: int):
        from .model.language_model.beam import BeamState
        P, nb, M = self.prompts, self.num_beams, self.max_new
        st = BeamState.__new__(BeamState)
        st.run_ids = self.run_ids2[steps & 1].view(P, nb, M)
        st.run_score, st.fin_score = self.run_score.view(P, nb), self.fin_score.view(P, nb)
        st.fin_ids, st.fin_len = self.fin_ids.view(P, nb, M), self.fin_len.view(P, nb)
        st.fin_ok, st.unsat, st.all_hit = self.fin_ok.view(P, nb).bool(), self.unsat.bool(), self.all_hit.bool()
        return st


def decode_beam(logits: torch.Tensor, num_beams: int, eos: int, state: DecodeBeamState, step: int, n_tok: torch.Tensor,
                pos: torch.Tensor, key_valid: torch.Tensor, t: int, embed: torch.Tensor, x: torch.Tensor, hd: int,
                rope_base: float, cos: torch.Tensor, sin: torch.Tensor, desc=None, layers=None, L0: int = 0) -> None:
    """One step of beam search and the next decode step's inputs in one library call: ``logits`` fp32 [prompts * num_beams, V]
    of the running beams (row ``prompt * num_beams + slot``), ``state`` the call's ``DecodeBeamState``, ``step`` 0-based with
    ``state.max_new`` steps at most (the last one finishes every candidate), ``eos`` -1 = none.  Updates ``state`` as
    ``beam.beam_update`` does, writes ``pos``, ``key_valid[:, t]``, ``x = embed[token]``, cos / sin as ``decode_next``, and with
    ``desc`` / ``layers`` (a ``DecodeStepPlan``'s) moves every layer's K / V of the generated columns ``L0 .. t - 1`` from each
    beam's parent row to its own, in place.  ``state.unfinished`` (a device byte) says whether the search goes on."""
    R, V = logits.shape
    L.call("cmb_decode_beam", logits.data_ptr(), logits.stride(0), R, num_beams, V, eos, state.buf.data_ptr(), state.bytes, step,
           state.max_new, n_tok.data_ptr(), pos.data_ptr(), key_valid.data_ptr(), key_valid.stride(0), t, embed.data_ptr(),
           embed.stride(0), embed.shape[0], embed.shape[1], x.data_ptr(), x.stride(0), hd, rope_base, cos.data_ptr(),
           sin.data_ptr(), None if desc is None else C.byref(desc), layers, L0, state.unfinished.data_ptr(), device=logits.device)


def decode_beam_reorder(desc, layers, parent: torch.Tensor, num_beams: int, L0: int, t: int) -> None:
    """The cache half of ``decode_beam`` on its own: in every layer's K / V cache of ``desc`` / ``layers`` and for the columns
    ``L0 <= c < t``, row ``prompt * num_beams + i`` takes the values of row ``prompt * num_beams + parent[...]`` (int32 GPU
    [rows]), in place; nothing else is written."""
    L.require_gpu(parent)
    if parent.dtype != torch.int32 or parent.shape != (desc.B,) or not parent.is_contiguous():
        raise L.CambrianAmdError(f"decode_beam_reorder: parent is a contiguous int32 [{desc.B}] tensor")
    L.call("cmb_decode_beam_reorder", C.byref(desc), layers, parent.data_ptr(), num_beams, L0, t, device=parent.device)


def trim_after_all_done(ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """``ids`` [B, n] of a greedy loop that ran past the point where every row had produced ``eos_token_id`` (it polls
    ``done`` only every ``DECODE_STEP_POLL`` steps): the columns up to and including the first one at which every row is done
    — a row is done from its first eos on — which is where a loop that tests ``done.all()`` after every token stops.  All
    of ``ids`` when no such column exists."""
    if ids.shape[1] == 0:
        return ids
    all_done = ((ids == eos_token_id).long().cumsum(dim=1) > 0).all(dim=0)
    hit = torch.nonzero(all_done)
    return ids if hit.numel() == 0 else ids[:, :int(hit[0, 0]) + 1]


# ================================================================================================
# optimizer: global gradient norm and the one-pass AdamW step (optim.hip) over lists of tensors
# ================================================================================================
# Both kernels read a job table in device memory, one job per tensor.  The table is cached on a signature of every pointer
# in it and uploaded again only when one moves (gradients freed by zero_grad() usually come back at the same addresses from
# the caching allocator); the upload goes through a pinned host copy and does not block, so a step never waits for the
# device.  The partials of the norm live in one workspace per device, grown on demand and reused.
OPTIM_CHUNK = 65536        # CMB_OPTIM_CHUNK of csrc/optim_core.h (tests/test_optim_host.py checks it against cmb_optim_chunks)
_OPTIM_TABLES: dict = {}   # signature -> (device table, its pinned host copy, n_jobs, total_chunks)
_OPTIM_WS: dict = {}       # device -> fp32 workspace of the chunk partials


def _optim_check(name: str, t: torch.Tensor, numel: int, dev: torch.device, dtypes) -> None:
    if t.device != dev or t.numel() != numel or t.dtype not in dtypes or not t.is_contiguous():
        raise L.CambrianAmdError(f"optimizer kernels: {name} must be a contiguous {' / '.join(str(d) for d in dtypes)} tensor "
                                 f"of {numel} elements on {dev}; got {tuple(t.shape)} {t.dtype} on {t.device}"
                                 f"{'' if t.is_contiguous() else ', not contiguous'}")


def _optim_table(grads, params=None, lows=None, exp_avgs=None, exp_avg_sqs=None):
    """(device job table, n_jobs, total_chunks) of a list of tensors; every tensor is validated here, since the library cannot
    look into a table that lives in device memory."""
    n = len(grads)
    dev = grads[0].device
    rows = []
    for i, g in enumerate(grads):
        _optim_check("a gradient", g, g.numel(), dev, (torch.float32, torch.bfloat16))
        p = m = v = low = None
        if params is not None:
            p, m, v = params[i], exp_avgs[i], exp_avg_sqs[i]
            low = lows[i] if lows is not None else None
            _optim_check("a parameter / master", p, g.numel(), dev, (torch.float32,))
            _optim_check("exp_avg", m, g.numel(), dev, (torch.float32,))
            _optim_check("exp_avg_sq", v, g.numel(), dev, (torch.float32,))
            if low is not None:
                _optim_check("the low-precision copy", low, g.numel(), dev, (torch.bfloat16,))
        rows.append((g.data_ptr(), L.ptr(p) or 0, L.ptr(low) or 0, L.ptr(m) or 0, L.ptr(v) or 0, g.numel(), L.dtype_code(g.dtype)))
    sig = (dev, tuple(rows))
    hit = _OPTIM_TABLES.get(sig)
    if hit is None:
        lib = L.load()
        jobs = (L.OptimJob * n)()
        chunk0 = 0
        for i, (gp, pp, lp, mp, vp, numel, code) in enumerate(rows):
            j = jobs[i]
            j.grad, j.param, j.low, j.exp_avg, j.exp_avg_sq = gp, pp or None, lp or None, mp or None, vp or None
            j.n, j.chunk0, j.grad_dtype, j.reserved = numel, chunk0, code, 0
            chunk0 += lib.cmb_optim_chunks(numel)
        host = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).pin_memory()
        if len(_OPTIM_TABLES) >= 64:   # pointers that keep moving: do not collect stale tables without bound
            _OPTIM_TABLES.clear()
        hit = _OPTIM_TABLES[sig] = (host.to(dev, non_blocking=True), host, n, chunk0)
    return hit[0], hit[2], hit[3]


def grad_sqnorm(grads: Sequence[torch.Tensor]) -> torch.Tensor:
    """Sum of squares of every element of ``grads`` (fp32 / bf16 tensors on one device, any sizes, views at any element
    offset) as an fp32 device scalar: the square of the global L2 norm ``torch.nn.utils.clip_grad_norm_`` clips by.  The
    same bits on every run and for every placement of the same values; the host does not wait for it."""
    grads = list(grads)
    if not grads:
        raise L.CambrianAmdError("grad_sqnorm: an empty list has no device to put the result on")
    L.require_gpu(*grads)
    grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
    table, n, chunks = _optim_table(grads)
    dev = grads[0].device
    need = int(L.load().cmb_grad_sqnorm_workspace(chunks))
    ws = _OPTIM_WS.get(dev)
    if ws is None or ws.numel() < max(need, 1):
        ws = _OPTIM_WS[dev] = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    L.call("cmb_grad_sqnorm", table.data_ptr(), n, chunks, ws.data_ptr(), ws.numel(), out.data_ptr(), device=dev)
    return out


def adamw_step(grads: Sequence[torch.Tensor], params: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
               exp_avg_sqs: Sequence[torch.Tensor], lows: Optional[Sequence[Optional[torch.Tensor]]] = None, *, lr: float,
               beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0,
               sumsq: Optional[torch.Tensor] = None, max_norm: float = 0.0) -> None:
    """One launch of torch.optim.AdamW's update, in place, over a list of tensors that share their hyper-parameters and
    their step count ``step`` (>= 1, the count INCLUDING this step).  ``params`` / moments fp32, ``grads`` fp32 or bf16,
    ``lows[i]``: the bf16 compute copy of ``params[i]`` to refresh in the same pass, or None.  The gradient enters as
    ``g * grad_scale * coef`` with ``coef = min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6))`` when ``sumsq`` (the fp32
    device scalar of ``grad_sqnorm``) is given and ``max_norm`` > 0, else 1; ``sumsq`` is read on the device."""
    grads, params, exp_avgs, exp_avg_sqs = list(grads), list(params), list(exp_avgs), list(exp_avg_sqs)
    if not (len(grads) == len(params) == len(exp_avgs) == len(exp_avg_sqs)) or (lows is not None and len(lows) != len(grads)):
        raise L.CambrianAmdError("adamw_step: the lists differ in length")
    if step < 1:
        raise L.CambrianAmdError("adamw_step: step counts from 1")
    if not grads:
        return
    L.require_gpu(*grads, *params, *exp_avgs, *exp_avg_sqs, *(lows or ()), sumsq)
    if sumsq is not None and (sumsq.dtype != torch.float32 or sumsq.numel() != 1 or sumsq.device != grads[0].device):
        raise L.CambrianAmdError("adamw_step: sumsq is the fp32 device scalar of grad_sqnorm")
    table, n, chunks = _optim_table(grads, params, lows, exp_avgs, exp_avg_sqs)
    dev = grads[0].device
    L.call("cmb_adamw_step", table.data_ptr(), n, chunks, lr, beta1, beta2, eps, weight_decay, 1.0 - beta1 ** step,
           1.0 - beta2 ** step, grad_scale, L.ptr(sumsq), max_norm, device=dev)


# ================================================================================================
# bilinear token-grid resample that back-propagates on our own kernels (elementwise.hip: resample_kernel and its adjoint
# resample_bwd_kernel) — the trainable towers' 27^2 -> 24^2 / multi-stage -> 96^2 resize and the S5 query-group resize
# ================================================================================================
def resample_enabled() -> bool:
    """``CAMBRIAN_AMD_RESAMPLE_BWD=0`` in the environment: every resize that carries a gradient (and the eval-path query-group
    resize) takes the ATen body — permute, fp32 up-cast, ``F.interpolate``, cast, permute (A/B runs)."""
    return L.env_flag("CAMBRIAN_AMD_RESAMPLE_BWD", True)


def resample_supported(dtype: torch.dtype, channels: int) -> bool:
    """What ``cmb_resample_bilinear`` / ``_bwd`` take: bf16 / fp32 rows of a multiple of 8 channels."""
    return dtype in (torch.bfloat16, torch.float32) and channels > 0 and channels % 8 == 0


def _resample_aten(x: torch.Tensor, hi: int, wi: int, ho: int, wo: int) -> torch.Tensor:
    """The reference's own resize (clip_encoder.py:83-88, cambrian_arch.py:395-401): NCHW, fp32, align_corners=False."""
    B, _, C = x.shape
    y = x.reshape(B, hi, wi, C).permute(0, 3, 1, 2)
    y = F.interpolate(y.to(torch.float32), size=(ho, wo), mode="bilinear", align_corners=False).to(x.dtype)
    return y.permute(0, 2, 3, 1).reshape(B, ho * wo, C)


def _vec8_rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when the kernels' 16-byte row accesses can walk it in place (unit last stride, every other stride a
    multiple of 8 elements, an aligned base), else a contiguous copy."""
    if t.stride(-1) == 1 and all(st % 8 == 0 for st in t.stride()[:-1]) and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def k_resample(x: torch.Tensor, hi: int, wi: int, out: torch.Tensor, ho: int, wo: int, col_offset: int = 0) -> None:
    """x [B, hi*wi, C] -> out[:, :, col_offset:col_offset+C] with out [B, ho*wo, Ctot] (bilinear, fp32 lerp)."""
    L.require_gpu(x, out)
    B, T, C = x.shape
    assert T == hi * wi and out.shape[0] == B and out.shape[1] == ho * wo and x.stride(2) == 1 and out.stride(2) == 1
    optr = out.data_ptr() + col_offset * out.element_size()
    L.call("cmb_resample_bilinear", L.dtype_code(x.dtype), x.data_ptr(), B, hi, wi, C, x.stride(1), x.stride(0), optr, ho, wo,
           out.stride(1), out.stride(0), device=x.device)


def k_resample_bwd(dout: torch.Tensor, ho: int, wo: int, dx: torch.Tensor, hi: int, wi: int, col_offset: int = 0) -> None:
    """Adjoint of ``k_resample``: dout[:, :, col_offset:col_offset+C] with dout [B, ho*wo, Ctot] -> dx [B, hi*wi, C], written in
    full (cells no output refers to get 0).  Gather form in a fixed order: no atomics, bit-reproducible."""
    L.require_gpu(dout, dx)
    B, T, C = dx.shape
    assert T == hi * wi and dout.shape[0] == B and dout.shape[1] == ho * wo and dx.stride(2) == 1 and dout.stride(2) == 1
    assert dout.dtype == dx.dtype and 0 <= col_offset and col_offset + C <= dout.shape[2]
    gptr = dout.data_ptr() + col_offset * dout.element_size()
    L.call("cmb_resample_bilinear_bwd", L.dtype_code(dx.dtype), gptr, B, ho, wo, C, dout.stride(1), dout.stride(0), dx.data_ptr(),
           hi, wi, dx.stride(1), dx.stride(0), device=dx.device)


def _resample_maps(maps: Sequence[torch.Tensor], side: int) -> torch.Tensor:
    """maps [B, Hs, Ws, Cs] -> a new [B, side*side, sum Cs]: one ``k_resample`` per map into its column slice of the one buffer."""
    B = maps[0].shape[0]
    out = torch.empty((B, side * side, sum(m.shape[3] for m in maps)), dtype=maps[0].dtype, device=maps[0].device)
    off = 0
    for m in maps:
        _, Hs, Ws, Cs = m.shape
        k_resample(_vec8_rows(m.reshape(B, Hs * Ws, Cs)), Hs, Ws, out, side, side, col_offset=off)
        off += Cs
    return out


class ResampleBilinearFn(torch.autograd.Function):
    """x [B, hi*wi, C] (strided rows are read in place) -> [B, ho*wo, C]; backward = the adjoint gather kernel."""

    @staticmethod
    def forward(ctx, x, hi: int, wi: int, ho: int, wo: int):
        x = _vec8_rows(x)
        B, _, C = x.shape
        out = torch.empty((B, ho * wo, C), dtype=x.dtype, device=x.device)
        k_resample(x, hi, wi, out, ho, wo)
        ctx.grids = (hi, wi, ho, wo)
        return out

    @staticmethod
    def backward(ctx, g):
        hi, wi, ho, wo = ctx.grids
        g = _vec8_rows(g)
        dx = torch.empty((g.shape[0], hi * wi, g.shape[2]), dtype=g.dtype, device=g.device)
        k_resample_bwd(g, ho, wo, dx, hi, wi)
        return dx, None, None, None, None


def resample_bilinear(x: torch.Tensor, hi: int, wi: int, ho: int, wo: int) -> torch.Tensor:
    """Bilinear resize (fp32 lerp, align_corners=False) of the token grid x [B, hi*wi, C] to [B, ho*wo, C], channels-last both
    ways; ``x`` itself when the grids are equal.  Differentiable: forward ``cmb_resample_bilinear``, backward its exact adjoint
    ``cmb_resample_bilinear_bwd`` (deterministic, no fp32 NCHW copies).  The ATen body runs instead under
    ``CAMBRIAN_AMD_RESAMPLE_BWD=0`` and for inputs the kernels do not take."""
    if x.dim() != 3 or x.shape[1] != hi * wi:
        raise L.CambrianAmdError(f"resample_bilinear: x {tuple(x.shape)} is not [B, {hi}*{wi}, C]")
    if (hi, wi) == (ho, wo):
        return x
    if not (resample_enabled() and resample_supported(x.dtype, x.shape[2])):
        return _resample_aten(x, hi, wi, ho, wo)
    return ResampleBilinearFn.apply(x, hi, wi, ho, wo)


class ResampleConcatFn(torch.autograd.Function):
    """maps[s] NHWC [B, Hs, Ws, Cs] -> [B, side*side, sum Cs]: one forward launch per map into its column slice of the one
    buffer, one backward launch per map that needs a gradient, reading its slice of the incoming gradient in place."""

    @staticmethod
    def forward(ctx, side: int, *maps):
        ctx.side, ctx.shapes = side, [tuple(m.shape) for m in maps]
        return _resample_maps(maps, side)

    @staticmethod
    def backward(ctx, g):
        g = _vec8_rows(g)
        grads, off = [], 0
        for k, (B, Hs, Ws, Cs) in enumerate(ctx.shapes):
            dx = None
            if ctx.needs_input_grad[1 + k]:
                dx = torch.empty((B, Hs * Ws, Cs), dtype=g.dtype, device=g.device)
                k_resample_bwd(g, ctx.side, ctx.side, dx, Hs, Ws, col_offset=off)
                dx = dx.view(B, Hs, Ws, Cs)
            grads.append(dx)
            off += Cs
        return (None, *grads)


def resample_concat(maps: Sequence[torch.Tensor], out_side: int) -> torch.Tensor:
    """The ConvNeXt multi-stage output (clip_convnext_encoder.py:99-119,143): every map [B, Hs, Ws, Cs] bilinearly resized to
    out_side x out_side and channel-concatenated, [B, out_side^2, sum Cs], as ONE differentiable operator — no per-map
    output, no ``torch.cat``, and a backward that reads the concatenated gradient where it lies."""
    maps = list(maps)
    if not maps or any(m.dim() != 4 or m.shape[0] != maps[0].shape[0] or m.dtype != maps[0].dtype for m in maps):
        raise L.CambrianAmdError("resample_concat: maps are [B, Hs, Ws, Cs] tensors of one batch size and dtype")
    if not (resample_enabled() and all(resample_supported(m.dtype, m.shape[3]) for m in maps)):
        B = maps[0].shape[0]
        return torch.cat([_resample_aten(m.reshape(B, m.shape[1] * m.shape[2], m.shape[3]), m.shape[1], m.shape[2], out_side,
                                         out_side) for m in maps], -1)
    return ResampleConcatFn.apply(out_side, *maps)


class AddRmsNormFn(torch.autograd.Function):
    """(s, y) = (x + delta, rmsnorm(x + delta) * w) in one pass — the decoder layer's "h = h + attn; mlp_in = norm(h)".
    Backward: d(x) = d(delta) = g_s + rmsnorm_backward(g_y), also one pass when the weight is frozen."""

    @staticmethod
    def forward(ctx, x, delta, weight, eps: float):
        L.require_gpu(x, delta, weight)
        shape = x.shape
        D = shape[-1]
        x2, d2 = x.reshape(-1, D), delta.reshape(-1, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        d2 = d2 if d2.is_contiguous() else d2.contiguous()
        if d2.dtype != x2.dtype:
            d2 = d2.to(x2.dtype)
        w32 = k_cast(weight, torch.float32)
        s, y, rstd = k_add_rmsnorm_fwd(x2, d2, w32, eps)
        ctx.save_for_backward(s, w32, rstd)
        ctx.shape, ctx.w_dtype = shape, weight.dtype
        return s.view(shape), y.view(shape)

    @staticmethod
    def backward(ctx, g_s, g_y):
        s, w32, rstd = ctx.saved_tensors
        rows, D = s.shape
        if g_y is None:
            return g_s, g_s, None, None
        gy = _as_dtype_contig(g_y.reshape(rows, D), s.dtype)
        gs = None if g_s is None else _as_dtype_contig(g_s.reshape(rows, D), s.dtype)
        dx, dw = k_rmsnorm_bwd(gy, s, w32, rstd, add=gs, want_dw=ctx.needs_input_grad[2])
        dx = dx.view(ctx.shape)    # one tensor for two inputs: not marked as handed to one receiver (RmsNormForkFn)
        return dx, dx, _param_grad(dw, ctx.w_dtype), None


def add_rmsnorm(x, delta, weight, eps: float = 1e-6):
    return AddRmsNormFn.apply(x, delta, weight, eps)


# ================================================================================================
# linear over channel-concatenated resized stage maps with the resize commuted behind the projection: bilinear resizing acts
# on positions, the linear on channels, so R_s(X_s) W_s^T = R_s(X_s W_s^T).  A stage with fewer positions than the output
# grid is projected at its own resolution and only the N-wide product is resized and summed (cmb_resample_accum); at the
# ConvNeXt-XXL aux projector (stages 64^2 and 32^2 hold 4608 of 5760 channels, output 96^2) the forward and weight-gradient
# GEMM work falls from 2.61 to 0.98 TFLOP per step and the resized stage-3/4 channels are never written.  Opt-in.
# ================================================================================================
def commuted_proj_enabled(config=None) -> bool:
    """``CAMBRIAN_AMD_COMMUTED_PROJ=1`` in the environment (read at call time) or ``config.mm_commuted_aux_projection``.
    Off by default: every path is then exactly what it was."""
    return L.env_flag("CAMBRIAN_AMD_COMMUTED_PROJ", False) or bool(getattr(config, "mm_commuted_aux_projection", False))


# partial products (the dense stages' ``base`` and every commuted stage's Y_s) in fp32: the pre-activation is then rounded
# once, as in the one unfused GEMM (CPU emulation: error 0.74-0.94 x the unfused path's; with bf16 partials 0.75-1.36 x).  The
# price is the wider base / Y_s traffic of cmb_resample_accum.  CAMBRIAN_AMD_COMMUTED_PROJ_F32=0 keeps them in the compute
# dtype (A/B runs, tools/bench_commuted_proj.py).
def _commuted_f32_partials() -> bool:
    return L.env_flag("CAMBRIAN_AMD_COMMUTED_PROJ_F32", True)


def stage_maps_plan(grids, out_side: int) -> List[bool]:
    """Which stages of ``linear_stage_maps`` are commuted (True: projected at their own resolution, product resized) and
    which are dense (False: resized first): a stage is commuted iff it has fewer positions than the output grid.  ``grids``
    holds a side or an (H, W) pair per stage.  Pure: no tensors, no device."""
    out = []
    for g in grids:
        h, w = (g, g) if isinstance(g, int) else g
        out.append(h * w < out_side * out_side)
    return out


def k_resample_accum(out: torch.Tensor, ho: int, wo: int, *, base: Optional[torch.Tensor] = None,
                     bias: Optional[torch.Tensor] = None, srcs: Sequence[Tuple[torch.Tensor, int, int]] = (),
                     pre_out: Optional[torch.Tensor] = None, act: int = L.ACT_NONE) -> torch.Tensor:
    """out = act(base + bias + sum_s bilinear(src_s -> ho x wo)) on cmb_resample_accum.  ``out`` / ``pre_out`` / ``base`` are
    [B, ho*wo, C] (column slices of wider buffers are walked in place), ``srcs`` a list of (x [B, hi*wi, C], hi, wi), ``bias``
    fp32 [C].  base and the sources share one dtype: ``out``'s, or fp32 under a bf16 ``out``."""
    tens = [t for t in (base, pre_out) if t is not None] + [s[0] for s in srcs]
    L.require_gpu(out, bias, *tens)
    if out.dim() != 3 or out.shape[1] != ho * wo or any(t.dim() != 3 or t.stride(2) != 1 for t in [out] + tens):
        raise L.CambrianAmdError("resample_accum: operands are [B, positions, C] with a unit channel stride")
    B, _, Cc = out.shape
    for t in (base, pre_out):
        if t is not None and tuple(t.shape) != (B, ho * wo, Cc):
            raise L.CambrianAmdError("resample_accum: base / pre_out must have the shape of out")
    if pre_out is not None and pre_out.dtype != out.dtype:
        raise L.CambrianAmdError("resample_accum: pre_out has the dtype of out")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != Cc):
        raise L.CambrianAmdError("resample_accum: bias must be contiguous fp32 [C]")
    if len(srcs) > L.RESAMPLE_ACCUM_MAX_SRC:
        raise L.CambrianAmdError(f"resample_accum: at most {L.RESAMPLE_ACCUM_MAX_SRC} sources")
    src_t = [base] if base is not None else []
    src_t += [s[0] for s in srcs]
    sdt = src_t[0].dtype if src_t else out.dtype
    if any(t.dtype != sdt for t in src_t):
        raise L.CambrianAmdError("resample_accum: base and the sources share one dtype")
    d = L.ResampleAccumDesc()
    d.dtype, d.src_dtype, d.act, d.n_src = L.dtype_code(out.dtype), L.dtype_code(sdt), act, len(srcs)
    d.B, d.Ho, d.Wo, d.C = B, ho, wo, Cc
    d.base = L.ptr(base)
    d.ld_base, d.batch_stride_base = (base.stride(1), base.stride(0)) if base is not None else (0, 0)
    d.bias = L.ptr(bias)
    for k, (x, hi, wi) in enumerate(srcs):
        if tuple(x.shape) != (B, hi * wi, Cc):
            raise L.CambrianAmdError(f"resample_accum: source {k} is {tuple(x.shape)}, not [{B}, {hi}*{wi}, {Cc}]")
        d.src[k], d.Hi[k], d.Wi[k], d.ld_src[k], d.batch_stride_src[k] = x.data_ptr(), hi, wi, x.stride(1), x.stride(0)
    d.pre_out = L.ptr(pre_out)
    d.ld_pre, d.batch_stride_pre = (pre_out.stride(1), pre_out.stride(0)) if pre_out is not None else (0, 0)
    d.out, d.ld_out, d.batch_stride_out = out.data_ptr(), out.stride(1), out.stride(0)
    L.call("cmb_resample_accum", C.byref(d), device=out.device)
    return out


def _rows2d(m: torch.Tensor) -> torch.Tensor:
    """NHWC map [B, H, W, C] as GEMM rows [B*H*W, C] (in place when the 16-byte row accesses can walk it)."""
    x = m.reshape(-1, m.shape[-1])
    if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        x = x.contiguous()
    return x


def concat_stage_maps(maps: Sequence[torch.Tensor], out_side: int) -> torch.Tensor:
    """maps [B, Hs, Ws, Cs] -> [B, out_side^2, sum Cs]: the towers' own multi-stage output.  Maps that carry no gradient
    (frozen towers) go through ``cmb_resample_bilinear`` directly, as ConvNeXtTrunk.forward does; the rest through the
    differentiable ``resample_concat``."""
    maps = list(maps)
    if torch.is_grad_enabled() and any(m.requires_grad for m in maps):
        return resample_concat(maps, out_side)
    return _resample_maps(maps, out_side)


class StageMaps:
    """What a multi-stage tower hands the projector when the resize is to be commuted behind the projection: the stage maps
    [B, Hs, Ws, Cs] and the side of the common output grid, instead of their resized concatenation.  ``shape`` / ``dtype`` /
    ``device`` are those of the tensor ``concat()`` returns — the tower's ordinary [B, side^2, sum Cs] output."""

    def __init__(self, maps: Sequence[torch.Tensor], side: int):
        self.maps, self.side = list(maps), int(side)

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.maps[0].shape[0], self.side * self.side, sum(m.shape[3] for m in self.maps)))

    @property
    def dtype(self) -> torch.dtype:
        return self.maps[0].dtype

    @property
    def device(self) -> torch.device:
        return self.maps[0].device

    @property
    def requires_grad(self) -> bool:
        return any(m.requires_grad for m in self.maps)

    def concat(self) -> torch.Tensor:
        return concat_stage_maps(self.maps, self.side)


class LinearStageMapsFn(torch.autograd.Function):
    """act(concat_s R_s(X_s) @ W^T + b) with the commuted stages projected at their own resolution (see the section head)."""

    @staticmethod
    def forward(ctx, side: int, weight, bias, act: int, f32_partials: bool, *maps):
        dt, dev = maps[0].dtype, maps[0].device
        B, N, P = maps[0].shape[0], weight.shape[0], side * side
        shapes = [tuple(m.shape) for m in maps]
        plan = stage_maps_plan([(s[1], s[2]) for s in shapes], side)
        offs = [0]
        for s in shapes:
            offs.append(offs[-1] + s[3])
        prep = prepared_weight(weight, dt)
        w_c, w_t = prep if prep is not None else (k_cast(weight, dt), None)
        b_c = None if bias is None else k_cast(bias, torch.float32)
        pdt = torch.float32 if f32_partials else dt
        dense = [k for k, c in enumerate(plan) if not c]
        xd = base = None
        if dense:   # resized first, as today, into one buffer; one GEMM over their (contiguous) weight columns
            d0, d1 = offs[dense[0]], offs[dense[-1] + 1]
            xd = _resample_maps([maps[k] for k in dense], side)      # [B, P, d1 - d0]: the dense stages are neighbours
            base = k_gemm(xd.view(B * P, d1 - d0), w_c[:, d0:d1], out_dtype=pdt).view(B, P, N)
        srcs, xs = [], []
        for k, c in enumerate(plan):
            if not c:
                continue
            _, Hs, Ws, Cs = shapes[k]
            x = _rows2d(maps[k])
            xs.append(x)
            srcs.append((k_gemm(x, w_c[:, offs[k]:offs[k + 1]], out_dtype=pdt).view(B, Hs * Ws, N), Hs, Ws))
        need_pre = act != L.ACT_NONE and any(ctx.needs_input_grad)
        out = torch.empty((B * P, N), dtype=dt, device=dev)
        pre = torch.empty((B * P, N), dtype=dt, device=dev) if need_pre else None
        k_resample_accum(out.view(B, P, N), side, side, base=base, bias=b_c, srcs=srcs,
                         pre_out=None if pre is None else pre.view(B, P, N), act=act)
        ctx.side, ctx.act, ctx.shapes, ctx.plan, ctx.offs, ctx.dense = side, act, shapes, plan, offs, dense
        ctx.has_bias, ctx.w_dtype, ctx.b_dtype = bias is not None, weight.dtype, None if bias is None else bias.dtype
        ctx.has_wt = w_t is not None
        ctx.save_for_backward(w_c, w_t, pre, xd, *xs)
        return out

    @staticmethod
    def backward(ctx, dy):
        w_c, w_t, pre, xd, *xs = ctx.saved_tensors
        side, shapes, plan, offs, dense = ctx.side, ctx.shapes, ctx.plan, ctx.offs, ctx.dense
        dt = w_c.dtype
        B, P, N = shapes[0][0], side * side, w_c.shape[0]
        need_w, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        need_m = list(ctx.needs_input_grad[5:])
        g = _as_dtype_contig(dy, dt)
        if ctx.act != L.ACT_NONE:
            g = k_act_bwd(g, pre, ctx.act)
        g3 = g.view(B, P, N)
        dw = torch.empty((N, offs[-1]), dtype=torch.float32, device=g.device) if need_w else None
        if any(need_m) and w_t is None:
            w_t = k_transpose(w_c, N)                                   # [sum C, N]
        grads = [None] * len(shapes)
        if dense:
            d0, d1 = offs[dense[0]], offs[dense[-1] + 1]
            if need_w:
                _wgrad_into(g, xd.view(B * P, d1 - d0), dw[:, d0:d1])
            if any(need_m[k] for k in dense):                           # g W_dense, pushed through the adjoint resample
                dxd = k_gemm(g, w_t[d0:d1, :N]).view(B, P, d1 - d0)
                for k in dense:
                    if need_m[k]:
                        _, Hs, Ws, Cs = shapes[k]
                        dx = torch.empty((B, Hs * Ws, Cs), dtype=dt, device=g.device)
                        k_resample_bwd(dxd, side, side, dx, Hs, Ws, col_offset=offs[k] - d0)
                        grads[k] = dx.view(B, Hs, Ws, Cs)
        xi = 0
        for k, c in enumerate(plan):
            if not c:
                continue
            x = xs[xi]
            xi += 1
            if not (need_w or need_m[k]):
                continue
            _, Hs, Ws, Cs = shapes[k]
            gs = torch.empty((B, Hs * Ws, N), dtype=dt, device=g.device)  # g_s = R_s^T g: the adjoint kernel on the shared d(pre)
            k_resample_bwd(g3, side, side, gs, Hs, Ws)
            gs = gs.view(B * Hs * Ws, N)
            if need_w:
                _wgrad_into(gs, x, dw[:, offs[k]:offs[k + 1]])
            if need_m[k]:
                grads[k] = k_gemm(gs, w_t[offs[k]:offs[k + 1], :N]).view(B, Hs, Ws, Cs)
        dw = _param_grad(dw, ctx.w_dtype)
        db = _param_grad(k_colsum(g), ctx.b_dtype) if need_b else None
        return (None, dw, db, None, None, *grads)


def stage_maps_fusable(maps: Sequence[torch.Tensor], out_side: int, weight: torch.Tensor, bias: Optional[torch.Tensor],
                       act: int) -> bool:
    """What the commuted path takes: bf16 / fp32 NHWC maps of one batch on the GPU, at least one commuted stage and at most
    ``RESAMPLE_ACCUM_MAX_SRC`` of them, dense stages that own one contiguous run of weight columns, every channel count and
    N a multiple of the GEMM's K step (weight column slices are read in place through ``ldb``), no activation but erf-GELU."""
    maps = list(maps)
    if not maps or any(m.dim() != 4 or not m.is_cuda or m.shape[0] != maps[0].shape[0] or m.dtype != maps[0].dtype for m in maps):
        return False
    dt = maps[0].dtype
    if dt not in (torch.bfloat16, torch.float32) or act not in (L.ACT_NONE, L.ACT_GELU_ERF):
        return False
    ks = _kstep(dt)
    if (weight.dim() != 2 or not weight.is_cuda or weight.stride(1) != 1 or weight.shape[1] != sum(m.shape[3] for m in maps)
            or weight.dtype not in (torch.float32, dt) or weight.shape[0] % ks or any(m.shape[3] % ks for m in maps)):
        return False
    if bias is not None and (not bias.is_cuda or bias.numel() != weight.shape[0]):
        return False
    plan = stage_maps_plan([(m.shape[1], m.shape[2]) for m in maps], out_side)
    dense = [k for k, c in enumerate(plan) if not c]
    if not any(plan) or sum(plan) > L.RESAMPLE_ACCUM_MAX_SRC or (dense and dense != list(range(dense[0], dense[-1] + 1))):
        return False
    return True


def linear_stage_maps(maps: Sequence[torch.Tensor], out_side: int, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      act: int = L.ACT_NONE, heavy: bool = False, enabled: Optional[bool] = None) -> torch.Tensor:
    """``linear(resample_concat(maps, out_side).reshape(-1, sum Cs), weight, bias, act)`` -> [B * out_side^2, N], with the
    resize of every stage that has fewer positions than the output grid commuted behind its slice of the projection
    (``stage_maps_plan``).  ``weight`` is the one [N, sum Cs] parameter; its gradient comes back whole.  The unfused
    composition runs when the switch is off (``enabled``; None = ``commuted_proj_enabled()``), no stage would be commuted,
    an input is something the kernels do not take, or ``fp8_projections`` is active for this (``heavy``) projector."""
    maps = list(maps)
    on = commuted_proj_enabled() if enabled is None else enabled
    if not (on and not (heavy and _FP8_LINEAR) and stage_maps_fusable(maps, out_side, weight, bias, act)):
        x = concat_stage_maps(maps, out_side)
        return linear(x.reshape(-1, x.shape[-1]), weight, bias, act=act, heavy=heavy)
    return LinearStageMapsFn.apply(out_side, weight, bias, act, _commuted_f32_partials(), *maps)
