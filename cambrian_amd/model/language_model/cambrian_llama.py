"""Cambrian-Llama on MI355X — counterpart of ``cambrian/model/language_model/cambrian_llama.py``.

What is on the hot path here:
  * the in-LLM SVA hook (:168-207, static branch): after decoder layer ``start + k*stride`` the 576 latent-query
    rows of ``hidden[:, image_position : image_position+600]`` (24x25 grid, newline column skipped) go through
    ``vision_sampler_layers[k]`` and are written back in place — one strided gather kernel, the fused SVA layer,
    one strided scatter kernel;
  * RMSNorm (the reference's patched fp32 version, train_fsdp.py:1429-1438) and RoPE as HIP kernels;
  * fp32 logits + shifted cross-entropy exactly as :402-422.
The decoder's own GEMMs / causal attention stay stock PyTorch-ROCm (hipBLASLt, SDPA) per the north star; the
reference file's decoder loop is written against the transformers==4.37 tuple API and does not run on the installed
transformers 5.x, so the loop is re-stated here with HF-compatible parameter names
(``model.layers.{i}.self_attn.q_proj.weight`` ...).
"""
from __future__ import annotations

import os

import math
import weakref
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint as _checkpoint

try:  # HF config class only (no HF modelling code is used)
    from transformers import LlamaConfig
    from transformers.modeling_outputs import CausalLMOutputWithPast
except Exception:  # pragma: no cover - transformers is part of the image
    LlamaConfig = object
    CausalLMOutputWithPast = None

from ... import lib as _lib
from ... import ops
from ...constants import IGNORE_INDEX, IMAGE_TOKEN_INDEX
from ..cambrian_arch import CambrianMetaForCausalLM, CambrianMetaModel, SvaContext
from . import processors as PROC
from .beam import BeamState, beam_done, beam_fill, beam_result, beam_update


class CambrianConfig(LlamaConfig):
    model_type = "cambrian_llama"
    debug = "debug"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        # transformers 5.x folds rope_theta into `rope_parameters`; keep the 4.37 attribute the reference reads
        if not hasattr(self, "rope_theta"):
            rp = getattr(self, "rope_parameters", None) or {}
            self.rope_theta = float(rp.get("rope_theta", kwargs.get("rope_theta", 10000.0)))


class SvaDynamic:
    """In-LLM SVA inputs of the eval / generate branch: the reference-format lists of cambrian_arch.py:422-451."""

    def __init__(self, feats, masks, final_size, ctx):
        self.feats, self.masks, self.final_size, self.ctx = list(feats), list(masks), list(final_size), ctx


class HipRMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-6, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.variance_epsilon = eps

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.variance_epsilon)


def _fused_frozen_weight(owner: nn.Module, key: str, mods) -> Optional[torch.Tensor]:
    """[W_0; W_1; ...] of several bias-free nn.Linear whose weights are FROZEN (the pre-training stage freezes the
    whole LLM, train_fsdp.py:1677-1685), cached on ``owner`` and rebuilt when a weight moves or changes.  One GEMM with
    N = sum(N_i) then replaces len(mods) GEMMs forward and, in the backward, len(mods) dX GEMMs plus the adds that
    accumulate them.  Trainable or biased projections return None (callers keep the separate-GEMM path); parameter
    names / state_dict keys stay HF's (q_proj.weight, ...)."""
    ws = [m.weight for m in mods]
    if any(w.requires_grad for w in ws) or any(m.bias is not None for m in mods):
        return None
    if getattr(owner, "_cmb_no_weight_cache", False):
        return None  # ZeRO-3 unit: a cached concatenation would keep the whole layer resident on every rank
    tag = tuple((w.data_ptr(), w._version, w.dtype) for w in ws)
    cached = owner.__dict__.get(key)
    if cached is None or cached[0] != tag:
        cached = (tag, torch.cat([w.detach() for w in ws], dim=0).contiguous())
        owner.__dict__[key] = cached
    return cached[1]


class FrozenLinearFn(torch.autograd.Function):
    """y = x @ W^T (+ residual) for a FROZEN W [N,K], with the backward dX = g @ W computed as ``F.linear(g, W_t)`` on a
    cached transposed copy W_t [K,N].  hipBLASLt is fastest when both operands are contiguous along the contraction
    dimension (tools/mm_layout_probe.py: 1.34-1.64 PFLOP/s for that form against 1.36-1.41 for ``g @ W`` at the decoder's
    shapes), which the forward already is; the copy gives the backward the same form (-12 % on every decoder dX GEMM) for
    one more resident copy of the frozen weights (15 GB of the 288 GB for Llama-3-8B)."""

    @staticmethod
    def forward(ctx, x2, w, w_t, res2, out_shape):
        """2-D operands, result written into a FRESH tensor of the caller's N-D ``out_shape`` (the GEMM's ``out=`` is its
        2-D view; no autograd is recorded in here).  The result is therefore NOT a view: the SVA hook's in-place scatter
        into a decoder layer's output stays a plain in-place op — on a ``y2d.view(B, S, H)`` made outside, autograd wraps
        it in CopySlices (a clone and a copy of [B, S, H] per hook in the backward, and the gradient tensor the hook's
        scatter returns is no longer the one the layer receives)."""
        ctx.save_for_backward(w_t)
        ctx.has_res = res2 is not None
        out = torch.empty(out_shape, dtype=x2.dtype, device=x2.device)
        o2 = out.view(-1, w.shape[0])
        if res2 is None:
            torch.mm(x2, w.t(), out=o2)
        else:
            torch.addmm(res2, x2, w.t(), out=o2)
        return out

    @staticmethod
    def backward(ctx, g):
        (w_t,) = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        dx = F.linear(g2, w_t) if ctx.needs_input_grad[0] else None
        return dx, None, None, (g2 if ctx.has_res else None), None


def _frozen_transposed(owner: nn.Module, key: str, w: torch.Tensor) -> torch.Tensor:
    """W^T (contiguous) of a frozen weight, cached on ``owner`` and rebuilt when the weight moves or changes."""
    tag = (w.data_ptr(), w._version, w.dtype)
    cached = owner.__dict__.get(key)
    if cached is None or cached[0] != tag:
        cached = (tag, w.detach().t().contiguous())
        owner.__dict__[key] = cached
    return cached[1]


def frozen_linear(owner: nn.Module, key: str, x: torch.Tensor, w: torch.Tensor, residual: Optional[torch.Tensor] = None):
    """``F.linear(x, w)`` (+ residual); frozen bias-free GPU weights take FrozenLinearFn, anything else the stock path."""
    if w.requires_grad or not x.is_cuda or getattr(owner, "_cmb_no_weight_cache", False):
        # (ZeRO-3 units: no transposed copy either — the layer's storage is dropped between its uses, zero3.py)
        y = F.linear(x, w)
        return y if residual is None else residual + y
    x2 = x.reshape(-1, x.shape[-1])
    res2 = None if residual is None else residual.reshape(-1, w.shape[0])
    if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
        return FrozenLinearFn.apply(x2, w, _frozen_transposed(owner, key, w), res2, (*x.shape[:-1], w.shape[0]))
    # eval / generate: nothing will be back-propagated, so no transposed copy is made or kept
    y = F.linear(x2, w) if res2 is None else torch.addmm(res2, x2, w.t())
    return y.view(*x.shape[:-1], w.shape[0])


def _lin(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """nn.Linear forward; frozen bias-free weights go through FrozenLinearFn (faster dX)."""
    if lin.bias is not None:
        return lin(x)
    return frozen_linear(lin, "_w_t", x, lin.weight)


def _down_proj(lin: nn.Linear, inner: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
    if lin.bias is not None:
        y = lin(inner)
        return y if residual is None else residual + y
    return frozen_linear(lin, "_w_t", inner, lin.weight, residual)   # skip connection inside the GEMM (C = residual)


class LlamaMLP(nn.Module):
    def __init__(self, cfg, device, dtype):
        super().__init__()
        kw = dict(bias=False, device=device, dtype=dtype)
        self.gate_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, **kw)
        self.up_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, **kw)
        self.down_proj = nn.Linear(cfg.intermediate_size, cfg.hidden_size, **kw)

    def forward(self, x, residual=None):
        """``residual``: the layer's skip connection — added by the down-projection GEMM itself (C = residual, beta = 1)
        instead of a separate elementwise pass over [tokens, hidden]."""
        w_gu = _fused_frozen_weight(self, "_w_gate_up", (self.gate_proj, self.up_proj))
        if w_gu is not None and x.is_cuda:
            inner = ops.swiglu_packed(frozen_linear(self, "_w_gate_up_t", x, w_gu))
        else:
            inner = ops.swiglu(self.gate_proj(x), self.up_proj(x))
        return _down_proj(self.down_proj, inner, residual)


class KeyPadding:
    """The decoder's attention mask when it is "causal AND key-padding, diagonal open" (every collator batch without a
    sliding window): carried as the [B, S] key mask so the HIP flash kernels can apply it tile by tile; ``dense()`` builds
    the [B, 1, S, S] boolean mask for the stock kernel (what the reference's HF decoder materialises,
    cambrian_llama.py:142-166)."""

    def __init__(self, key_valid: torch.Tensor):
        self.key_valid = key_valid.to(torch.bool)
        self._dense = None

    def dense(self) -> torch.Tensor:
        if self._dense is None:
            B, S = self.key_valid.shape
            dev = self.key_valid.device
            m = torch.ones(S, S, dtype=torch.bool, device=dev).tril_()[None, None] & self.key_valid[:, None, None, :]
            # a fully masked query row would be NaN in SDPA; padded rows attend to themselves (their loss is ignored)
            self._dense = m | torch.eye(S, dtype=torch.bool, device=dev)[None, None]
        return self._dense


def use_decode_kernel(x: torch.Tensor, nh: int, nkv: int, hd: int) -> bool:
    """Whether a decode step runs on ``ops.decode_attention``: GPU tensors, a geometry the kernel takes, nothing to
    back-propagate, and not switched off with ``CAMBRIAN_AMD_DECODE_ATTN=0`` (A/B against the SDPA body)."""
    return (x.is_cuda and ops.decode_attention_enabled() and ops.decode_attention_supported(x.dtype, nh, nkv, hd)
            and not (torch.is_grad_enabled() and x.requires_grad))


def use_extend_kernel(x: torch.Tensor, nh: int, nkv: int, hd: int, Q: int) -> bool:
    """Whether a chunk of Q tokens runs on ``ops.extend_attention``: ``use_decode_kernel``'s conditions (so
    ``CAMBRIAN_AMD_DECODE_ATTN=0`` switches it off too) and a geometry ``cmb_extend_attn`` takes, which is bf16 only."""
    return use_decode_kernel(x, nh, nkv, hd) and ops.extend_attention_supported(x.dtype, nh, nkv, hd, Q)


def _frozen_plain(*mods) -> bool:
    """Bias-free modules whose weights are frozen and may be kept (no ZeRO-3 unit drops their storage between uses)."""
    return not any(m.weight.requires_grad or getattr(m, "bias", None) is not None
                   or getattr(m, "_cmb_no_weight_cache", False) for m in mods)


def decode_linear_weights(x: torch.Tensor, w_qkv, w_o, w_gate_up, w_down, norms, wide: bool = False) -> bool:
    """The weights' side of "this decode step runs as five launches" (``ops.decode_linear`` around
    ``ops.decode_attention``): the four (packed) weights present and taken by the kernel for x's rows, the norms frozen bf16
    vectors.  Callers have checked the rest: bf16 x of at most 16 sequences inside the ``use_decode_kernel`` arm, and the
    switch (``ops.decode_linear_enabled``) on for this batch.  ``wide``: the same question put to ``ops.decode_linear_wide``
    (17-64 rows, ``decode_wide_rows``)."""
    B = x.shape[0]
    if any(w is None for w in (w_qkv, w_o, w_gate_up, w_down)):
        return False
    if any(n.weight.requires_grad or n.weight.dtype != torch.bfloat16 for n in norms):
        return False
    if wide:
        return (ops.decode_linear_wide_supported(x.reshape(B, -1), w_qkv) and ops.decode_linear_wide_weight_supported(B, w_o)
                and ops.decode_linear_wide_weight_supported(B, w_gate_up, "swiglu")
                and ops.decode_linear_wide_weight_supported(B, w_down))
    return (ops.decode_linear_supported(x.reshape(B, -1), w_qkv) and ops.decode_linear_weight_supported(B, w_o)
            and ops.decode_linear_weight_supported(B, w_gate_up, "swiglu") and ops.decode_linear_weight_supported(B, w_down))


def decode_wide_rows(holder, rows: int) -> bool:
    """Whether a decode step of ``rows`` rows takes ``ops.decode_linear_wide`` in the place of ``ops.decode_linear``: 17-64
    rows, the wide switch on (``config.decode_linear_wide`` of the config ``holder`` was built from, or
    CAMBRIAN_AMD_DECODE_LINEAR_WIDE), and CAMBRIAN_AMD_DECODE_LINEAR not 0.  Off, which is the default, or at 16 rows and
    fewer, no dispatch site behaves differently.  What the step does NOT take at these rows: the e4m3 / MXFP4 weight streams
    (17-64 rows run the bf16 wide kernel and no quantised copy is made for them, exactly as none is made above 16 rows
    without the switch), the one-call step (``DecodeStepPlan.build`` keeps refusing more than 16 rows, so such a batch stays
    on the per-launch loop) and prompt lookup (16 rows at most).  The e4m3 K / V cache works through
    ``ops.decode_attention_any`` as at 16 rows.  fp32 models, trainable or biased projections and more than 64 rows keep the
    stock sequence."""
    if rows <= ops.DECODE_LINEAR_MAX_ROWS:
        return False
    cfg = holder.__dict__.get("_decode_cfg")               # a decoder layer; the language model has .config
    if cfg is None:
        cfg = getattr(holder, "config", None)
    return ops.decode_linear_wide_rows(rows, getattr(cfg, "decode_linear_wide", False))


def _decode_fp8_tag(w: torch.Tensor):
    return (w.data_ptr(), w._version, w.dtype)             # _frozen_transposed's tag


def _decode_quant_copies(fmt: str, holder: nn.Module, B: int, entries):
    """The quantised copies a decode step streams in the format ``fmt`` ("fp8": (e4m3 bytes, fp32 row factors) per linear,
    "fp4": (e2m1 nibbles, e8m0 block scales)), or None when ONE weight is refused: the step then runs on the bf16 weights and
    nothing is quantised or kept.  ``entries``: (owner, key, w, act) per linear; a copy is cached on ``owner`` under ``key``
    with _frozen_transposed's tag and the weight itself (so a replaced packed weight cannot hand its address on), and
    rebuilt when the weight moves or changes.  Every weight that needs a new copy is put to
    ``ops.decode_linear_<fmt>_weight_supported`` BEFORE any is quantised; a refusal is remembered on ``holder`` against the
    same tags, so the following steps ask nothing again, and stale copies of a refused set are dropped."""
    refused = "_decode_" + fmt + "_refused"
    tags = tuple(_decode_fp8_tag(w) for _, _, w, _ in entries)
    if holder.__dict__.get(refused) == tags:
        return None
    cached = [owner.__dict__.get(key) for owner, key, _, _ in entries]
    miss = [i for i, (c, tag) in enumerate(zip(cached, tags)) if c is None or c[0] != tag]
    if miss:
        supported = getattr(ops, "decode_linear_" + fmt + "_weight_supported")        # looked up when a step runs
        if not all(supported(B, entries[i][2], entries[i][3]) for i in miss):
            holder.__dict__[refused] = tags
            for owner, key, _, _ in entries:
                owner.__dict__.pop(key, None)
            return None
        holder.__dict__.pop(refused, None)
        quantise = getattr(ops, "decode_" + fmt + "_weight")
        for i in miss:
            owner, key, w, _ = entries[i]
            cached[i] = owner.__dict__[key] = (tags[i], quantise(w), w)
    return [c[1] for c in cached]


def decode_fp8_copies(holder: nn.Module, B: int, entries):
    """``_decode_quant_copies`` for e4m3.  Kept as a public name; the model code calls that function with the format."""
    return _decode_quant_copies("fp8", holder, B, entries)


def decode_fp4_copies(holder: nn.Module, B: int, entries):
    """``_decode_quant_copies`` for MXFP4 (a refusal: K % 32 != 0).  Kept as a public name, like ``decode_fp8_copies``."""
    return _decode_quant_copies("fp4", holder, B, entries)


def decode_layer_fused(layer, x, cos, sin, kcache, vcache, t, key_mask, w_qkv, w_o, w_gate_up, w_down, fp8=None, fp4=None,
                       linear=None):
    """The five launches of a decode step: norm + QKV projection, attention on the cache, o_proj + skip connection,
    norm + gate / up projection + SwiGLU, down_proj + skip connection.  ``fp8``: the four (bytes, factors) pairs of
    ``decode_fp8_copies`` — the linears then stream those instead of the bf16 weights.  ``fp4``: the four (nibbles, scales)
    pairs of ``decode_fp4_copies``, likewise (``fp4`` wins when both are given).  ``linear``: the bf16 linear,
    ``ops.decode_linear`` unless given (``ops.decode_linear_wide`` at 17-64 rows)."""
    return _five_launches(layer, x, (w_qkv, w_o, w_gate_up, w_down), fp8 if fp4 is None else fp4, fp4 is not None, linear,
                          ops.decode_attention_any, cos, sin, kcache, vcache, t, key_mask)


def _five_launches(layer, x, w, quant, fp4, linear, attend, *cache_args):
    """The one body of ``decode_layer_fused`` / ``decode_layer_fused_multi`` and the layers' ``decode``: x [rows, 1, H] through
    the bf16 weights ``w`` on ``linear`` (None: ``ops.decode_linear``) or, given ``quant``, their e4m3 (``fp4``: MXFP4) copies,
    around ``attend`` on the three views of the QKV row and ``cache_args`` (cos, sin, the caches, the slot, the key mask)."""
    if quant is None:
        lin, mats = (ops.decode_linear if linear is None else linear), ((w[0],), (w[1],), (w[2],), (w[3],))
    else:
        lin, mats = (ops.decode_linear_fp4 if fp4 else ops.decode_linear_fp8), quant
    attn = layer.self_attn
    rows = x.shape[0]
    nq, nk = attn.nh * attn.hd, attn.nkv * attn.hd
    n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
    x2 = x.reshape(rows, -1)
    row = lin(x2, *mats[0], norm_weight=n1.weight, eps=n1.variance_epsilon)
    o = attend(row[:, :nq], row[:, nq:nq + nk], row[:, nq + nk:], *cache_args)
    x2 = lin(o, *mats[1], residual=x2)
    inner = lin(x2, *mats[2], norm_weight=n2.weight, eps=n2.variance_epsilon, act="swiglu")
    return lin(inner, *mats[3], residual=x2).reshape(rows, 1, -1)


def lookup_mask(key_mask: torch.Tensor, t0: int, Q: int) -> torch.Tensor:
    """bool [Q, t0 + Q]: what token j of a multi-token step may attend — cached slots s < t0 under ``key_mask[0]``, the step's
    own slots t0 .. t0 + j always (``cmb_decode_attn_multi``'s rule; columns >= t0 of ``key_mask`` are not looked at)."""
    m = torch.empty(Q, t0 + Q, dtype=torch.bool, device=key_mask.device)
    m[:, :t0] = key_mask[0, :t0]
    m[:, t0:] = torch.ones(Q, Q, dtype=torch.bool, device=key_mask.device).tril()
    return m


def decode_layer_fused_multi(layer, x, cos, sin, kcache, vcache, t0, key_mask, w, quant=None, fp4=False):
    """``decode_layer_fused`` for Q consecutive tokens of ONE sequence, x [Q, 1, H]: the same five launches with
    ``ops.decode_attention_multi`` in the middle.  ``w``: the four bf16 weights; ``quant``: their e4m3 (``fp4``: MXFP4) copies,
    streamed instead when given."""
    return _five_launches(layer, x, w, quant, fp4, None, ops.decode_attention_multi, cos, sin, kcache, vcache, t0, key_mask)


def decode_multi_fused_or_none(layer, x, cos, sin, kcache, vcache, t0, key_mask, fp8, fp4):
    """The five-launch arm of a layer's ``decode_multi``, or None where it does not apply: ``decode``'s own five-launch
    conditions for Q rows (``decode_operands``), bf16 caches and a geometry ``ops.decode_attention_multi`` takes."""
    a = layer.self_attn
    if isinstance(kcache, ops.KvCacheE4M3) or not ops.decode_attention_multi_supported(x.dtype, a.nh, a.nkv, a.hd, x.shape[0]):
        return None
    found = layer.decode_operands(x, fp8, fp4)
    if found is None:
        return None
    return decode_layer_fused_multi(layer, x, cos, sin, kcache, vcache, t0, key_mask, found[0], found[1], fp4=bool(fp4))


def decode_step_operands(layer, x, fp8: bool = False, fp4: bool = False):
    """THE condition under which a decoder layer runs a decode step of x [B, 1, H] as five launches: (the four bf16 weights,
    their quantised copies or None, wide), or None for the stock sequence.  ``decode`` and ``decode_operands`` of both layer
    classes ask here, so the per-launch loop and ``DecodeStepPlan`` cannot disagree.  ``fp4`` / ``fp8`` ask for the MXFP4 /
    e4m3 copies (``fp4`` wins); None stands in their place when one weight is refused, and at wide rows
    (``decode_wide_rows``), which stream the bf16 weights on ``ops.decode_linear_wide`` and get no quantised copy."""
    a = layer.self_attn
    B = x.shape[0]
    wide = decode_wide_rows(layer, B)
    if not (x.dtype == torch.bfloat16 and (wide or (B <= ops.DECODE_LINEAR_MAX_ROWS and ops.decode_linear_enabled(B)))
            and use_decode_kernel(x, a.nh, a.nkv, a.hd)):
        return None
    fmt = None if wide else ("fp4" if fp4 else ("fp8" if fp8 else None))
    w, entries = layer.decode_entries(fmt)
    if not decode_linear_weights(x, *w, (layer.input_layernorm, layer.post_attention_layernorm), wide):
        return None
    return w, (None if fmt is None else _decode_quant_copies(fmt, layer, B, entries)), wide


class LlamaAttention(nn.Module):
    def __init__(self, cfg, device, dtype):
        super().__init__()
        self.nh, self.nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        self.hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        kw = dict(bias=getattr(cfg, "attention_bias", False), device=device, dtype=dtype)
        self.q_proj = nn.Linear(cfg.hidden_size, self.nh * self.hd, **kw)
        self.k_proj = nn.Linear(cfg.hidden_size, self.nkv * self.hd, **kw)
        self.v_proj = nn.Linear(cfg.hidden_size, self.nkv * self.hd, **kw)
        self.o_proj = nn.Linear(self.nh * self.hd, cfg.hidden_size, **kw)

    def forward(self, x, cos, sin, attn_mask, kv_out: Optional[list] = None):
        """``kv_out``: if a list, (k, v) [B,nkv,S,hd] (post-RoPE) are appended — the prefill of ``generate()``."""
        B, S, _ = x.shape
        w_qkv = _fused_frozen_weight(self, "_w_qkv", (self.q_proj, self.k_proj, self.v_proj))
        if w_qkv is not None and x.is_cuda:
            q, k, v = ops.qkv_rope(frozen_linear(self, "_w_qkv_t", x, w_qkv), cos, sin, self.nh, self.nkv, self.hd)
            if kv_out is not None:
                kv_out.append((k, v))
            # attn_mask is None (plain causal) or a KeyPadding marker (causal AND the collator's key mask, diagonal open):
            # both run on flash_bwd.hip; only a dense mask (sliding window) falls through to the stock kernel
            key_valid = attn_mask.key_valid if isinstance(attn_mask, KeyPadding) else None
            if (attn_mask is None or key_valid is not None) and torch.is_grad_enabled() and q.requires_grad \
                    and ops.causal_attention_supported(q, k):
                o = ops.causal_attention(q, k, v, key_valid)
            else:
                if key_valid is not None:
                    attn_mask = attn_mask.dense()
                o = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, is_causal=attn_mask is None,
                                                   enable_gqa=self.nkv != self.nh)
            return _lin(self.o_proj, o.transpose(1, 2).reshape(B, S, self.nh * self.hd))
        q = ops.rope(self.q_proj(x).view(B * S, self.nh, self.hd), cos, sin).view(B, S, self.nh, self.hd).transpose(1, 2)
        k = ops.rope(self.k_proj(x).view(B * S, self.nkv, self.hd), cos, sin).view(B, S, self.nkv, self.hd).transpose(1, 2)
        v = self.v_proj(x).view(B, S, self.nkv, self.hd).transpose(1, 2)
        if kv_out is not None:
            kv_out.append((k, v))
        key_valid = attn_mask.key_valid if isinstance(attn_mask, KeyPadding) else None
        if x.is_cuda and (attn_mask is None or key_valid is not None) and torch.is_grad_enabled() and q.requires_grad \
                and ops.causal_attention_supported(q, k):     # trainable projections (finetune stage): same HIP attention
            o = ops.causal_attention(q, k, v, key_valid)
            return self.o_proj(o.transpose(1, 2).reshape(B, S, self.nh * self.hd))
        if key_valid is not None:
            attn_mask = attn_mask.dense()
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, is_causal=attn_mask is None,
                                           enable_gqa=self.nkv != self.nh)
        return self.o_proj(o.transpose(1, 2).reshape(B, S, self.nh * self.hd))

    def decode(self, x, cos, sin, kcache, vcache, t: int, key_mask):
        """One new token per sequence against the cache (decode steps never see the SVA hook: cambrian_llama.py:174,
        ``prepare_inputs`` early-outs for length-1 inputs).  x [B,1,H]; k/v caches [B,nkv,Lmax,hd], slot t is filled here;
        key_mask bool [B, >= t+1] (columns past t are ignored).  On the GPU the whole step between the projections and
        o_proj is one ``ops.decode_attention`` call (decode_attn.hip); geometries it does not take, and
        ``CAMBRIAN_AMD_DECODE_ATTN=0``, run the stock SDPA body below."""
        B = x.shape[0]
        if use_decode_kernel(x, self.nh, self.nkv, self.hd):
            nq, nk = self.nh * self.hd, self.nkv * self.hd
            w_qkv = _fused_frozen_weight(self, "_w_qkv", (self.q_proj, self.k_proj, self.v_proj))
            if w_qkv is not None:
                row = F.linear(x.reshape(B, -1), w_qkv)                       # q heads | k heads | v heads per token
                q, k, v = row[:, :nq], row[:, nq:nq + nk], row[:, nq + nk:]
            else:
                x2 = x.reshape(B, -1)
                q, k, v = self.q_proj(x2), self.k_proj(x2), self.v_proj(x2)
            o = ops.decode_attention_any(q, k, v, cos, sin, kcache, vcache, t, key_mask)
            return self.o_proj(o.view(B, 1, nq))
        key_mask = key_mask[:, :t + 1]
        q = ops.rope(self.q_proj(x).view(B, self.nh, self.hd), cos, sin).view(B, 1, self.nh, self.hd).transpose(1, 2)
        k = ops.rope(self.k_proj(x).view(B, self.nkv, self.hd), cos, sin)
        kcache[:, :, t] = k
        vcache[:, :, t] = self.v_proj(x).view(B, self.nkv, self.hd)
        o = F.scaled_dot_product_attention(q, kcache[:, :, :t + 1], vcache[:, :, :t + 1], attn_mask=key_mask[:, None, None, :],
                                           enable_gqa=self.nkv != self.nh)
        return self.o_proj(o.transpose(1, 2).reshape(B, 1, self.nh * self.hd))

    def decode_multi(self, x, cos, sin, kcache, vcache, t0: int, key_mask):
        """Q consecutive tokens of ONE sequence against its cache, the plain torch body: x [Q,1,H]; cos / sin [Q, hd/2] at the
        tokens' positions; caches [1,nkv,Lmax,hd], slots t0 .. t0+Q-1 are filled here; token j attends under ``lookup_mask``.
        (The kernel form is the layer's: ``decode_layer_fused_multi``.)"""
        Q = x.shape[0]
        q = ops.rope(self.q_proj(x).view(Q, self.nh, self.hd), cos, sin)
        k = ops.rope(self.k_proj(x).view(Q, self.nkv, self.hd), cos, sin)
        kcache[0, :, t0:t0 + Q] = k.transpose(0, 1)
        vcache[0, :, t0:t0 + Q] = self.v_proj(x).view(Q, self.nkv, self.hd).transpose(0, 1)
        o = F.scaled_dot_product_attention(q.transpose(0, 1)[None], kcache[:, :, :t0 + Q], vcache[:, :, :t0 + Q],
                                           attn_mask=lookup_mask(key_mask, t0, Q)[None, None], enable_gqa=self.nkv != self.nh)
        return self.o_proj(o[0].transpose(0, 1).reshape(Q, 1, self.nh * self.hd))

    def extend(self, x, cos, sin, kcache, vcache, t0: int, key_mask):
        """A chunk of Q consecutive new tokens per sequence against the cache (the suffix of a prompt over a cached prefix):
        x [B,Q,H]; cos / sin [B*Q, hd/2] at the tokens' positions; caches [B,nkv,Lmax,hd], slots t0 .. t0+Q-1 are filled here;
        token j attends under ``ops.extend_mask`` (key_mask bool [B, >= t0+Q], read through column t0+Q-1).  On the GPU in
        bf16 everything between the projections and o_proj is one ``ops.extend_attention`` call (extend_attn.hip); fp32, other
        geometries and ``CAMBRIAN_AMD_DECODE_ATTN=0`` run the plain torch body below."""
        B, Q, _ = x.shape
        if use_extend_kernel(x, self.nh, self.nkv, self.hd, Q):
            nq, nk = self.nh * self.hd, self.nkv * self.hd
            w_qkv = _fused_frozen_weight(self, "_w_qkv", (self.q_proj, self.k_proj, self.v_proj))
            x2 = x.reshape(B * Q, -1)
            if w_qkv is not None:
                row = frozen_linear(self, "_w_qkv_t", x2, w_qkv)             # q heads | k heads | v heads per token
                q, k, v = row[:, :nq], row[:, nq:nq + nk], row[:, nq + nk:]
            else:
                q, k, v = self.q_proj(x2), self.k_proj(x2), self.v_proj(x2)
            o = ops.extend_attention(q, k, v, cos, sin, kcache, vcache, t0, key_mask)
            return _lin(self.o_proj, o.view(B, Q, nq))
        q = ops.rope(self.q_proj(x).view(B * Q, self.nh, self.hd), cos, sin).view(B, Q, self.nh, self.hd).transpose(1, 2)
        k = ops.rope(self.k_proj(x).view(B * Q, self.nkv, self.hd), cos, sin).view(B, Q, self.nkv, self.hd).transpose(1, 2)
        kcache[:, :, t0:t0 + Q] = k
        vcache[:, :, t0:t0 + Q] = self.v_proj(x).view(B, Q, self.nkv, self.hd).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, kcache[:, :, :t0 + Q], vcache[:, :, :t0 + Q],
                                           attn_mask=ops.extend_mask(key_mask, t0, Q)[:, None], enable_gqa=self.nkv != self.nh)
        return self.o_proj(o.transpose(1, 2).reshape(B, Q, self.nh * self.hd))


class LlamaDecoderLayer(nn.Module):
    def __init__(self, cfg, device, dtype):
        super().__init__()
        self.__dict__["_decode_cfg"] = cfg                 # decode_wide_rows reads config.decode_linear_wide when a step runs
        self.self_attn = LlamaAttention(cfg, device, dtype)
        self.mlp = LlamaMLP(cfg, device, dtype)
        self.input_layernorm = HipRMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device, dtype)
        self.post_attention_layernorm = HipRMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device, dtype)

    def forward(self, x, cos, sin, attn_mask, kv_out: Optional[list] = None):
        n1 = self.input_layernorm
        x, xn = ops.rmsnorm_fork(x, n1.weight, n1.variance_epsilon)   # (skip path, attention input): one backward node
        a = self.self_attn(xn, cos, sin, attn_mask, kv_out)
        n2 = self.post_attention_layernorm
        x, h = ops.add_rmsnorm(x, a, n2.weight, n2.variance_epsilon)  # x + a and norm(x + a) in one pass
        return self.mlp(h, residual=x)

    def extend(self, x, cos, sin, kcache, vcache, t0: int, key_mask):
        """``forward`` for a chunk x [B,Q,H] of new tokens against the cache (``self_attn.extend``): the same norms, MLP and
        frozen-linear route — GEMM-sized rows, so the weight-streaming decode linears and their reduced formats play no part."""
        n1 = self.input_layernorm
        x, xn = ops.rmsnorm_fork(x, n1.weight, n1.variance_epsilon)
        a = self.self_attn.extend(xn, cos, sin, kcache, vcache, t0, key_mask)
        n2 = self.post_attention_layernorm
        x, h = ops.add_rmsnorm(x, a, n2.weight, n2.variance_epsilon)
        return self.mlp(h, residual=x)

    def decode_entries(self, fmt=None):
        """(the four weights of a five-launch step, None where a projection is trainable or biased; with ``fmt`` their (owner,
        key, weight, act) entries for ``_decode_quant_copies``, else None).  The packed ones are _fused_frozen_weight's."""
        a, mlp = self.self_attn, self.mlp
        w = (_fused_frozen_weight(a, "_w_qkv", (a.q_proj, a.k_proj, a.v_proj)),
             a.o_proj.weight if _frozen_plain(a.o_proj) else None,
             _fused_frozen_weight(mlp, "_w_gate_up", (mlp.gate_proj, mlp.up_proj)),
             mlp.down_proj.weight if _frozen_plain(mlp.down_proj) else None)
        if fmt is None:
            return w, None
        return w, ((a, "_w_qkv_" + fmt, w[0], None), (a.o_proj, "_w_" + fmt, w[1], None),
                   (mlp, "_w_gate_up_" + fmt, w[2], "swiglu"), (mlp.down_proj, "_w_" + fmt, w[3], None))

    def decode_operands(self, x, fp8=False, fp4=False):
        """(the four weights, their e4m3 — ``fp4``: MXFP4 — copies or None) when ``decode`` runs a step of x [B, 1, H] as five
        launches, else None: ``decode_step_operands``, the condition ``decode`` runs on, for ``DecodeStepPlan``."""
        found = decode_step_operands(self, x, fp8, fp4)
        return None if found is None else found[:2]

    def decode(self, x, cos, sin, kcache, vcache, t, key_mask, fp8=False, fp4=False):
        """``fp8``: stream e4m3 copies of the weights where the five-launch step is taken (``ops.decode_fp8_enabled``,
        resolved once by ``generate``).  ``fp4``: MXFP4 copies instead (``ops.decode_fp4_enabled``); ``generate`` never sets
        both (``ops.decode_weight_format``), and ``fp4`` wins here if a caller does.  At 17-64 rows with the wide switch on
        (``decode_wide_rows``) the five launches run on ``ops.decode_linear_wide`` and the bf16 weights."""
        found = decode_step_operands(self, x, fp8, fp4)
        if found is None:
            x = x + self.self_attn.decode(self.input_layernorm(x), cos, sin, kcache, vcache, t, key_mask)
            return x + self.mlp(self.post_attention_layernorm(x))
        w, quant, wide = found
        return _five_launches(self, x, w, quant, fp4, ops.decode_linear_wide if wide else None, ops.decode_attention_any,
                              cos, sin, kcache, vcache, t, key_mask)

    def decode_multi(self, x, cos, sin, kcache, vcache, t0, key_mask, fp8=False, fp4=False):
        """``decode`` for Q consecutive tokens of ONE sequence, x [Q, 1, H] (the verify step of prompt-lookup decoding): five
        launches around ``ops.decode_attention_multi`` where ``decode`` itself would take five launches for Q rows, else the
        modules' own projections and SDPA."""
        out = decode_multi_fused_or_none(self, x, cos, sin, kcache, vcache, t0, key_mask, fp8, fp4)
        if out is not None:
            return out
        x = x + self.self_attn.decode_multi(self.input_layernorm(x), cos, sin, kcache, vcache, t0, key_mask)
        return x + self.mlp(self.post_attention_layernorm(x))


class LlamaBackbone(nn.Module):
    """HF ``LlamaModel`` parameter layout (embed_tokens / layers / norm), minimal forward.  ``layer_class`` is the
    decoder block; cambrian_phi3.py swaps in the Phi-3 block (packed qkv_proj / gate_up_proj parameters)."""
    layer_class = None  # set below, once LlamaDecoderLayer's own class statement has run

    def __init__(self, config, device=None, llm_dtype=torch.bfloat16):
        super().__init__()
        self.config = config
        self.llm_dtype = llm_dtype
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size, device=device, dtype=llm_dtype)
        block = type(self).layer_class or LlamaDecoderLayer
        self.layers = nn.ModuleList([block(config, device, llm_dtype) for _ in range(config.num_hidden_layers)])
        self.norm = HipRMSNorm(config.hidden_size, config.rms_norm_eps, device, llm_dtype)

    @property
    def dtype(self):
        """dtype for NEW trainable parameters (vision_query, image_newline): fp32 masters, as in the reference
        run where parameters are fp32 and only the compute is bf16 (fsdp_config.json:6, train_fsdp.py:1267-1398)."""
        return torch.float32


class CambrianLlamaModel(CambrianMetaModel, LlamaBackbone):
    config_class = CambrianConfig

    def __init__(self, config, device=None, llm_dtype=torch.bfloat16):
        # CambrianMetaModel.__init__ -> super().__init__(config) -> LlamaBackbone.__init__(config)
        self._ctor_kw = (device, llm_dtype)
        LlamaBackbone.__init__(self, config, device, llm_dtype)
        if hasattr(config, "mm_vision_tower_aux_list"):
            # re-run the mixin's config-driven construction on the already initialised backbone
            _BackboneShim.attach(self, config)

    def forward(self, inputs_embeds: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, sva=None, kv_out: Optional[list] = None) -> torch.Tensor:
        cfg = self.config
        B, S, H = inputs_embeds.shape
        dev = inputs_embeds.device
        if position_ids is None:
            position_ids = torch.arange(S, device=dev).unsqueeze(0).expand(B, S)
        hd = self.layers[0].self_attn.hd
        cos, sin = ops.rope_table(position_ids, hd, float(getattr(cfg, "rope_theta", 10000.0)))
        attn_mask = None
        window = getattr(cfg, "sliding_window", None)
        if window is not None and S <= window + 1:
            window = None                      # every key is within reach: plain causal attention
        if attention_mask is not None and window is None:
            attn_mask = KeyPadding(attention_mask)
        elif attention_mask is not None or window is not None:
            causal = torch.ones(S, S, dtype=torch.bool, device=dev).tril_()
            if window is not None:             # Phi-3 eager mask (phi3/modeling_phi3.py:1180-1186): 0 <= i - j <= window
                causal = causal & ~torch.ones(S, S, dtype=torch.bool, device=dev).tril_(-(window + 1))
            attn_mask = causal[None, None]
            if attention_mask is not None:
                attn_mask = attn_mask & attention_mask.to(torch.bool)[:, None, None, :]
                # a fully masked query row would be NaN in SDPA; padded rows attend to themselves (their loss is ignored)
                attn_mask = attn_mask | torch.eye(S, dtype=torch.bool, device=dev)[None, None]
        hidden = inputs_embeds
        hook_layers = {}
        if sva is not None and not getattr(cfg, "connector_only", True):
            start, stride = cfg.start_of_vision_sampler_layers, cfg.stride_of_vision_sampler_layers
            hook_layers = {start + k * stride: k for k in range(len(self.vision_sampler_layers))}  # :170-172
        # Activation re-computation (the reference: `--gradient_checkpointing True` in the finetune scripts,
        # scripts/cambrian/finetune_cambrian_8b.sh; FSDP wraps and checkpoints every decoder layer, fsdp_config.json:9, and
        # cambrian_llama.py:189-196 checkpoints the in-LLM SVA layers): a layer keeps only its input, its forward runs a second
        # time inside the backward.  Non-reentrant, so the custom autograd operators' saved tensors are the recomputed ones.
        ckpt = bool(getattr(cfg, "gradient_checkpointing", False)) and torch.is_grad_enabled() and kv_out is None
        for i, layer in enumerate(self.layers):
            if ckpt and hidden.requires_grad:
                hidden = _checkpoint(layer, hidden, cos, sin, attn_mask, None, use_reentrant=False)
            else:
                hidden = layer(hidden, cos, sin, attn_mask, kv_out)
            if i in hook_layers:
                if isinstance(sva, SvaDynamic):
                    hidden = self._sva_hook_dynamic(hidden, hook_layers[i], sva)
                else:
                    hidden = self._sva_hook(hidden, hook_layers[i], sva)
        return self.norm(hidden)

    def _sva_hook_dynamic(self, hidden: torch.Tensor, k: int, sva: "SvaDynamic") -> torch.Tensor:
        """cambrian_llama.py:209-253 (eval branch): every sample has its own cur_h x (cur_w + 1) block of latent
        queries + newline column starting at ``image_position``; the queries of all samples go through the sampler layer
        as one [sum h*w, 1, H] batch (KV lists / masks / context rows were concatenated the same way by
        rearrange_vision_tower_features_inference(unpad=True)) and are written back; newline rows stay."""
        p0 = self.config.image_position
        rows, nums = [], []
        for b, (h, w) in enumerate(sva.final_size):
            blk = hidden[b, p0:p0 + h * (w + 1)].view(h, w + 1, -1)
            rows.append(blk[:, :w].reshape(h * w, 1, -1))
            nums.append(h * w)
        q = torch.cat(rows, 0)
        feats = [f if f.dtype == q.dtype else f.to(q.dtype) for f in sva.feats]      # :186 (same cast in both branches)
        out = self.vision_sampler_layers[k](q, sva.ctx.to(q.dtype), *feats, *sva.masks)
        hidden = hidden.clone()
        for b, ob in enumerate(torch.split(out, nums, 0)):
            h, w = sva.final_size[b]
            hidden[b, p0:p0 + h * (w + 1)].view(h, w + 1, -1)[:, :w] = ob.view(h, w, -1)
        return hidden

    def _sva_hook(self, hidden: torch.Tensor, k: int, sva: SvaContext) -> torch.Tensor:
        """cambrian_llama.py:177-207 (static branch)."""
        cfg = self.config
        p0 = cfg.image_position
        side = int(cfg.image_token_len ** 0.5)
        hidden = hidden if hidden.is_contiguous() else hidden.contiguous()
        span = ops.region_begin("sva_in_llm")                                          # (bench.py roofline.region)
        link = None if os.environ.get("CAMBRIAN_AMD_NO_HOOK_LINK") else {}             # gather / scatter share d(hidden)
        q2 = ops.gather_query_rows(hidden, p0, side, link)                             # [B*576, H]
        q2 = ops.region_mark(q2, span, "b1")
        feats = [f if f.dtype == q2.dtype else f.to(q2.dtype) for f in sva.feats]      # :186
        sampler = self.vision_sampler_layers[k]
        if bool(getattr(cfg, "gradient_checkpointing", False)) and torch.is_grad_enabled() and q2.requires_grad:
            out = _checkpoint(sampler.forward_fused, q2, sva.ctx_b.to(q2.dtype), feats, sva.masks_u8, sva.holders, sva.B, side,
                              use_reentrant=False)                                     # cambrian_llama.py:189-196
        else:
            out = sampler.forward_fused(q2, sva.ctx_b.to(q2.dtype), feats, sva.masks_u8, sva.holders, sva.B, side)
        out = ops.region_mark(out, span, "b0")
        hidden = ops.scatter_query_rows(hidden, out, p0, side, link)
        ops.region_fwd_end(span)
        return hidden


class _BackboneShim:
    """CambrianMetaModel.__init__ calls ``super().__init__(config)`` (it is written as a mixin placed before the HF
    model class).  Our backbone is already constructed when we need the mixin's body, so run that body with a
    no-op super().__init__."""

    @staticmethod
    def attach(model: "CambrianLlamaModel", config):
        from ..cambrian_arch import _sva_modules, build_vision_projector, build_vision_tower_aux_list
        projector_type = getattr(config, "mm_projector_type", "linear")
        model.vision_tower_aux_list = build_vision_tower_aux_list(config, delay_load=True)
        if projector_type == "sva":
            _sva_modules(model, config, model.vision_tower_aux_list, config.hidden_size)
            model.vision_query = nn.Parameter(torch.randn((config.num_query_group, config.vision_hidden_size), dtype=model.dtype))
        else:
            config.mm_hidden_size = sum(t.hidden_size for t in model.vision_tower_aux_list)
            model.mm_projector = build_vision_projector(config)
        model.image_newline = nn.Parameter(torch.empty(config.hidden_size, dtype=model.dtype))


class CambrianLlamaForCausalLM(nn.Module, CambrianMetaForCausalLM):
    config_class = CambrianConfig
    model_class = CambrianLlamaModel

    def __init__(self, config, device=None, llm_dtype=torch.bfloat16):
        super().__init__()
        self.config = config
        self.model = type(self).model_class(config, device, llm_dtype)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False, device=device, dtype=llm_dtype)

    def get_model(self):
        return self.model

    @property
    def device(self):
        return self.lm_head.weight.device

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def get_output_embeddings(self):
        return self.lm_head

    def resize_token_embeddings(self, new_num_tokens: int):
        """HF ``PreTrainedModel.resize_token_embeddings`` for the two vocabulary-sized matrices (``load_pretrained_model``
        calls it after adding the image tokens, model/builder.py:158): old rows kept, new rows ~ N(0, initializer_range)."""
        old = self.model.embed_tokens.weight
        n_old, H = old.shape
        if new_num_tokens == n_old:
            return self.model.embed_tokens
        std = float(getattr(self.config, "initializer_range", 0.02))

        def grown(w):
            out = torch.empty((new_num_tokens, H), dtype=w.dtype, device=w.device).normal_(0.0, std)
            n = min(n_old, new_num_tokens)
            out[:n] = w.detach()[:n]
            return out

        emb = nn.Embedding(new_num_tokens, H, device=old.device, dtype=old.dtype)
        emb.weight = nn.Parameter(grown(old), requires_grad=old.requires_grad)
        self.model.embed_tokens = emb
        head = nn.Linear(H, new_num_tokens, bias=False, device=old.device, dtype=self.lm_head.weight.dtype)
        head.weight = nn.Parameter(grown(self.lm_head.weight), requires_grad=self.lm_head.weight.requires_grad)
        self.lm_head = head
        self.vocab_size = self.config.vocab_size = new_num_tokens
        return self.model.embed_tokens

    def forward(self, *args, **kwargs):
        """``config.fp8_projections`` (BASELINE configs[4]): the forward GEMMs of the SVA-side projections — aux
        projectors, connector and in-LLM SVA layers, mm_projector, i.e. everything that goes through ``ops.linear`` —
        run on the fp8 MFMA with row-wise e4m3 scaling; towers and decoder are untouched, the backward stays bf16."""
        try:
            with ops.fp8_projections(bool(getattr(self.config, "fp8_projections", False))):
                return self._forward(*args, **kwargs)
        finally:
            ops.weight_step_end()   # (the window prepare_inputs_labels_for_multimodal opened for this forward's linears)

    def _forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                 labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                 image_aux_attention_masks_list=None, image_sizes=None, return_dict=None, cache_position=None):
        sva = _masks = _final_size = _ctx = None
        if inputs_embeds is None:  # cambrian_llama.py:315-336
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels, sva, _masks, _final_size,
             _ctx) = self.prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                               labels, images, image_aux_attention_masks_list, image_sizes)
            if inputs_embeds is None:  # text-only early-out (cambrian_arch.py:346-347)
                inputs_embeds = self.model.embed_tokens(input_ids)
        if isinstance(sva, (list, tuple)):
            # reference-format lists (eval branch, or sva_fused = False): window-major KV, bool masks, per-sample (h, w),
            # one context row per query — consumed by the general per-sample hook (cambrian_llama.py:209-253)
            sva = SvaDynamic(sva, _masks, _final_size, _ctx)
        hidden = self.model(inputs_embeds.to(self.model.llm_dtype), position_ids, attention_mask, sva)
        if labels is not None and getattr(self.config, "fused_loss", False) == "scored_rows":
            # Opt-in (round 5, ``config.fused_loss = "scored_rows"``): lm_head and the cross-entropy only over the positions that
            # are scored — shifted label != IGNORE_INDEX; the collator masks the 600 visual slots, the prompt and the padding
            # (train_fsdp.py:1089-1165), a third of the synthetic batch and more of a real one.  Ignored rows contribute nothing to
            # the loss and receive a zero gradient, so loss and every gradient are those of the full computation
            # (tests/test_model_gpu.py::test_scored_rows_loss_equals_the_full_one); what changes is that ``logits`` is not
            # produced (None) — the reference's training_step reads ``loss`` only (cambrian_trainer.py:226-236).  Labels handed
            # over on the CPU (as the collator makes them) give the row list without a device synchronisation.
            Bq_, Sq_, Hd_ = hidden.shape
            shift_labels = torch.full_like(labels, IGNORE_INDEX)
            shift_labels[:, :-1] = labels[:, 1:]
            flat = shift_labels.reshape(-1)
            idx = torch.nonzero(flat != IGNORE_INDEX).squeeze(1)
            if idx.numel() > 0:
                sel = flat[idx].to(hidden.device, non_blocking=True)
                h_sel = hidden.reshape(Bq_ * Sq_, Hd_).index_select(0, idx.to(hidden.device, non_blocking=True))
                loss = ops.cross_entropy(_lin(self.lm_head, h_sel), sel, IGNORE_INDEX, inplace=True)
                if CausalLMOutputWithPast is not None:
                    return CausalLMOutputWithPast(loss=loss, logits=None)
                return {"loss": loss, "logits": None}
        logits = _lin(self.lm_head, hidden)                                          # :402-408
        loss = None
        if labels is not None and getattr(self.config, "fused_loss", False):
            # :409-422 without logits.float() / the shifted copy: labels are shifted instead of the logits (position
            # t is scored against labels[t+1], the last position of every sequence is ignored), fp32 log-sum-exp over
            # the bf16 logits in one pass, dlogits written in place of the logits in the backward.  ``logits`` is then
            # returned in the compute dtype (its .float() is the reference's tensor) and is consumed by backward().
            B_, S_, V_ = logits.shape
            shift_labels = torch.full_like(labels, IGNORE_INDEX)
            shift_labels[:, :-1] = labels[:, 1:]
            loss = ops.cross_entropy(logits.view(B_ * S_, V_), shift_labels.view(-1).to(logits.device), IGNORE_INDEX,
                                     inplace=True)
        else:
            logits = logits.float()                                                  # :409
            if labels is not None:                                                   # :411-422
                shift_logits = logits[..., :-1, :].contiguous().view(-1, self.vocab_size)
                shift_labels = labels[..., 1:].contiguous().view(-1).to(shift_logits.device)
                loss = F.cross_entropy(shift_logits, shift_labels, ignore_index=IGNORE_INDEX)
        if CausalLMOutputWithPast is not None:
            return CausalLMOutputWithPast(loss=loss, logits=logits)
        return {"loss": loss, "logits": logits}


# generate() keyword arguments that change nothing here: the K/V cache is always on, padding / bos ids are not needed by a
# loop that returns only the new tokens, and the listed output switches are accepted at their "off" value only
_GENERATE_ACCEPTED_NOOPS = {"use_cache": (True, None), "pad_token_id": None, "bos_token_id": None, "output_scores": (False, None),
                            "return_dict_in_generate": (False, None), "output_attentions": (False, None),
                            "output_hidden_states": (False, None), "num_return_sequences": (1, None),
                            "repetition_penalty": (1.0, None), "length_penalty": (1.0, None), "early_stopping": (False, None),
                            "stopping_criteria": (None,), "logits_processor": (None,), "streamer": (None,)}


def filter_logits_top_k_top_p(logits: torch.Tensor, top_k=None, top_p=None) -> torch.Tensor:
    """HF's TopKLogitsWarper then TopPLogitsWarper (the order GenerationMixin applies them in, after the temperature), on
    fp32 logits [B, V]: tokens outside the k largest, then tokens outside the smallest set whose probability mass reaches
    ``top_p`` (ascending sort, drop while the cumulative mass <= 1 - top_p, always keep the most probable), are set to -inf."""
    if top_k is not None and int(top_k) > 0:
        k = min(int(top_k), logits.shape[-1])
        kth = torch.topk(logits, k, dim=-1).values[..., -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p is not None and float(top_p) < 1.0:
        if not 0.0 < float(top_p):
            raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
        srt, idx = torch.sort(logits, descending=False, dim=-1)
        cum = srt.softmax(-1).cumsum(-1)
        drop = cum <= (1.0 - float(top_p))
        drop[..., -1:] = False
        logits = logits.masked_fill(torch.zeros_like(drop).scatter(-1, idx, drop), float("-inf"))
    return logits


def _decode_logits_found(self, x: torch.Tensor, fp8: bool, fp4: bool):
    """(lm_head weight, its e4m3 — with ``fp4`` its MXFP4 — copy or None, wide) when a decode step's logits are one launch,
    else None: the one condition ``_decode_logits`` and ``DecodeStepPlan`` share.  A refused MXFP4 head falls back to bf16,
    not to e4m3; at wide rows (``decode_wide_rows``) no copy is made."""
    model, head = self.model, self.lm_head
    a = model.layers[0].self_attn if len(model.layers) else None        # a decoder without layers keeps the stock line
    B = x.shape[0]
    wide = decode_wide_rows(self, B)
    if a is not None and use_decode_kernel(x, a.nh, a.nkv, a.hd) and x.dtype == torch.bfloat16 \
            and (wide or (B <= ops.DECODE_LINEAR_MAX_ROWS and ops.decode_linear_enabled(B))) \
            and _frozen_plain(head) and not model.norm.weight.requires_grad and model.norm.weight.dtype == torch.bfloat16 \
            and (ops.decode_linear_wide_supported if wide else ops.decode_linear_supported)(x[:, 0], head.weight):
        fmt = None if wide else ("fp4" if fp4 else ("fp8" if fp8 else None))
        quant = None if fmt is None else _decode_quant_copies(fmt, head, B, ((head, "_w_" + fmt, head.weight, None),))
        return head.weight, (None if quant is None else quant[0]), wide
    return None


def _decode_logits_operands(self, x: torch.Tensor, fp8: bool = False, fp4: bool = False):
    """(lm_head weight, its quantised copy or None) when ``_decode_logits`` takes its one-launch arm, else None."""
    found = _decode_logits_found(self, x, fp8, fp4)
    return None if found is None else found[:2]


def _decode_logits(self, x: torch.Tensor, fp8: bool = False, fp4: bool = False) -> torch.Tensor:
    """fp32 logits of a decode step from the last layer's x [B, 1, H]: final norm + lm_head in one ``ops.decode_linear``
    launch under the conditions of the layers' five-launch step, else the norm kernel, the stock GEMM and a cast.
    ``fp8``: that launch streams the lm_head's e4m3 copy (``ops.decode_linear_fp8``) where the kernel takes it; ``fp4``: its
    MXFP4 copy (``ops.decode_linear_fp4``).  At 17-64 rows with the wide switch on (``decode_wide_rows``) the one launch is
    ``ops.decode_linear_wide`` on the bf16 lm_head, whatever ``fp8`` / ``fp4`` say."""
    norm = self.model.norm
    found = _decode_logits_found(self, x, fp8, fp4)
    if found is None:
        return self.lm_head(norm(x)[:, 0]).float()
    w, quant, wide = found
    if quant is None:
        lin, mat = (ops.decode_linear_wide if wide else ops.decode_linear), (w,)
    else:
        lin, mat = (ops.decode_linear_fp4 if fp4 else ops.decode_linear_fp8), quant
    return lin(x[:, 0], *mat, norm_weight=norm.weight, eps=norm.variance_epsilon, out_dtype=torch.float32)


class DecodeStepPlan:
    """What the decode steps of ONE ``generate()`` call share when they are issued as one library call per token
    (``ops.decode_step``): the layer table and the step descriptor in host memory, the objects that own every pointer in
    them, the workspace and the logits buffer.  ``build`` returns None unless the whole model qualifies — every layer under
    the five-launch conditions, the lm_head under ``_decode_logits``' condition, with ``fp8`` the e4m3 copies (with ``fp4`` the
    MXFP4 copies, ``cmb_decode_step_desc.fp8`` = 2) of every weight — and the call then runs on the per-launch loop, unchanged.
    ``caches``: per layer (k, v), bf16 tensors or ``ops.KvCacheE4M3`` pairs (the step is then ``cmb_decode_step_kv8``)."""

    @classmethod
    def build(cls, lm, B: int, caches, t_max: int, fp8: bool, fp4: bool = False):
        model = lm.model
        if not len(model.layers) or len(caches) != len(model.layers) or not 1 <= B <= ops.DECODE_LINEAR_MAX_ROWS:
            return None
        dev = lm.lm_head.weight.device
        if model.llm_dtype != torch.bfloat16 or dev.type != "cuda":
            return None
        cfg = lm.config
        a0 = model.layers[0].self_attn
        H, nh, nkv, hd = cfg.hidden_size, a0.nh, a0.nkv, a0.hd
        x = torch.empty(B, 1, H, dtype=torch.bfloat16, device=dev)       # what the predicates look at; never read
        quant = bool(fp8 or fp4)
        head = _decode_logits_operands(lm, x, fp8, fp4)
        if head is None or (quant and head[1] is None):
            return None
        eps = float(model.norm.variance_epsilon)
        kv8 = isinstance(caches[0][0], ops.KvCacheE4M3)          # e4m3 caches: byte tensors + factor arrays (cmb_decode_step_kv8)
        if kv8 and not ops.decode_attention_kv8_supported(torch.bfloat16, nh, nkv, hd):
            return None
        kc0 = caches[0][0].q if kv8 else caches[0][0]
        inv0 = caches[0][0].inv if kv8 else None
        keep, rows, inter, factors = [x, head, model.norm.weight, caches], [], None, []
        for layer, (kc, vc) in zip(model.layers, caches):
            a = layer.self_attn
            n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
            if not hasattr(layer, "decode_operands") or (a.nh, a.nkv, a.hd) != (nh, nkv, hd) \
                    or float(n1.variance_epsilon) != eps or float(n2.variance_epsilon) != eps:
                return None
            found = layer.decode_operands(x, fp8, fp4) if fp4 else layer.decode_operands(x, fp8)
            if found is None or (quant and found[1] is None):
                return None
            w, q8 = found
            if w[2].shape[0] % 2 or (inter is not None and w[2].shape[0] // 2 != inter) or w[0].shape != ((nh + 2 * nkv) * hd, H) \
                    or w[1].shape != (H, nh * hd) or w[3].shape != (H, w[2].shape[0] // 2) or w[2].shape[1] != H:
                return None
            inter = w[2].shape[0] // 2
            if kv8:
                if not (isinstance(kc, ops.KvCacheE4M3) and isinstance(vc, ops.KvCacheE4M3)) \
                        or any(c.inv.stride() != inv0.stride() for c in (kc, vc)):
                    return None
                factors.append(_lib.DecodeKv8Factors(kc.inv.data_ptr(), vc.inv.data_ptr()))
                kc, vc = kc.q, vc.q
            if kc.dtype != (torch.uint8 if kv8 else torch.bfloat16) or vc.dtype != kc.dtype or kc.shape != (B, nkv, kc0.shape[2], hd) \
                    or vc.shape != kc.shape or kc.stride() != kc0.stride() or vc.stride() != kc0.stride() or kc.stride(3) != 1:
                return None
            row = _lib.DecodeLayer()
            mats = q8 if quant else [(wi, None) for wi in w]
            if fp4 and any(sc.stride(0) != sc.shape[1] for _, sc in mats):      # the step takes scale rows K / 32 apart
                return None
            for name, (m, sc) in zip(("qkv", "o", "gate_up", "down"), mats):
                setattr(row, "w_" + name, m.data_ptr())
                setattr(row, "ld_" + name, m.stride(0))
                setattr(row, "w_" + name + "_scale", _lib.ptr(sc))
            row.norm1, row.norm2 = n1.weight.data_ptr(), n2.weight.data_ptr()
            row.kcache, row.vcache = kc.data_ptr(), vc.data_ptr()
            rows.append(row)
            keep.append((found, n1.weight, n2.weight))
        if t_max >= kc0.shape[2]:
            return None
        self = cls()
        hw, hs = head[1] if quant else (head[0], None)
        if fp4 and hs.stride(0) != hs.shape[1]:
            return None
        V = head[0].shape[0]
        self.desc = _lib.DecodeStepDesc(B=B, layers=len(rows), H=H, I=inter, nh=nh, nkv=nkv, hd=hd, fp8=2 if fp4 else int(bool(fp8)), V=V, eps=eps,
                                     scale=1.0 / math.sqrt(hd), c_sb=kc0.stride(0), c_sh=kc0.stride(1), c_st=kc0.stride(2),
                                     final_norm=model.norm.weight.data_ptr(), head=hw.data_ptr(), ld_head=hw.stride(0),
                                     head_scale=_lib.ptr(hs))
        self.table = (_lib.DecodeLayer * len(rows))(*rows)
        self.kv8 = ((_lib.DecodeKv8Factors * len(factors))(*factors), inv0.stride(0), inv0.stride(1)) if kv8 else None
        self.keep = keep
        self.ws = ops.decode_step_workspace(dev, ops.decode_step_ws_floats(B, H, inter, nh, nkv, hd, t_max))
        self.logits = torch.empty(B, (V + 7) // 8 * 8, dtype=torch.float32, device=dev)[:, :V]
        self.B, self.H, self.hd, self.t_max = B, H, hd, t_max
        return self

    def step(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, t: int, key_valid: torch.Tensor) -> torch.Tensor:
        """fp32 logits [B, V] (the plan's buffer, overwritten by the next step) of the token whose embeddings are x [B, H]."""
        return ops.decode_step(self.desc, self.table, x, cos, sin, t, key_valid, self.ws, self.logits, kv8=self.kv8)


def _generate(self, inputs=None, images=None, image_sizes=None, max_new_tokens: int = 16, do_sample: bool = False,
              temperature: float = 1.0, eos_token_id=None, attention_mask=None, position_ids=None, top_p=None, top_k=None,
              num_beams: int = 1, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, _draft_fn=None, prefix=None,
              **kwargs):
    """cambrian_llama.py:437-483: ``generate(input_ids, images=, image_sizes=)`` of the eval harness
    (eval/eval/*/…_eval.py, e.g. gqa_eval.py:108-117: do_sample / temperature / top_p / num_beams / max_new_tokens /
    use_cache).  Prefill = the eval branch of prepare_inputs_labels_for_multimodal + the decoder with the per-sample in-LLM
    SVA hook, K/V of every layer kept; decode steps = one token against the cache, no hook (cambrian_llama.py:174).
    Greedy, or sampling with temperature -> top-k -> nucleus top-p as HF's logits warpers define them; returns the NEW
    token ids [B, <= max_new_tokens] (like HF generate() called with inputs_embeds).  The reference inherits the loop from HF
    GenerationMixin; what this loop does not implement RAISES instead of being dropped: beam search (``num_beams > 1``) unless
    it is switched on (``config.decode_beam_search`` / CAMBRIAN_AMD_DECODE_BEAM=1: ``_beam_search``, HF's beam search without
    sampling, length penalty 1, no early stopping, one returned sequence), ``inputs_embeds`` (the reference raises too,
    cambrian_llama.py:447-448) and any keyword it does not know.
    ``prompt_lookup_num_tokens`` (1 .. 15; None / 0 = off) with ``max_matching_ngram_size`` (default 2): HF's prompt-lookup
    assisted decoding for greedy decoding of ONE prompt (``_lookup_loop``): drafts by n-gram lookup in the prompt and the
    output so far, verified in one multi-token step; the call leaves ``self.lookup_stats``.  ``_draft_fn`` (private) stands in
    for ``lookup.ngram_draft``.
    With the logits processors switched on (``config.decode_logits_processors`` / CAMBRIAN_AMD_DECODE_PROCESS=1):
    ``repetition_penalty``, ``no_repeat_ngram_size``, ``min_new_tokens``, ``bad_words_ids``, ``suppress_tokens`` as HF's
    processors define them over the GENERATED ids (``processors.py``; one ``ops.decode_process`` launch per token before the
    selection, on both loops), and ``eos_token_id`` may be a list: a row is done from its first id of the set and then emits
    ``eos[0]``.  They do not combine with beam search or prompt-lookup decoding (NotImplementedError); switched off, anything
    but their off values raises a ValueError that names the switch.
    ``prefix`` (a ``PrefixCache`` of ``prefill_prefix``): ``inputs`` [N, Q] are then N >= 1 suffixes of the ONE cached prompt
    head, left-padded under ``attention_mask``; the head's K / V is copied into every row's cache, one ``extend_step`` runs the
    suffixes against it and the loops below go on from slot P + Q.  Row n returns what ``generate(cat(prefix_ids, suffix_n),
    images=...)`` returns for that prompt alone (``_prefix_args`` has what is refused)."""
    _prefix_args(self, prefix, inputs, attention_mask, images, num_beams, prompt_lookup_num_tokens, position_ids, image_sizes)
    if "inputs_embeds" in kwargs:
        raise NotImplementedError("`inputs_embeds` is not supported")          # cambrian_llama.py:447-448
    beams = 1 if num_beams is None else int(num_beams)
    if beams > 1:
        if not ops.decode_beam_enabled(getattr(getattr(self, "config", None), "decode_beam_search", False)):
            raise NotImplementedError(f"generate(num_beams={num_beams}): beam search is not implemented in cambrian_amd "
                                      "(greedy / temperature / top-k / top-p sampling only); pass num_beams=1, or switch beam "
                                      "search on (config.decode_beam_search / CAMBRIAN_AMD_DECODE_BEAM=1)")
        if do_sample:
            raise NotImplementedError(f"generate(num_beams={num_beams}, do_sample=True): beam sampling is not implemented")
        if int(max_new_tokens) < 1:
            raise ValueError(f"generate(num_beams={num_beams}): max_new_tokens has to be >= 1, but is {max_new_tokens}")
    if "max_length" in kwargs and kwargs["max_length"] is not None:
        raise NotImplementedError("generate(max_length=...): use max_new_tokens")
    kwargs.pop("max_length", None)
    # the logits processors that read the generated ids, opt-in; switched off, repetition_penalty keeps the rule below
    proc_on = ops.decode_process_enabled(getattr(getattr(self, "config", None), "decode_logits_processors", False))
    proc_args = {k: kwargs.pop(k, None) for k in PROC.ARGUMENTS if k != "repetition_penalty" or proc_on}
    for k, v in kwargs.items():
        ok = _GENERATE_ACCEPTED_NOOPS.get(k, ())
        if k not in _GENERATE_ACCEPTED_NOOPS or (ok is not None and v not in ok):
            raise ValueError(f"generate(): unsupported argument {k}={v!r} (cambrian_amd implements greedy / temperature / "
                             "top_k / top_p decoding with a K/V cache)")
    lookup = _lookup_args(self, inputs, prompt_lookup_num_tokens, max_matching_ngram_size, do_sample, temperature, beams)
    spec = PROC.parse(proc_on, eos_token_id, beams=beams, lookup=lookup is not None, **proc_args)
    if proc_on and eos_token_id is not None:            # an int, a list of one id, or a set: eos[0] is what a done row emits
        eos_token_id = PROC.eos_list(eos_token_id)[0]
    prompt_ids, prompt_mask = inputs, attention_mask        # what the lookup drafts from (the multimodal prefill replaces both)
    with torch.no_grad():
        model = self.model
        nh_kv, hd = model.layers[0].self_attn.nkv, model.layers[0].self_attn.hd
        if prefix is not None:
            logits, caches, valid = _prefix_extend(self, prefix, inputs, attention_mask, int(max_new_tokens))
            (B, L), dev = valid.shape, valid.device
            Lmax = L + max_new_tokens
        else:
            hidden, kv_out, valid = _prefill(self, inputs, images, image_sizes, attention_mask, position_ids)
            (B, L), dev = valid.shape, valid.device
            last = valid.long().sum(1) - 1                                              # last real token of every row
            if not bool((valid[:, 1:] <= valid[:, :-1]).all()):
                last = torch.full_like(last, L - 1)                                      # left padding: the last column
            logits = self.lm_head(hidden[torch.arange(B, device=dev), last]).float()
            if beams > 1:
                return _beam_search(self, logits, kv_out, valid, L, int(max_new_tokens), eos_token_id,
                                    kwargs.get("pad_token_id"), beams, _kv8_wanted(self, dev, kv_out))
            Lmax = L + max_new_tokens
            # e4m3 K / V cache, opt-in: resolved once per call
            caches = (_kv8_prefill if _kv8_wanted(self, dev, kv_out) else _bf16_prefill)(kv_out, B, 1, nh_kv, L, Lmax, hd, dev)
        key_mask = torch.zeros(B, Lmax, dtype=torch.bool, device=dev)
        key_mask[:, :L] = valid
        n_tok = valid.long().sum(1)
        out_ids = []
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        theta = float(getattr(self.config, "rope_theta", 10000.0))
        fmt = ops.decode_weight_format(self.config)            # e4m3 or MXFP4 weight stream, opt-in; both on raises
        fp8, fp4 = fmt == "fp8", fmt == "fp4"
        if lookup is not None:
            return _lookup_loop(self, logits, caches, key_mask, n_tok, L, int(max_new_tokens), eos_token_id, prompt_ids,
                                prompt_mask, lookup, _draft_fn, fp8, fp4, hd, theta)
        plan = None                                                                       # one library call per token, opt-in
        if max_new_tokens > 1 and ops.decode_step_enabled(getattr(self.config, "decode_step_fused", False)):
            plan = DecodeStepPlan.build(self, B, caches, Lmax - 1, fp8, fp4)
        sampled = bool(do_sample and temperature > 0)
        proc = None if spec is None else ops.DecodeProcess(spec, dev)          # the lists go to the device once per call
        if plan is not None and (not sampled or ops.decode_sample_enabled(getattr(self.config, "decode_sample_device", False))):
            emb = model.embed_tokens.weight
            if _fused_embedding_ok(emb, logits.shape[1], eos_token_id):
                if sampled:
                    return _sample_fused(plan, emb, logits, key_mask, n_tok, L, max_new_tokens, eos_token_id, hd, theta,
                                         temperature, top_k, top_p, proc)
                return _greedy_fused(plan, emb, logits, key_mask, n_tok, L, max_new_tokens, eos_token_id, hd, theta, proc)
        if proc is not None:                     # the history the kernel reads, and the eos set a row is done on
            hist = torch.zeros(B, max_new_tokens, dtype=torch.int64, device=dev)
            eos_set = torch.tensor(spec.eos, dtype=torch.int64, device=dev)
        for step in range(max_new_tokens):
            if proc is not None:                 # processors first, warpers after: HF's order
                ops.decode_process(logits, hist, step, proc)
            if do_sample and temperature > 0:
                warped = filter_logits_top_k_top_p(logits / temperature, top_k, top_p)
                nxt = torch.multinomial(torch.softmax(warped, -1), 1)[:, 0]
            else:
                nxt = logits.argmax(-1)
            if eos_token_id is not None:
                nxt = torch.where(done, torch.full_like(nxt, eos_token_id), nxt)
                done = done | (nxt == eos_token_id if proc is None else torch.isin(nxt, eos_set))
            if proc is not None:
                hist[:, step] = nxt
            out_ids.append(nxt)
            if step + 1 == max_new_tokens or (eos_token_id is not None and bool(done.all())):
                break
            t = L + step
            key_mask[:, t] = True
            cos, sin = ops.rope_table((n_tok + step)[:, None], hd, theta)
            x = model.embed_tokens(nxt)[:, None, :].to(model.llm_dtype)
            if plan is not None:                 # sampling: torch's warpers above, the layers and the logits in one call
                logits = plan.step(x[:, 0], cos, sin, t, key_mask)
            else:
                logits = _decode_token(self, x, cos, sin, caches, t, key_mask, fp8, fp4)
        return torch.stack(out_ids, 1)


def _prefill(self, inputs, images, image_sizes, attention_mask, position_ids):
    """The prefill of ``generate`` and ``prefill_prefix``: the eval branch of prepare_inputs_labels_for_multimodal (with
    ``images``) and the decoder with the per-sample in-LLM SVA hook, K / V of every layer kept.  -> (hidden [B, L, H], kv_out:
    (k, v) [B, nkv, L, hd] per layer, valid bool [B, L]); L is the length after the image expansion.  Under no_grad."""
    model = self.model
    if images is not None:
        self._dynamic_path = True
        try:
            (_, position_ids, attention_mask, _, inputs_embeds, _, kv, masks, final_size, ctx) = \
                self.prepare_inputs_labels_for_multimodal(inputs, position_ids, attention_mask, None, None, images,
                                                          image_sizes=image_sizes)
        finally:
            self._dynamic_path = False
        sva = None if kv is None else SvaDynamic(kv, masks, final_size, ctx)
    else:
        inputs_embeds, sva = model.embed_tokens(inputs), None
    B, L, _ = inputs_embeds.shape
    dev = inputs_embeds.device
    valid = torch.ones(B, L, dtype=torch.bool, device=dev) if attention_mask is None else attention_mask.bool()
    pos = (valid.long().cumsum(1) - 1).clamp_min(0) if position_ids is None else position_ids
    kv_out: list = []
    hidden = model(inputs_embeds.to(model.llm_dtype), pos, attention_mask, sva, kv_out=kv_out)
    return hidden, kv_out, valid


class PrefixCache:
    """What ``prefill_prefix`` keeps of ONE prompt head, read-only: ``kv`` — every layer's (k, v) [1, nkv, P, hd] after RoPE;
    ``key_mask`` bool [1, P]; ``n_tok`` — its valid tokens (the position of the next one); ``last_hidden`` [1, H] — the final
    norm's row of the last valid token; ``P`` — the length AFTER the image expansion; and the model (a weak reference), dtype,
    device and (layers, nkv, hd) it was made with, for ``generate(prefix=...)``'s compatibility check.  ``generate`` copies
    from it and never writes it, so one cache serves any number of calls."""

    def __init__(self, owner, kv, key_mask, n_tok: int, last_hidden, dtype, device):
        self.owner = weakref.ref(owner)
        self.kv, self.key_mask, self.n_tok, self.last_hidden = kv, key_mask, int(n_tok), last_hidden
        self.P = int(key_mask.shape[1])
        self.dtype, self.device = dtype, device
        self.geometry = (len(kv),) + ((kv[0][0].shape[1], kv[0][0].shape[3]) if kv else (0, 0))


def prefill_prefix(self, inputs, images=None, image_sizes=None, attention_mask=None) -> PrefixCache:
    """The prefill of ONE prompt head (batch 1) — system text, ``<image>``, anything every question shares — kept as a
    ``PrefixCache`` for ``generate(suffix_ids, prefix=cache)``: exactly the prefill ``generate(inputs, images=...)`` runs
    (towers, connector SVA, the in-LLM hook, every layer's K / V).  Attention is causal and the hook rewrites only the image
    block's rows, so nothing in the head depends on what follows it."""
    if inputs is None or inputs.dim() != 2 or inputs.shape[0] != 1 or inputs.shape[1] < 1:
        raise ValueError("prefill_prefix: one prompt of at least one token, input ids [1, P]")
    with torch.no_grad():
        hidden, kv_out, valid = _prefill(self, inputs, images, image_sizes, attention_mask, None)
        n_tok = int(valid.long().sum())
        left_padded = not bool((valid[:, 1:] <= valid[:, :-1]).all())
        last = valid.shape[1] - 1 if left_padded else max(n_tok - 1, 0)
        return PrefixCache(self, [(k, v) for k, v in kv_out], valid, n_tok, hidden[:, last].clone(), self.model.llm_dtype,
                           hidden.device)


def _prefix_args(self, prefix, inputs, attention_mask, images, num_beams, lookup_tokens, position_ids=None,
                 image_sizes=None) -> None:
    """``generate(prefix=...)``'s refusals, all before the model is touched.  ValueError: no ``PrefixCache``, one of another
    model, dtype or device, ``images`` / ``image_sizes`` / ``position_ids`` beside it, no suffix token, an image token in a suffix, a suffix mask that is not
    left-padded.  NotImplementedError: beams, prompt lookup and the e4m3 K / V cache, which are not built on a prefix."""
    if prefix is None:
        return
    if not isinstance(prefix, PrefixCache):
        raise ValueError(f"generate(prefix=...): expected the PrefixCache of prefill_prefix, got {type(prefix).__name__}")
    if images is not None:
        raise ValueError("generate(prefix=..., images=...): images belong to the prefix (prefill_prefix(inputs, images=...)); a "
                         "suffix holds text only")
    if image_sizes is not None:
        raise ValueError("generate(prefix=..., image_sizes=...): image sizes belong to the prefix "
                         "(prefill_prefix(inputs, images=..., image_sizes=...))")
    if position_ids is not None:
        raise ValueError("generate(prefix=..., position_ids=...): suffix positions follow the prefix (its valid tokens + the "
                         "running count of the suffix mask); explicit position ids are not taken")
    if inputs is None or inputs.dim() != 2 or inputs.shape[0] < 1 or inputs.shape[1] < 1:
        raise ValueError("generate(prefix=...): suffix ids [N, Q] with N >= 1 and Q >= 1 (Q == 0: there is nothing to extend "
                         "the prefix with)")
    if bool((inputs == IMAGE_TOKEN_INDEX).any()):
        raise ValueError("generate(prefix=...): an image token in a suffix; images belong to the prefix")
    if attention_mask is not None:
        m = attention_mask.bool()
        if m.shape != inputs.shape or not bool(m[:, -1].all()) or not bool((m[:, 1:] >= m[:, :-1]).all()):
            raise ValueError("generate(prefix=...): the suffix mask has to be left-padded, [N, Q] with every row's valid tokens "
                             "right-aligned")
    layers = self.model.layers
    a0 = layers[0].self_attn if len(layers) else None
    if prefix.owner() is not self or prefix.dtype != self.model.llm_dtype or prefix.device != inputs.device \
            or prefix.geometry != (len(layers), getattr(a0, "nkv", 0), getattr(a0, "hd", 0)):
        raise ValueError("generate(prefix=...): the PrefixCache was made by another model, or in another dtype or on another "
                         "device than this call's")
    if num_beams is not None and int(num_beams) > 1:
        raise NotImplementedError(f"generate(prefix=..., num_beams={num_beams}): beam search over a cached prefix is not "
                                  "implemented (the caches would have to be spread over the beams)")
    if not (lookup_tokens is None or (not isinstance(lookup_tokens, bool) and lookup_tokens == 0)):
        raise NotImplementedError("generate(prefix=..., prompt_lookup_num_tokens=...): prompt-lookup decoding over a cached "
                                  "prefix is not implemented")
    if ops.decode_kv_fp8_enabled(getattr(getattr(self, "config", None), "decode_kv_fp8", False)):
        raise NotImplementedError("generate(prefix=...): the chunk step reads and writes bf16 K / V caches; switch the e4m3 K / V "
                                  "cache off (config.decode_kv_fp8 / CAMBRIAN_AMD_DECODE_KV_FP8)")


def extend_step(self, ids, caches, t0: int, pos, key_mask) -> torch.Tensor:
    """Final-norm hidden states [B, Q, H] of a chunk of Q new tokens ``ids`` [B, Q] per sequence against the caches:
    embeddings, the RoPE table at ``pos`` [B, Q], every layer's ``extend`` (K / V of token j into cache slot t0 + j, attention
    under ``ops.extend_mask`` of ``key_mask`` [B, >= t0 + Q]) and the final norm.  No SVA hook: a chunk holds no image tokens."""
    model = self.model
    hd = model.layers[0].self_attn.hd
    cos, sin = ops.rope_table(pos, hd, float(getattr(self.config, "rope_theta", 10000.0)))
    x = model.embed_tokens(ids).to(model.llm_dtype)
    for layer, (kc, vc) in zip(model.layers, caches):
        x = layer.extend(x, cos, sin, kc, vc, t0, key_mask)
    return model.norm(x)


def _prefix_extend(self, prefix: PrefixCache, ids, attention_mask, max_new_tokens: int):
    """The prefill of ``generate(prefix=...)``: every layer's cache of P + Q + max_new_tokens slots per suffix row with the
    prefix's columns copied in (``_bf16_prefill`` spreading one prompt over N rows; the ``PrefixCache`` is only read), then one
    ``extend_step`` over the N suffixes.  -> (fp32 logits [N, V] of the last column, caches, valid bool [N, P + Q])."""
    model = self.model
    N, Q = ids.shape
    P, dev = prefix.P, ids.device
    a0 = model.layers[0].self_attn
    caches = _bf16_prefill(prefix.kv, 1, N, a0.nkv, P, P + Q + max_new_tokens, a0.hd, dev)
    valid = torch.ones(N, P + Q, dtype=torch.bool, device=dev)
    valid[:, :P] = prefix.key_mask
    if attention_mask is not None:
        valid[:, P:] = attention_mask.bool()
    pos = (prefix.n_tok + valid[:, P:].long().cumsum(1) - 1).clamp_min(0)
    hidden = extend_step(self, ids, caches, P, pos, valid)
    return self.lm_head(hidden[:, -1]).float(), caches, valid


def _decode_token(self, x, cos, sin, caches, t: int, key_mask, fp8: bool, fp4: bool) -> torch.Tensor:
    """The per-launch decode step: x [B, 1, H] through every layer's ``decode`` (K / V into cache slot ``t``; the step reads
    columns 0..t of ``key_mask`` [B, Lmax]), then ``_decode_logits``."""
    for layer, (kc, vc) in zip(self.model.layers, caches):
        x = layer.decode(x, cos, sin, kc, vc, t, key_mask, fp8=fp8, fp4=fp4)
    return _decode_logits(self, x, fp8, fp4)


def _fused_embedding_ok(emb: torch.Tensor, V: int, eos_token_id) -> bool:
    """Whether the fused selection kernels can read rows of the embedding table ``emb`` for a vocabulary of ``V``: bf16 rows,
    aligned, at least V of them, and the eos id (if any) one of them."""
    return (emb.dtype == torch.bfloat16 and emb.stride(1) == 1 and emb.stride(0) % 8 == 0 and emb.data_ptr() % 16 == 0
            and emb.shape[0] >= V and (eos_token_id is None or 0 <= int(eos_token_id) < emb.shape[0]))


def _lookup_args(self, inputs, num_tokens, max_ngram, do_sample, temperature, beams):
    """``generate``'s prompt-lookup arguments, checked before the model is touched: None when the mode is off, else
    (num_tokens, max_ngram)."""
    if max_ngram is not None and (isinstance(max_ngram, bool) or int(max_ngram) != max_ngram or int(max_ngram) < 1):
        raise ValueError(f"generate(max_matching_ngram_size={max_ngram!r}): has to be an integer >= 1")
    if num_tokens is None or (not isinstance(num_tokens, bool) and num_tokens == 0):
        return None
    if isinstance(num_tokens, bool) or int(num_tokens) != num_tokens or not 1 <= int(num_tokens) < ops.DECODE_LOOKUP_MAX_ROWS:
        raise ValueError(f"generate(prompt_lookup_num_tokens={num_tokens!r}): has to be an integer in 1 .. "
                         f"{ops.DECODE_LOOKUP_MAX_ROWS - 1} (a step verifies the last token and the drafts in at most "
                         f"{ops.DECODE_LOOKUP_MAX_ROWS} rows), or None / 0 for off")
    if inputs is not None and inputs.dim() == 2 and inputs.shape[0] != 1:
        raise ValueError(f"generate(prompt_lookup_num_tokens=...): batch size 1 only, got {inputs.shape[0]} (HF's assisted "
                         "decoding has the same rule)")
    if do_sample and temperature > 0:
        raise NotImplementedError("generate(prompt_lookup_num_tokens=..., do_sample=True): prompt-lookup decoding is greedy only")
    if beams > 1:
        raise NotImplementedError(f"generate(prompt_lookup_num_tokens=..., num_beams={beams}): prompt-lookup decoding does "
                                  "not combine with beam search")
    if ops.decode_kv_fp8_enabled(getattr(getattr(self, "config", None), "decode_kv_fp8", False)):
        raise NotImplementedError("generate(prompt_lookup_num_tokens=...): the multi-token step reads bf16 K / V caches; switch "
                                  "the e4m3 K / V cache off (config.decode_kv_fp8 / CAMBRIAN_AMD_DECODE_KV_FP8)")
    return int(num_tokens), 2 if max_ngram is None else int(max_ngram)


def lookup_step(self, ids, caches, t0: int, n_tok0: int, key_mask, fp8: bool = False, fp4: bool = False) -> torch.Tensor:
    """fp32 logits [Q, V] of Q consecutive tokens ``ids`` [Q] of ONE sequence in one step: embeddings, the RoPE table at
    positions n_tok0 .. n_tok0 + Q - 1, every layer's ``decode_multi`` (K / V of token j into cache slot t0 + j), final norm
    + lm_head.  Row j is the model's distribution after ids[: j + 1]."""
    model = self.model
    Q = ids.shape[0]
    hd = model.layers[0].self_attn.hd
    theta = float(getattr(self.config, "rope_theta", 10000.0))
    pos = torch.arange(n_tok0, n_tok0 + Q, dtype=torch.int64, device=ids.device)
    cos, sin = ops.rope_table(pos[:, None], hd, theta)
    x = model.embed_tokens(ids)[:, None, :].to(model.llm_dtype)
    for layer, (kc, vc) in zip(model.layers, caches):
        x = layer.decode_multi(x, cos, sin, kc, vc, t0, key_mask, fp8=fp8, fp4=fp4)
    return _decode_logits(self, x, fp8, fp4)


def _lookup_loop(self, logits, caches, key_mask, n_tok, L: int, max_new_tokens: int, eos_token_id, prompt_ids, prompt_mask,
                 lookup, draft_fn, fp8: bool, fp4: bool, hd: int, theta: float):
    """Greedy decoding of one prompt with prompt-lookup drafts (HF ``generate(prompt_lookup_num_tokens=...)``).  Every step
    drafts up to ``num_tokens`` ids from the prompt and the output so far; with d drafts it runs ``lookup_step`` on
    [last token, drafts] (Q = d + 1 rows), takes the argmax of every row — one host read — and emits the leading drafts the
    model reproduced plus the model's own next token.  K / V of rejected drafts stay in their slots, closed in the key mask,
    and are overwritten by the next step.  A step without drafts is the per-launch loop's step, ``layer.decode``.  Drafts are
    cut to the remaining budget, so no slot past L + max_new_tokens - 2 (the per-launch loop's last) is written."""
    from .lookup import accept, ngram_draft
    model = self.model
    num_tokens, max_ngram = lookup
    draft_fn = ngram_draft if draft_fn is None else draft_fn
    a0 = model.layers[0].self_attn
    max_rows = min(ops.DECODE_LOOKUP_MAX_ROWS, 64 // max(1, a0.nh // a0.nkv))
    vocab = logits.shape[1]
    eos = None if eos_token_id is None else int(eos_token_id)
    src = prompt_ids[0] if prompt_mask is None else prompt_ids[0][prompt_mask[0].bool()]
    src = [int(i) for i in src.tolist()]
    n0 = int(n_tok[0])
    out = [int(logits.argmax(-1)[0])]
    stats = {"steps": 0, "drafted": 0, "accepted": 0}
    while len(out) < max_new_tokens and not (eos is not None and out[-1] == eos):
        step = len(out) - 1
        t = L + step                                   # slot of the last emitted token, which this step feeds
        room = min(num_tokens, max_rows - 1, max_new_tokens - len(out) - 1)
        draft = [int(i) for i in draft_fn(src + out, room, max_ngram, vocab, eos)][:room] if room > 0 else []
        stats["steps"] += 1
        if not draft:
            key_mask[:, t] = True
            cos, sin = ops.rope_table((n_tok + step)[:, None], hd, theta)
            x = model.embed_tokens(torch.tensor([out[-1]], dtype=torch.int64, device=logits.device))[:, None, :].to(model.llm_dtype)
            out.append(int(_decode_token(self, x, cos, sin, caches, t, key_mask, fp8, fp4).argmax(-1)[0]))
            continue
        ids = torch.tensor([out[-1]] + draft, dtype=torch.int64, device=logits.device)
        picked = lookup_step(self, ids, caches, t, n0 + step, key_mask, fp8, fp4).argmax(-1).tolist()
        a = accept(draft, picked)
        key_mask[:, t:t + a + 1] = True
        stats["drafted"] += len(draft)
        stats["accepted"] += a
        new = draft[:a] + [int(picked[a])]
        if eos is not None and eos in new:
            new = new[:new.index(eos) + 1]
        out.extend(new)
    self.lookup_stats = stats
    return torch.tensor([out], dtype=torch.int64, device=logits.device)


def _kv8_wanted(self, dev, kv_out) -> bool:
    """Whether this ``generate()`` call keeps its K / V cache in e4m3 (``ops.decode_kv_fp8_enabled``): only when every
    layer's decode step takes the decode-attention kernel — GPU, bf16, ``CAMBRIAN_AMD_DECODE_ATTN`` not 0, one geometry
    that ``ops.decode_attention_kv8_supported`` accepts — because the SDPA branch of ``decode`` reads bf16 caches.  Otherwise
    the call keeps bf16 caches and nothing extra is allocated."""
    if not ops.decode_kv_fp8_enabled(getattr(getattr(self, "config", None), "decode_kv_fp8", False)):
        return False
    layers = self.model.layers
    if dev.type != "cuda" or not len(layers) or len(kv_out) != len(layers) or not ops.decode_attention_enabled():
        return False
    a0 = layers[0].self_attn
    return all((l.self_attn.nh, l.self_attn.nkv, l.self_attn.hd) == (a0.nh, a0.nkv, a0.hd) for l in layers) \
        and ops.decode_attention_kv8_supported(self.model.llm_dtype, a0.nh, a0.nkv, a0.hd) \
        and all(k.dtype == v.dtype == torch.bfloat16 and k.is_cuda for k, v in kv_out)


def _kv8_prefill(kv_out: list, B: int, nb: int, nkv: int, L: int, Lmax: int, hd: int, dev):
    """The e4m3 caches of ``B * nb`` rows (``nb`` beams per prompt, 1 = none) from the prefill's ``kv_out``, layer by layer:
    each layer's bf16 (k, v) is quantised (``ops.kv_quantize_e4m3``; with beams once per prompt, bytes and factors then copied
    into every beam's row) and dropped from ``kv_out`` before the next layer's cache is allocated, so the peak never holds both
    caches in full."""
    caches = []
    for i in range(len(kv_out)):
        pair = []
        for src in kv_out[i]:
            c = ops.KvCacheE4M3.empty(B * nb, nkv, Lmax, hd, dev)
            if nb == 1:
                ops.kv_quantize_e4m3(src, c, L)
            else:
                one = ops.kv_quantize_e4m3(src, ops.KvCacheE4M3.empty(B, nkv, L, hd, dev), L)
                c.q.view(B, nb, nkv, Lmax, hd)[:, :, :, :L] = one.q[:, None]
                c.inv.view(B, nb, nkv, Lmax)[:, :, :, :L] = one.inv[:, None]
            pair.append(c)
        kv_out[i] = None
        del src
        caches.append(tuple(pair))
    return caches


def _bf16_prefill(kv_out: list, B: int, nb: int, nkv: int, L: int, Lmax: int, hd: int, dev):
    """The caches of ``B * nb`` rows in the prefill's own dtype: zeros of ``Lmax`` slots per layer with the prefill's (k, v) in
    slots 0 .. L - 1, each prompt's columns copied into all of its ``nb`` beams' rows (1 = no beams)."""
    caches = []
    for k, v in kv_out:
        kc = torch.zeros(B * nb, nkv, Lmax, hd, dtype=k.dtype, device=dev)
        vc = torch.zeros_like(kc)
        kc.view(B, nb, nkv, Lmax, hd)[:, :, :, :L] = k[:, None]
        vc.view(B, nb, nkv, Lmax, hd)[:, :, :, :L] = v[:, None]
        caches.append((kc, vc))
    return caches


def _greedy_fused(plan, emb, logits, key_mask, n_tok, L0: int, max_new_tokens: int, eos_token_id, hd: int, theta: float,
                  proc=None, select=None):
    """The greedy loop as two library calls per token and no ATen call: ``ops.decode_next`` (selection, eos rule, position,
    key mask, embedding row, RoPE table; ``select``, given by ``_sample_fused``, stands in for it) then ``ops.decode_step``
    (every layer and the lm_head).  The first token comes from the prefill ``logits`` through the same selection.  With an
    eos id the host reads ``done`` only every ``ops.DECODE_STEP_POLL`` steps, so the loop may run up to that many tokens
    past the point where every row is done; ``ops.trim_after_all_done`` cuts the result back to the column where the
    per-token loop stops.  ``proc`` (an ``ops.DecodeProcess``): one more library call per token, ``ops.decode_process`` on
    the logits before the selection (HF's order: processors, then warpers), reading the ids in ``out``; a row that ends on a
    secondary eos is marked done by that call one step later, so the trim looks for ids of the set
    (``ops.trim_after_all_done_set``)."""
    select = ops.decode_next if select is None else select
    B = logits.shape[0]
    dev = logits.device
    eos = -1 if eos_token_id is None else int(eos_token_id)
    out = torch.zeros(B, max_new_tokens, dtype=torch.int64, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev) if eos >= 0 else None
    pos = torch.empty(B, dtype=torch.int64, device=dev)
    x = torch.empty(B, plan.H, dtype=torch.bfloat16, device=dev)
    cos = torch.empty(B, hd // 2, dtype=torch.float32, device=dev)
    sin = torch.empty_like(cos)
    n_tok = n_tok.contiguous()
    n = 0
    for step in range(max_new_tokens):
        if proc is not None:
            ops.decode_process(logits, out, step, proc, done)
        select(logits, eos, done, out, step, n_tok, pos, key_mask, L0 + step, emb, x, hd, theta, cos, sin)
        n = step + 1
        if n == max_new_tokens or (eos >= 0 and n % ops.DECODE_STEP_POLL == 0 and bool(done.all())):
            break
        logits = plan.step(x, cos, sin, L0 + step, key_mask)
    ids = out[:, :n]
    if eos >= 0:
        ids = ops.trim_after_all_done(ids, eos) if proc is None else ops.trim_after_all_done_set(ids, proc.spec.eos)
    return ids.contiguous()


def _sample_fused(plan, emb, logits, key_mask, n_tok, L0: int, max_new_tokens: int, eos_token_id, hd: int, theta: float,
                  temperature: float, top_k, top_p, proc=None):
    """``_greedy_fused`` with ``ops.decode_sample`` as the selection: temperature, top-k, top-p and the draw on the device, so
    sampled decoding too is two library calls per token and no ATen call.  ``top_k`` None / 0 and ``top_p`` None / >= 1 mean
    off; ``top_p <= 0`` raises what ``filter_logits_top_k_top_p`` raises.  The seed is one int64 drawn once per call ON the
    device from torch's generator (``torch.manual_seed`` governs it, the host never waits for it), before any buffer of the
    loop is allocated; the draws of a call are counted by (element, row, step) under that seed, so they are not
    torch.multinomial's stream."""
    k = 0 if top_k is None else max(int(top_k), 0)
    p = 1.0 if top_p is None or float(top_p) >= 1.0 else float(top_p)
    if not 0.0 < p:
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
    inv_t = float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))        # float32(1 / T), formed on the host
    seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=logits.device)

    def select(logits, *rest):
        ops.decode_sample(logits, inv_t, k, p, seed, *rest)

    return _greedy_fused(plan, emb, logits, key_mask, n_tok, L0, max_new_tokens, eos_token_id, hd, theta, proc, select)


def _beam_search(self, logits, kv_out, valid, L: int, max_new_tokens: int, eos_token_id, pad_token_id, nb: int,
                 kv8: bool = False):
    """Beam search after the prefill (``logits`` fp32 [B, V], ``kv_out`` every layer's K / V of the B prompts): the ``nb`` beams
    of a prompt are ``nb`` rows of a decode step, so the caches take ``nb`` times the memory of greedy decoding and the
    prompt's columns are copied into every beam's row.  Where the one-call plan is available the loop is ``_beam_fused``;
    else selection is ``beam.beam_update`` (plain torch) around ``layer.decode`` / ``plan.step``, and each step moves the
    generated columns of every cache from the parents' rows with an ``index_select``.  ``kv8``: e4m3 caches
    (``_kv8_wanted``) — the B prompts are quantised once and their bytes and factors copied into every beam's row, the
    selection is always the torch one (``cmb_decode_beam`` moves bf16 columns only) and the per-step ``index_select`` moves the
    generated columns of bytes and of factors."""
    model = self.model
    B, V = logits.shape
    dev = logits.device
    R = B * nb
    nh_kv, hd = model.layers[0].self_attn.nkv, model.layers[0].self_attn.hd
    Lmax = L + max_new_tokens
    caches = (_kv8_prefill if kv8 else _bf16_prefill)(kv_out, B, nb, nh_kv, L, Lmax, hd, dev)
    key_mask = torch.zeros(R, Lmax, dtype=torch.bool, device=dev)
    key_mask[:, :L] = valid.repeat_interleave(nb, dim=0)
    n_tok = valid.long().sum(1).repeat_interleave(nb).contiguous()
    logits = logits.repeat_interleave(nb, dim=0)
    theta = float(getattr(self.config, "rope_theta", 10000.0))
    fmt = ops.decode_weight_format(self.config)
    fp8, fp4 = fmt == "fp8", fmt == "fp4"
    fill = beam_fill(pad_token_id, eos_token_id)
    plan = None
    if max_new_tokens > 1 and ops.decode_step_enabled(getattr(self.config, "decode_step_fused", False)):
        plan = DecodeStepPlan.build(self, R, caches, Lmax - 1, fp8, fp4)
    if plan is not None and not kv8 and R <= ops.DECODE_BEAM_MAX and V >= 2 and V * nb < 2 ** 31:
        emb = model.embed_tokens.weight
        if _fused_embedding_ok(emb, V, eos_token_id):
            return _beam_fused(plan, emb, logits, key_mask, n_tok, L, max_new_tokens, eos_token_id, fill, nb, hd, theta)
    state = BeamState(B, nb, max_new_tokens, dev)
    first = (torch.arange(B, device=dev) * nb)[:, None]
    for step in range(max_new_tokens):
        parent, tok = beam_update(state, logits, step, eos_token_id, step + 1 == max_new_tokens)
        if step + 1 == max_new_tokens or beam_done(state):
            break
        t = L + step
        if step:
            rows = (parent + first).reshape(-1)
            for kc, vc in caches:
                for c in ((kc.q, kc.inv, vc.q, vc.inv) if kv8 else (kc, vc)):
                    c[:, :, L:t] = c[:, :, L:t].index_select(0, rows)
        key_mask[:, t] = True
        cos, sin = ops.rope_table((n_tok + step)[:, None], hd, theta)
        x = model.embed_tokens(tok.reshape(-1))[:, None, :].to(model.llm_dtype)
        if plan is not None:
            logits = plan.step(x[:, 0], cos, sin, t, key_mask)
        else:
            logits = _decode_token(self, x, cos, sin, caches, t, key_mask, fp8, fp4)
    return beam_result(state, fill)


def _beam_fused(plan, emb, logits, key_mask, n_tok, L0: int, max_new_tokens: int, eos_token_id, fill: int, nb: int, hd: int,
                theta: float):
    """Beam search as two library calls per token and no ATen call: ``ops.decode_beam`` (selection across the beams, the
    hypotheses, the early-stop flag, the K / V of the generated columns moved to each beam's row, position, key mask,
    embedding rows, RoPE table) then ``ops.decode_step``.  With an eos id the host reads the ``unfinished`` byte every
    ``ops.DECODE_STEP_POLL`` steps; steps past the stopping point cannot change the kept hypotheses (a new one scores 1e9
    lower once the flag is satisfied).  Without an eos id nothing is read before the last step."""
    R = logits.shape[0]
    dev = logits.device
    eos = -1 if eos_token_id is None else int(eos_token_id)
    state = ops.DecodeBeamState(R // nb, nb, max_new_tokens, dev)
    pos = torch.empty(R, dtype=torch.int64, device=dev)
    x = torch.empty(R, plan.H, dtype=torch.bfloat16, device=dev)
    cos = torch.empty(R, hd // 2, dtype=torch.float32, device=dev)
    sin = torch.empty_like(cos)
    n = 0
    for step in range(max_new_tokens):
        ops.decode_beam(logits, nb, eos, state, step, n_tok, pos, key_mask, L0 + step, emb, x, hd, theta, cos, sin, plan.desc,
                        plan.table, L0)
        n = step + 1
        if n == max_new_tokens or (eos >= 0 and n % ops.DECODE_STEP_POLL == 0 and not bool(state.unfinished.item())):
            break
        logits = plan.step(x, cos, sin, L0 + step, key_mask)
    return beam_result(state.view(n), fill)


CambrianLlamaForCausalLM.generate = _generate
CambrianLlamaForCausalLM.prefill_prefix = prefill_prefix
CambrianLlamaForCausalLM.extend_step = extend_step


def llama3_8b_config(**overrides) -> CambrianConfig:
    """Meta-Llama-3-8B-Instruct geometry (the LLM of Cambrian-8B, scripts/cambrian/pretrain_cambrian_8b.sh:12)."""
    kw = dict(vocab_size=128256, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
              num_key_value_heads=8, rms_norm_eps=1e-5, rope_theta=500000.0, max_position_embeddings=8192)
    kw.update(overrides)
    return CambrianConfig(**kw)


def apply_release_8b_vision_config(cfg, towers: Optional[List[str]] = None, token_lens: Optional[List[int]] = None):
    """scripts/cambrian/pretrain_cambrian_8b.sh:15-27 copied onto the config as train_fsdp.py:1671-1709 does."""
    cfg.mm_vision_tower_aux_list = towers or ["siglip/CLIP-ViT-SO400M-14-384", "openai/clip-vit-large-patch14-336",
                                              "facebook/dinov2-giant-res378", "clip-convnext-XXL-multi-stage"]
    cfg.mm_vision_tower_aux_token_len_list = token_lens or [576, 576, 576, 9216]
    cfg.image_token_len = 576
    cfg.num_query_group = 1
    cfg.query_num_list = [576]
    cfg.connector_depth = 3
    cfg.vision_hidden_size = 1024
    cfg.connector_only = False
    cfg.num_of_vision_sampler_layers = 10
    cfg.start_of_vision_sampler_layers = 0
    cfg.stride_of_vision_sampler_layers = 3
    cfg.mm_projector_type = "sva"
    cfg.image_position = 91
    cfg.mm_vision_select_layer = -2
    cfg.mm_vision_select_feature = "patch"
    cfg.unfreeze_mm_vision_tower = False
    cfg.sva_fused = True
    return cfg
