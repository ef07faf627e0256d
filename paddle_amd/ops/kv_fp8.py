"""The quantisation contract of the fp8 (OCP e4m3fn) KV cache, in plain torch.

One power-of-two scale per vector of ``D`` elements -- one (token, kv head) -- and one code
per element.  This file is the definition: the CPU path, the reference the GPU kernels of
``csrc/kernels/attn_decode.hip`` (``pa_kv_append_f8`` ...) are tested against bit for bit,
and what ``KVCache.dequant`` runs.

  amax   max |x_i| over the vector; a NaN element is ignored, an infinite amax counts as
         the largest finite fp32
  scale  2 ** clamp(ceil(log2(amax / 448)), -100, 100), and 1 for an all-zero vector (the
         rule of ``quantize_weight_fp8``).  In integers on the bits of amax = m * 2^e, m in
         [1, 2): the exponent is e - 8, plus one when m > 1.75 (448 = 1.75 * 2^8)
  codes  round_to_nearest_even(x / scale) clamped to +-448: a finite or infinite input never
         gives a NaN code, a NaN gives a NaN code (as the bf16 cache would have kept it)

``codes * scale`` is exact in bf16 and fp32 (4 significant bits, exponents within
[-109, 109]), so a quantised cache is exactly a bf16 cache that holds the dequantised values.
Quantising those values again may halve the scale (an amax that rounded down to
``224 * scale``): the map is not idempotent.
"""
from __future__ import annotations

import torch

__all__ = ["quantize_kv_fp8", "dequantize_kv_fp8", "KV_DTYPES", "E4M3_MAX"]

E4M3_MAX = 448.0
KV_DTYPES = ("fp8_e4m3",)
_FP8 = getattr(torch, "float8_e4m3fn", None)
_F32_MAX = torch.finfo(torch.float32).max


def check_kv_dtype(kv_dtype):
    """None (a cache in the model's dtype) or one of ``KV_DTYPES``; anything else raises."""
    if kv_dtype is not None and kv_dtype not in KV_DTYPES:
        raise ValueError(f"unknown kv_dtype {kv_dtype!r} (supported: None, {', '.join(map(repr, KV_DTYPES))})")
    return kv_dtype


@torch.no_grad()
def quantize_kv_fp8(x):
    """``x [..., D]`` (bf16 or fp32) -> ``(codes [..., D] float8_e4m3fn, scale [...] fp32)``."""
    if not (torch.is_tensor(x) and x.dim() >= 1 and x.dtype in (torch.bfloat16, torch.float32)):
        raise ValueError("quantize_kv_fp8: a bf16 or fp32 tensor [..., D] is expected")
    xf = x.detach().float()
    a = xf.abs()
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(-1).clamp(max=_F32_MAX)  # frexp(inf) has e = 0
    # frexp: amax = m * 2^e with m in [0.5, 1), so amax / 448 = (m / 0.875) * 2^(e - 9)
    m, e = torch.frexp(amax)
    e = (e - 9 + (m > 0.875).to(e.dtype)).clamp(-100, 100)
    one = torch.ones_like(amax)
    scale = torch.where(amax > 0, torch.ldexp(one, e), one)
    codes = (xf / scale.unsqueeze(-1)).clamp(-E4M3_MAX, E4M3_MAX).to(_FP8)  # clamp keeps a NaN
    return codes, scale


@torch.no_grad()
def dequantize_kv_fp8(codes, scale, dtype=torch.bfloat16):
    """``codes * scale`` in ``dtype`` (exact in bf16 and fp32)."""
    return (codes.float() * scale.unsqueeze(-1)).to(dtype)
