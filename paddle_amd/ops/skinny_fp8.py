"""FP8 (OCP e4m3) weight-only storage for the decode-step GEMMs
(``csrc/kernels/gemm_skinny_f8.hip``).

``quantize_weight_fp8(w)`` turns a ``[K, N]`` weight into an :class:`Fp8Weight`: codes
``q [K, N]`` (``torch.float8_e4m3fn``) and one fp32 scale per output column,

    scale[n] = 2 ** clamp(ceil(log2(amax_n / 448)), -100, 100)     (1 for an all-zero column)
    q        = round_to_nearest_even(w / scale), clamped to +-448  (so never a NaN code)

The scale is a power of two, so ``q * scale`` is exactly representable in bf16 (3 mantissa
bits against 7) and scaling a sum equals summing scaled terms bit for bit in fp32: a
quantised layer *is* the bf16 layer whose weight is ``w.dequant()``.  Every path that does
not run the fp8 kernel therefore evaluates the existing expression on ``w.dequant()`` and
loses nothing.

``ops.skinny_linear(x, w, ...)`` accepts an ``Fp8Weight`` for ``w``: on the GPU with bf16
``x`` and at most ``ROUTED_ROWS`` (16) rows the weight-streaming fp8 kernel (fp32 accumulation,
scale, bias, activation, one rounding); otherwise (CPU, fp32, more rows, shapes the kernel
does not cover, ``FLAGS_skinny_fp8=0``) the usual expression on ``w.dequant()``.

The split count is a function of (N, K) only and the K terms of an output element are added
in one fixed order: a row's result does not depend on the other rows of the call, and two
runs give the same bits.
"""
from __future__ import annotations

import torch

from ..utils import flags as _flags
from . import _native as N
from . import fused as F

__all__ = ["Fp8Weight", "quantize_weight_fp8", "skinny_fp8_ok", "skinny_fp8_default_splits"]

E4M3_MAX = 448.0
_FP8 = torch.float8_e4m3fn
MAX_ROWS = 16  # what the kernel covers
# What skinny_linear routes to it: all of them.  The bf16 kernel stops at 8 rows because the
# MFMA GEMMs win beyond; a quantised model's only alternative is dequant + ops.linear, which
# the kernel beats 1.2x to 2x on every llama-7b product even at 16 rows, where its two passes
# of 8 read the weight twice (profiles/skinny_fp8_bench.md).
ROUTED_ROWS = 16

_EPI = {None: 0, "bias": 1, "gelu_tanh": 2, "swiglu_interleaved": 3}
_ACTS = (None, "gelu_tanh", "swiglu_interleaved")


class Fp8Weight(torch.nn.Module):
    """A ``[K, N]`` weight held as e4m3 codes ``q [K, N]`` and fp32 column scales ``scale [N]``
    (buffers of a module, so ``model.to(...)`` moves them and ``buffers()`` counts them)."""

    def __init__(self, q, scale):
        super().__init__()
        if not (torch.is_tensor(q) and q.dtype == _FP8 and q.dim() == 2):
            raise ValueError("Fp8Weight: q must be a 2-D torch.float8_e4m3fn tensor")
        if not (torch.is_tensor(scale) and scale.dtype == torch.float32 and scale.shape == (q.shape[1],)):
            raise ValueError("Fp8Weight: scale must be fp32 of shape [N]")
        self.register_buffer("q", q, persistent=False)
        self.register_buffer("scale", scale, persistent=False)

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @property
    def nbytes(self):
        return self.q.numel() + 4 * self.scale.numel()

    @torch.no_grad()
    def dequant(self, dtype=torch.bfloat16):
        """A fresh ``[K, N]`` tensor ``q * scale`` (bf16 by default: exact for the quantiser's
        power-of-two scales; otherwise the fp32 product rounded once).  Never a cached or
        reused buffer: ops cache derived images on the tensor objects they are given."""
        q, s = self.q, self.scale
        K, Nn = q.shape
        if dtype == torch.bfloat16 and q.is_cuda and Nn % 16 == 0 and q.stride(1) == 1 and q.stride(0) % 16 == 0 \
                and q.data_ptr() % 16 == 0 and s.is_contiguous() and K > 0:
            out = torch.empty(K, Nn, dtype=torch.bfloat16, device=q.device)
            N.call("pa_fp8w_dequant", N.ptr(q), N.ptr(s), N.ptr(out), K, Nn, q.stride(0), Nn, N.stream())
            return out
        return (q.float() * s).to(dtype)

    def extra_repr(self):
        return f"K={self.q.shape[0]}, N={self.q.shape[1]}, e4m3 codes + fp32 column scales"


@torch.no_grad()
def quantize_weight_fp8(w) -> Fp8Weight:
    """``w [K, N]`` (any float dtype, in the layout the layer holds) -> :class:`Fp8Weight`.
    Plain torch, the same code on the CPU and the GPU.  Raises ``ValueError`` for a weight
    with a non-finite value."""
    if not (torch.is_tensor(w) and w.dim() == 2 and w.is_floating_point()):
        raise ValueError("quantize_weight_fp8: a 2-D floating-point weight is expected")
    wf = w.detach().float()
    if not torch.isfinite(wf).all():
        raise ValueError("quantize_weight_fp8: the weight has a non-finite value")
    amax = wf.abs().amax(0)
    # frexp: amax / 448 = m * 2^e with m in [0.5, 1), so ceil(log2(.)) is e, or e - 1 at m == 0.5
    m, e = torch.frexp(amax / E4M3_MAX)
    e = torch.where(m == 0.5, e - 1, e).clamp(-100, 100)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
    q = (wf / scale).clamp(-E4M3_MAX, E4M3_MAX).to(_FP8)
    return Fp8Weight(q.contiguous(), scale.contiguous())


def skinny_fp8_default_splits(N_, K):
    """K slices for a [K, N] e4m3 weight: a function of N and K only, computed on the host
    (``pa_gemm_skinny_f8_splits``; no GPU needed)."""
    return int(N.lib().pa_gemm_skinny_f8_splits(int(N_), int(K)))


def _epi(bias, act):
    if act is None:
        return 0 if bias is None else 1
    return _EPI[act]


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _problem(x, w, bias, act, num_splits=None, policy=True):
    """(x2, q, scale, M, N, K, epi, splits) when the fp8 kernel takes this call (and, with
    ``policy``, the ops route it there), else None."""
    if act not in _ACTS or (policy and not _flags.get("skinny_fp8")) or not isinstance(w, Fp8Weight):
        return None
    q, scale = w.q, w.scale  # once: a module's buffers are looked up through __getattr__
    if not (torch.is_tensor(x) and x.is_cuda and q.is_cuda and x.dim() >= 1 and x.dtype == torch.bfloat16
            and q.stride(1) == 1 and scale.is_contiguous()):
        return None
    K, Nn = q.shape
    if K < 8 or x.shape[-1] != K or x.numel() == 0:
        return None
    M = x.numel() // K
    if M > MAX_ROWS or (policy and M > ROUTED_ROWS):
        return None
    if act == "gelu_tanh" and bias is None:
        return None
    if act == "swiglu_interleaved" and bias is not None:
        return None
    if bias is not None and not (torch.is_tensor(bias) and bias.is_cuda and bias.dim() == 1 and bias.shape[0] == Nn
                                 and bias.is_contiguous() and bias.dtype in (torch.bfloat16, torch.float32)):
        return None
    x2 = x.reshape(M, K)
    if x2.stride(1) != 1:
        return None
    epi = _epi(bias, act)
    splits = skinny_fp8_default_splits(Nn, K) if num_splits is None else int(num_splits)
    nout = Nn // 2 if epi == 3 else Nn
    # the output is a fresh contiguous [M, nout] buffer: a stand-in with the allocator's alignment
    if not N.lib().pa_gemm_skinny_f8_ok(M, Nn, K, _ld(x2), _ld(q), nout, epi, splits, _ptr(x2), _ptr(q), 256,
                                        _ptr(bias), _ptr(scale)):
        return None
    return x2, q, scale, M, Nn, K, epi, splits


def skinny_fp8_ok(x, w, bias=None, act=None) -> bool:
    """Whether ``skinny_linear(x, w, bias, act)`` runs the fp8 kernel for the ``Fp8Weight`` w
    (else: the usual expression on ``w.dequant()``)."""
    return _problem(x, w, bias, act) is not None


def _launch(x2, q, scale, out, bias, ws, M, Nn, K, epi, splits):
    """The one place the fp8 skinny kernel is launched from (tests wrap this to count)."""
    rc = N.lib().pa_gemm_skinny_f8(N.ptr(x2), N.ptr(q), N.ptr(scale), N.ptr(out), N.ptr(bias),
                                   int(bias is not None and bias.dtype == torch.float32), N.ptr(ws), M, Nn, K,
                                   _ld(x2), _ld(q), _ld(out), epi, splits, N.stream())
    N.check(rc, "pa_gemm_skinny_f8")
    return out


def _run(prob, x, bias):
    x2, q, scale, M, Nn, K, epi, splits = prob
    if bias is not None:
        F.param_ready(bias)
    nout = Nn // 2 if epi == 3 else Nn
    out = torch.empty(M, nout, dtype=torch.bfloat16, device=x.device)
    nws = int(N.lib().pa_gemm_skinny_f8_ws_floats(M, Nn, splits))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    _launch(x2, q, scale, out, bias, ws, M, Nn, K, epi, splits)
    return out.view(*x.shape[:-1], nout)


@torch.no_grad()
def skinny_kernel(x, w, *, bias=None, act=None, num_splits=None):
    """The fp8 kernel itself wherever it covers the problem (up to 16 rows), whatever the
    routing policy and the flag say: for tests and benchmarks.  Raises where it does not."""
    prob = _problem(x, w, bias, act, num_splits, policy=False)
    if prob is None:
        raise ValueError("skinny_fp8.skinny_kernel: the kernel does not cover this problem")
    return _run(prob, x, bias)


def linear(x, w, bias, act, num_splits):
    """``skinny_linear`` for an ``Fp8Weight``: the kernel where it is routed, else None (the
    caller evaluates its usual expression on ``w.dequant()``)."""
    prob = _problem(x, w, bias, act, num_splits)
    return None if prob is None else _run(prob, x, bias)


def dequant_for(x, w):
    """``w.dequant()`` in ``x``'s dtype, as the parent expression wants it (bf16 and fp32 hold
    ``q * scale`` exactly)."""
    return w.dequant(x.dtype if x.is_floating_point() else torch.bfloat16)
