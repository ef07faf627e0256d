"""Weight-only e4m3 GEMM for more rows than the decode kernel covers
(``csrc/kernels/gemm_rows_f8.hip``).

``ops.fp8_linear(x, w8, bias, act)`` is ``ops.skinny_linear`` for an ``ops.Fp8Weight`` and any
row count: up to 16 rows it *is* ``skinny_linear`` (the weight-streaming kernel of
ops/skinny_fp8.py); from 17 to ``ROUTED_ROWS`` rows of bf16 ``x`` on the GPU it runs the
multi-row-tile MFMA kernel on the codes as stored -- no dequantised copy of the weight is written
or read and no second layout of the codes is kept --; everything else (CPU, fp32, more rows,
shapes the kernel refuses, ``FLAGS_fp8_rows=0``) is ``skinny_linear`` again, i.e. the usual
expression on ``w8.dequant()``.

The K terms of an output element are added in one fixed order that depends on (N, K,
num_splits) only: a row's result does not depend on the row count, on the row's position or on
the other rows, and two runs give the same bits.  The default split count
(:func:`rows_fp8_default_splits`) is a function of (N, K) only.  **Not** promised: the bits of
``skinny_fp8.skinny_kernel`` (fp32 FMAs there, MFMA here) or of dequant + ``ops.linear`` -- a
row's bits may change when a call crosses from 16 to 17 rows, as they did before this kernel.
"""
from __future__ import annotations

import torch

from ..utils import flags as _flags
from . import _native as N
from . import fused as F
from . import skinny as _SK
from .skinny_fp8 import Fp8Weight, _ACTS, _epi, _ld, _ptr

__all__ = ["fp8_linear", "fp8_linear_ok", "rows_fp8_default_splits"]

MAX_ROWS = 256  # what the kernel covers
MIN_ROUTED_ROWS = 17  # up to 16 rows the decode kernel reads the weight once
# The largest measured row count at which the kernel beats dequant + ops.linear by more than that
# baseline's spread on all four llama-7b products (profiles/fp8_rows_bench.md: at 192 rows qkv
# and gate|up lose, 0.95x and 0.93x).
ROUTED_ROWS = 128


def rows_fp8_default_splits(N_, K):
    """K slices for a [K, N] e4m3 weight: a function of N and K only, computed on the host
    (``pa_gemm_rows_f8_splits``; no GPU needed)."""
    return int(N.lib().pa_gemm_rows_f8_splits(int(N_), int(K)))


def _problem(x, w, bias, act, num_splits=None, policy=True):
    """(x2, q, scale, M, N, K, epi, splits) when the kernel takes this call (and, with
    ``policy``, ``fp8_linear`` routes it there), else None."""
    if act not in _ACTS or (policy and not _flags.get("fp8_rows")) or not isinstance(w, Fp8Weight):
        return None
    q, scale = w.q, w.scale  # once: a module's buffers are looked up through __getattr__
    if not (torch.is_tensor(x) and x.is_cuda and q.is_cuda and scale.is_cuda and x.dim() >= 1
            and x.dtype == torch.bfloat16 and q.stride(1) == 1 and scale.is_contiguous()):
        return None
    K, Nn = q.shape
    if K < 1 or x.shape[-1] != K or x.numel() == 0:
        return None
    M = x.numel() // K
    if M > MAX_ROWS or (policy and not MIN_ROUTED_ROWS <= M <= ROUTED_ROWS):
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
    splits = rows_fp8_default_splits(Nn, K) if num_splits is None else int(num_splits)
    nout = Nn // 2 if epi == 3 else Nn
    # the output is a fresh contiguous [M, nout] buffer: a stand-in with the allocator's alignment
    if not N.lib().pa_gemm_rows_f8_ok(M, Nn, K, _ld(x2), _ld(q), nout, epi, splits, _ptr(x2), _ptr(q), 256,
                                      _ptr(bias), _ptr(scale)):
        return None
    return x2, q, scale, M, Nn, K, epi, splits


def fp8_linear_ok(x, w, bias=None, act=None) -> bool:
    """Whether ``fp8_linear(x, w, bias, act)`` runs the multi-row-tile kernel (else:
    ``ops.skinny_linear``)."""
    return _problem(x, w, bias, act) is not None


def _launch(x2, q, scale, out, bias, ws, M, Nn, K, epi, splits):
    """The one place the kernel is launched from (tests wrap this to count)."""
    rc = N.lib().pa_gemm_rows_f8(N.ptr(x2), N.ptr(q), _ld(q), N.ptr(scale), N.ptr(out), N.ptr(bias),
                                 int(bias is not None and bias.dtype == torch.float32), N.ptr(ws), M, Nn, K,
                                 _ld(x2), _ld(out), epi, splits, N.stream())
    N.check(rc, "pa_gemm_rows_f8")
    return out


def _run(prob, x, bias):
    x2, q, scale, M, Nn, K, epi, splits = prob
    if bias is not None:
        F.param_ready(bias)
    nout = Nn // 2 if epi == 3 else Nn
    out = torch.empty(M, nout, dtype=torch.bfloat16, device=x.device)
    nws = int(N.lib().pa_gemm_rows_f8_ws_floats(M, Nn, splits))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    _launch(x2, q, scale, out, bias, ws, M, Nn, K, epi, splits)
    return out.view(*x.shape[:-1], nout)


@torch.no_grad()
def rows_kernel(x, w, *, bias=None, act=None, num_splits=None):
    """The kernel itself wherever it covers the problem (1..256 rows), whatever the routing
    policy and the flag say: for tests and benchmarks.  Raises where it does not."""
    prob = _problem(x, w, bias, act, num_splits, policy=False)
    if prob is None:
        raise ValueError("rows_fp8.rows_kernel: the kernel does not cover this problem")
    return _run(prob, x, bias)


@torch.no_grad()
def fp8_linear(x, w, bias=None, act=None, num_splits=None):
    """``ops.skinny_linear(x, w, bias, act)`` for an ``ops.Fp8Weight`` w [K, N] and any row
    count of x [..., K]; ``act`` as there (None, "gelu_tanh", "swiglu_interleaved")."""
    if act not in _ACTS:
        raise ValueError(f"fp8_linear: unknown act {act!r}")
    prob = _problem(x, w, bias, act, num_splits)
    if prob is not None:
        return _run(prob, x, bias)
    return _SK.skinny_linear(x, w, bias, act)
