"""MXFP4 weight GEMM for more rows than the decode kernel covers
(``csrc/kernels/gemm_rows_mxfp4.hip``).

``ops.mxfp4_linear(x, w4, bias, act)`` is ``ops.skinny_linear`` for an ``ops.Mxfp4Weight`` and
any row count: up to 16 rows it *is* ``skinny_linear`` (the weight-streaming kernel of
ops/skinny_mxfp4.py); from 17 to ``ROUTED_ROWS`` rows of bf16 ``x`` on the GPU it runs the
multi-row-tile MFMA kernel on the same packed image -- no dequantised copy of the weight is
written or read --; everything else (CPU, fp32, more rows, shapes the kernel refuses,
``FLAGS_mxfp4_rows=0``) is ``skinny_linear`` again, i.e. the usual expression on ``w4.dequant()``.

The kernel keeps the decode kernel's arithmetic: the K terms of an output element are added in
one fixed order that depends on (N, K, num_splits) only.  A row's result does not depend on the
row count, on the row's position or on the other rows, two runs give the same bits, and for an
equal ``num_splits`` a row has the bits of ``skinny_mxfp4.skinny_kernel`` for that row.  The
default split count (:func:`rows_mxfp4_default_splits`) is a function of (N, K) only but is
smaller than the decode kernel's -- the fp32 partials of 256 rows cost more traffic than the
weight --, so with the default splits a row's bits may change between a 16-row and a 17-row
call.
"""
from __future__ import annotations

import torch

from ..utils import flags as _flags
from . import _native as N
from . import fused as F
from . import skinny as _SK
from .skinny_mxfp4 import GROUP, Mxfp4Weight, _ACTS, _epi, _ld, _ptr

__all__ = ["mxfp4_linear", "mxfp4_linear_ok", "rows_mxfp4_default_splits"]

MAX_ROWS = 256  # what the kernel covers
MIN_ROUTED_ROWS = 17  # up to 16 rows the decode kernel reads the weight once and is never slower
# The largest row count up to which the kernel beats dequant + ops.linear by more than that
# baseline's spread on all four llama-7b products (profiles/mxfp4_rows_bench.md: at 192 rows
# qkv and gate|up lose, 0.95x and 1.00x).
ROUTED_ROWS = 128


def rows_mxfp4_default_splits(N_, K):
    """K slices for a [K, N] mxfp4 weight: a function of N and K only, computed on the host
    (``pa_gemm_rows_mxfp4_splits``; no GPU needed)."""
    return int(N.lib().pa_gemm_rows_mxfp4_splits(int(N_), int(K)))


def _problem(x, w, bias, act, num_splits=None, policy=True):
    """(x2, packed, scale, M, N, K, epi, splits) when the kernel takes this call (and, with
    ``policy``, ``mxfp4_linear`` routes it there), else None."""
    if act not in _ACTS or (policy and not _flags.get("mxfp4_rows")) or not isinstance(w, Mxfp4Weight):
        return None
    pk, sc = w.packed, w.scale_e8m0
    if not (torch.is_tensor(x) and x.is_cuda and pk.is_cuda and sc.is_cuda and x.dim() >= 1
            and x.dtype == torch.bfloat16 and sc.is_contiguous()):
        return None
    K, Nn = sc.shape[0] * GROUP, sc.shape[1]
    if x.shape[-1] != K or x.numel() == 0:
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
    splits = rows_mxfp4_default_splits(Nn, K) if num_splits is None else int(num_splits)
    nout = Nn // 2 if epi == 3 else Nn
    # the output is a fresh contiguous [M, nout] buffer: a stand-in with the allocator's alignment
    if not N.lib().pa_gemm_rows_mxfp4_ok(M, Nn, K, _ld(x2), nout, epi, splits, _ptr(x2), _ptr(pk), 256, _ptr(bias),
                                         _ptr(sc)):
        return None
    return x2, pk, sc, M, Nn, K, epi, splits


def mxfp4_linear_ok(x, w, bias=None, act=None) -> bool:
    """Whether ``mxfp4_linear(x, w, bias, act)`` runs the multi-row-tile kernel (else:
    ``ops.skinny_linear``)."""
    return _problem(x, w, bias, act) is not None


def _launch(x2, pk, sc, out, bias, ws, M, Nn, K, epi, splits):
    """The one place the kernel is launched from (tests wrap this to count)."""
    rc = N.lib().pa_gemm_rows_mxfp4(N.ptr(x2), N.ptr(pk), N.ptr(sc), N.ptr(out), N.ptr(bias),
                                    int(bias is not None and bias.dtype == torch.float32), N.ptr(ws), M, Nn, K,
                                    _ld(x2), _ld(out), epi, splits, N.stream())
    N.check(rc, "pa_gemm_rows_mxfp4")
    return out


def _run(prob, x, bias):
    x2, pk, sc, M, Nn, K, epi, splits = prob
    if bias is not None:
        F.param_ready(bias)
    nout = Nn // 2 if epi == 3 else Nn
    out = torch.empty(M, nout, dtype=torch.bfloat16, device=x.device)
    nws = int(N.lib().pa_gemm_rows_mxfp4_ws_floats(M, Nn, splits))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    _launch(x2, pk, sc, out, bias, ws, M, Nn, K, epi, splits)
    return out.view(*x.shape[:-1], nout)


@torch.no_grad()
def rows_kernel(x, w, *, bias=None, act=None, num_splits=None):
    """The kernel itself wherever it covers the problem (1..256 rows), whatever the routing
    policy and the flag say: for tests and benchmarks.  Raises where it does not."""
    prob = _problem(x, w, bias, act, num_splits, policy=False)
    if prob is None:
        raise ValueError("rows_mxfp4.rows_kernel: the kernel does not cover this problem")
    return _run(prob, x, bias)


@torch.no_grad()
def mxfp4_linear(x, w, bias=None, act=None, num_splits=None):
    """``ops.skinny_linear(x, w, bias, act)`` for an ``ops.Mxfp4Weight`` w [K, N] and any row
    count of x [..., K]; ``act`` as there (None, "gelu_tanh", "swiglu_interleaved")."""
    if act not in _ACTS:
        raise ValueError(f"mxfp4_linear: unknown act {act!r}")
    prob = _problem(x, w, bias, act, num_splits)
    if prob is not None:
        return _run(prob, x, bias)
    return _SK.skinny_linear(x, w, bias, act)
