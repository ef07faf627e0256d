"""Skinny-M linear ops for decode steps (``csrc/kernels/gemm_skinny.hip``).

``skinny_linear`` / ``skinny_linear_t`` compute what ``ops.linear`` / ``ops.linear_gelu`` /
the unfused SwiGLU projection / ``ops.linear_t`` compute, for at most 16 rows of ``x``: on
the GPU (bf16) one weight-streaming kernel with the bias / GELU / SwiGLU epilogue applied
in fp32 before the single rounding to bf16.  They are inference ops: ``torch.no_grad()``,
nothing on the tape.

Where :func:`skinny_ok` is false (CPU tensors, fp32, more than 16 rows, strides the kernel
does not take, shapes measured slower than the path they would replace -- ``_routed`` --,
``FLAGS_skinny_gemm=0``) the functions evaluate exactly the expressions the
models used before these ops existed, so results on those inputs do not change.

The split count comes from the layout, N and K alone (:func:`skinny_default_splits`), and
for a given split count the kernel adds the K terms of an output element in one fixed
order: a row's result does not depend on the other rows of the call, and two runs give the
same bits.
"""
from __future__ import annotations

import torch

from ..utils import flags as _flags
from . import _native as N
from . import fused as F
from . import skinny_fp8 as _F8

__all__ = ["skinny_ok", "skinny_linear", "skinny_linear_t", "skinny_default_splits"]

MAX_ROWS = 16  # what the kernel covers
# What the ops route to it (measured, profiles/skinny_gemm_bench.md: the default routing is
# never slower than the path it replaces).  More than 8 rows lose to the MFMA paths on five
# of six llama-7b / GPT products; with N >= 8192 and no fused SwiGLU the vendor and training
# GEMMs have enough tiles of their own from 4 rows on, so those products are routed at one row.
ROUTED_ROWS = 8
WIDE_N = 8192


def _routed(b_kmaj, M, Nn, act):
    if M > ROUTED_ROWS:
        return False
    return M == 1 or Nn < WIDE_N or act == "swiglu_interleaved"
_EPI = {None: 0, "bias": 1, "gelu_tanh": 2, "swiglu_interleaved": 3}
_ACTS = (None, "gelu_tanh", "swiglu_interleaved")


def skinny_default_splits(b_kmaj, N_, K):
    """K slices for a [K, N] (``b_kmaj`` false) or [N, K] weight: a function of the layout,
    N and K only, computed on the host (``pa_gemm_skinny_splits``; no GPU needed).
    MN-major: enough (128-column tile, slice) workgroups for two per compute unit of a
    256-CU chip, slices of at least 256 K rows.  K-major: 16 outputs per workgroup, K cut
    only where N alone cannot fill the chip."""
    return int(N.lib().pa_gemm_skinny_splits(int(bool(b_kmaj)), int(N_), int(K)))


def _epi(bias, act):
    if act is None:
        return 0 if bias is None else 1
    return _EPI[act]


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _ld(t):
    """Row stride of a 2-D operand (a single row has no meaningful one: its length)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _problem(x, w, b_kmaj, bias, act, num_splits=None, policy=True):
    """(x2, M, N, K, epi, splits) when the kernel takes this call (and, with ``policy``, the
    ops route it there), else None."""
    if act not in _ACTS or (policy and not _flags.get("skinny_gemm")):
        return None
    if not (torch.is_tensor(x) and torch.is_tensor(w) and x.is_cuda and w.is_cuda and w.dim() == 2 and x.dim() >= 1
            and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.stride(1) == 1):
        return None
    Nn, K = (w.shape[0], w.shape[1]) if b_kmaj else (w.shape[1], w.shape[0])
    if K < 8 or x.shape[-1] != K or x.numel() == 0:
        return None
    M = x.numel() // K
    if M > MAX_ROWS or (policy and not _routed(b_kmaj, M, Nn, act)):
        return None
    if act == "gelu_tanh" and bias is None:
        return None
    if act == "swiglu_interleaved" and (bias is not None or b_kmaj):
        return None
    if bias is not None and not (bias.is_cuda and bias.dim() == 1 and bias.shape[0] == Nn and bias.is_contiguous()
                                 and bias.dtype in (torch.bfloat16, torch.float32)):
        return None
    x2 = x.reshape(M, K)  # a view for every layout the models produce
    if x2.stride(1) != 1:
        return None
    epi = _epi(bias, act)
    splits = skinny_default_splits(b_kmaj, Nn, K) if num_splits is None else int(num_splits)
    nout = Nn // 2 if epi == 3 else Nn
    # the output is a fresh contiguous [M, nout] buffer: 16-byte aligned, ldc = nout; the C
    # pointer is judged by alignment only, so a stand-in with the allocator's alignment does
    if not N.lib().pa_gemm_skinny_ok(int(b_kmaj), M, Nn, K, _ld(x2), _ld(w), nout, epi, splits, _ptr(x2), _ptr(w),
                                     256, _ptr(bias)):
        return None
    return x2, M, Nn, K, epi, splits


def skinny_ok(x, w, *, b_kmaj=False, bias=None, act=None) -> bool:
    """Whether ``skinny_linear`` (``b_kmaj`` false, w [K, N]) / ``skinny_linear_t`` (true, w
    [N, K]) runs the skinny kernel for these arguments (else: the models' usual path)."""
    return _problem(x, w, b_kmaj, bias, act) is not None


def _launch(b_kmaj, x2, w, out, bias, ws, M, Nn, K, epi, splits):
    """The one place a skinny kernel is launched from (tests wrap this to count)."""
    rc = N.lib().pa_gemm_skinny(int(b_kmaj), N.ptr(x2), N.ptr(w), N.ptr(out), N.ptr(bias),
                                int(bias is not None and bias.dtype == torch.float32), N.ptr(ws), M, Nn, K, _ld(x2),
                                _ld(w), _ld(out), epi, splits, N.stream())
    N.check(rc, "pa_gemm_skinny")
    return out


def _run(prob, x, w, b_kmaj, bias):
    x2, M, Nn, K, epi, splits = prob
    F.param_ready(w)
    if bias is not None:
        F.param_ready(bias)
    nout = Nn // 2 if epi == 3 else Nn
    out = torch.empty(M, nout, dtype=torch.bfloat16, device=x.device)
    nws = int(N.lib().pa_gemm_skinny_ws_floats(M, Nn, splits))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    _launch(b_kmaj, x2, w, out, bias, ws, M, Nn, K, epi, splits)
    return out.view(*x.shape[:-1], nout)


@torch.no_grad()
def skinny_kernel(x, w, *, b_kmaj=False, bias=None, act=None, num_splits=None):
    """The kernel itself wherever it covers the problem (up to 16 rows), whatever the routing
    policy and the flag say: for tests and benchmarks.  Raises where it does not."""
    prob = _problem(x, w, b_kmaj, bias, act, num_splits, policy=False)
    if prob is None:
        raise ValueError("skinny_kernel: the kernel does not cover this problem")
    return _run(prob, x, w, b_kmaj, bias)


@torch.no_grad()
def skinny_linear(x, w, bias=None, act=None, num_splits=None):
    """x [..., K] (at most 16 rows) times w [K, N] (a bf16 tensor or an ``ops.Fp8Weight``) with
    an optional epilogue:

    * ``act=None``: ``x w (+ bias)`` -- ``ops.linear``;
    * ``act="gelu_tanh"``: ``gelu(x w + bias)`` -- ``ops.linear_gelu``;
    * ``act="swiglu_interleaved"``: w is a gate|up matrix in the interleaved layout of
      ``ops.interleave_gate_up``; returns ``silu(gate) * up`` [..., N/2]."""
    if act not in _ACTS:
        raise ValueError(f"skinny_linear: unknown act {act!r}")
    if isinstance(w, _F8.Fp8Weight):
        # e4m3 weight (ops/skinny_fp8.py): its own kernel where routed, else the expressions
        # below on the dequantised weight, which is exact
        out = _F8.linear(x, w, bias, act, num_splits)
        if out is not None:
            return out
        w, num_splits = _F8.dequant_for(x, w), None
    prob = _problem(x, w, False, bias, act, num_splits)
    if prob is not None:
        return _run(prob, x, w, False, bias)
    if act is None:
        return F.linear(x, w, bias)
    if act == "gelu_tanh":
        return F.linear_gelu(x, w, bias)
    gu = F.linear(x, w, bias)
    g, u = F.deinterleave_gate_up(gu)
    return (torch.nn.functional.silu(g.float()) * u.float()).to(x.dtype)


@torch.no_grad()
def skinny_linear_t(x, w, num_splits=None):
    """x [..., K] (at most 16 rows) times w^T for w [N, K] (a tied embedding table used as
    the LM head; any N) -- ``ops.linear_t``."""
    prob = _problem(x, w, True, None, None, num_splits)
    if prob is not None:
        return _run(prob, x, w, True, None)
    return F.linear_t(x, w)
