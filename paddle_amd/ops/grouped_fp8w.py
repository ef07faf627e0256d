"""SwiGLU expert MLP over expert-sorted rows on ``Fp8ExpertWeights`` as they are stored
(``csrc/kernels/moe_rows_f8.hip``): the quantised MoE layer for more rows than
``ops.moe_decode_ffn`` covers, with no dequantised image of any expert.

``grouped_swiglu_mlp_fp8w(x, gate_up, down, counts)`` is an inference op (``torch.no_grad()``,
nothing on the tape).  ``x [R, H]`` holds the rows sorted by expert, ``counts [E]`` the rows per
expert (a device tensor -- no host read on the kernel path -- or host ints that sum to R),
``gate_up [E, H, 2I]`` (``[gate | up]`` columns) and ``down [E, I, H]`` are two
:class:`Fp8ExpertWeights`.  The plain-torch function below is the CPU path, the fallback wherever
:func:`grouped_fp8w_ok` is false, and the definition of the contract:

* per row r of expert e: ``g, u = x_r . gate_up[e]`` accumulated in fp32 over the exact images of
  the codes, the power-of-two column scale applied to the sum, ``a = round(silu(g) * u)``,
  ``y_r = round(a . down[e])`` likewise: two roundings (to ``x.dtype``) per row;
* a row's result does not depend on R, on the counts, on its position or on the other rows, and
  two runs give the same bits.  Equal bits to ``moe_decode_ffn`` or to the dequantised path are
  not promised.

On the GPU a call is two launches (gate|up + SwiGLU, down) whose grids come from R and E alone;
the offsets are made on the device and nothing is read back.
"""
from __future__ import annotations

import itertools

import torch

from ..utils import flags as _flags
from . import _native as N
from .moe_decode import Fp8ExpertWeights

__all__ = ["grouped_swiglu_mlp_fp8w", "grouped_fp8w_ok", "grouped_fp8w_kernel"]

# tile constants of moe_rows_f8.hip (kTileM, kChunkK; ``pa_moe_rows_f8_const`` returns the same)
TM = 32         # rows per workgroup
CHUNK_K = 512   # k of the rows a workgroup stages at a time
MAX_EXPERTS = 256
# The largest number of sorted rows (tokens x top_k) that ``GroupedSwiGLUExperts.forward_grouped``
# routes here (None would be no limit).  Measured at the a3b shapes (profiles/moe_rows_fp8_bench.md):
# 5.0x to 3.9x faster than dequant + the bf16 grouped GEMM at 102..1536 sorted rows, 1.46x at 6144
# (1024 tokens x 6), 0.58x at 24576: the largest count of the list that is won.
ROUTED_SORTED_ROWS = 6144


def _shapes(x, gate_up, down, counts):
    if isinstance(gate_up, Fp8ExpertWeights) != isinstance(down, Fp8ExpertWeights):
        raise ValueError("grouped_swiglu_mlp_fp8w: gate_up and down must both be Fp8ExpertWeights")
    if not isinstance(gate_up, Fp8ExpertWeights):
        raise ValueError("grouped_swiglu_mlp_fp8w: Fp8ExpertWeights stacks expected (bf16 stacks: "
                         "ops.grouped.grouped_swiglu_mlp)")
    if not (torch.is_tensor(x) and x.dim() == 2):
        raise ValueError("grouped_swiglu_mlp_fp8w: x [R, H] expected")
    R, H = x.shape
    E, Hg, I2 = gate_up.shape
    if Hg != H or I2 % 2 or tuple(down.shape) != (E, I2 // 2, H):
        raise ValueError(f"grouped_swiglu_mlp_fp8w: gate_up {tuple(gate_up.shape)} / down {tuple(down.shape)} do "
                         f"not match x {tuple(x.shape)}")
    if torch.is_tensor(counts):
        if counts.numel() != E or counts.is_floating_point():
            raise ValueError(f"grouped_swiglu_mlp_fp8w: counts must hold {E} integers")
    else:
        counts = [int(c) for c in counts]
        if len(counts) != E or min(counts, default=0) < 0 or sum(counts) != R:
            raise ValueError(f"grouped_swiglu_mlp_fp8w: counts must be {E} non-negative ints that sum to R = {R}")
    return R, H, I2 // 2, E, counts


def _ref(x, gate_up, down, counts):
    """The definition: row by row in fp32 on dequantised images of the experts that have rows."""
    if torch.is_tensor(counts):
        counts = [int(c) for c in counts.tolist()]
        if sum(counts) != x.shape[0] or min(counts, default=0) < 0:
            raise ValueError("grouped_swiglu_mlp_fp8w: counts must be non-negative and sum to the rows of x")
    I = down.shape[1]
    y = torch.empty_like(x)
    r = 0
    for e, n in enumerate(counts):
        if n == 0:
            continue
        sel = torch.tensor([e])
        gu, dn = gate_up.dequant(torch.float32, experts=sel)[0], down.dequant(torch.float32, experts=sel)[0]
        for t in range(r, r + n):  # a row's result cannot depend on the other rows
            h = x[t].float() @ gu
            a = (torch.nn.functional.silu(h[:I]) * h[I:]).to(x.dtype)
            y[t] = (a.float() @ dn).to(x.dtype)
        r += n
    return y


def _problem(x, gate_up, down, policy=True):
    """Whether ``pa_moe_rows_f8`` takes these operands (and, with ``policy``, the op routes them
    there)."""
    if policy and not _flags.get("moe_rows_fp8"):
        return False
    if not (isinstance(gate_up, Fp8ExpertWeights) and isinstance(down, Fp8ExpertWeights)):
        return False
    ts = (gate_up.q, gate_up.scale, down.q, down.scale)
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[0] > 0
            and x.stride(1) == 1 and all(t.is_cuda and t.is_contiguous() for t in ts)):
        return False
    R, H = x.shape
    E, Hg, I2 = gate_up.shape
    if Hg != H or I2 % 2 or tuple(down.shape) != (E, I2 // 2, H):
        return False
    # a and y are fresh contiguous buffers: a stand-in with the allocator's alignment
    return bool(N.lib().pa_moe_rows_f8_ok(R, H, I2 // 2, E, _ld(x), x.data_ptr(), *(t.data_ptr() for t in ts), 256,
                                          256, 256))


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def grouped_fp8w_ok(x, gate_up, down) -> bool:
    """Whether ``grouped_swiglu_mlp_fp8w`` runs the kernels for these operands (else: the
    plain-torch definition).  False for CPU tensors, fp32 rows, H or I no multiple of 16, more
    than 256 experts and ``FLAGS_moe_rows_fp8=0``."""
    return _problem(x, gate_up, down)


def _offsets(counts, device):
    """offs [E + 1] int32 on the device, as ``grouped.expert_offsets`` makes them."""
    if torch.is_tensor(counts):
        offs = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=device)
        offs[1:] = torch.cumsum(counts.reshape(-1).to(device), 0)
        return offs
    return torch.tensor([0, *itertools.accumulate(counts)], dtype=torch.int32).to(device, non_blocking=True)


def _launch(x, gate_up, down, offs):
    """The one place the kernels are launched from."""
    R, H = x.shape
    E, _, I2 = gate_up.shape
    I = I2 // 2
    a = torch.empty(R, I, dtype=torch.bfloat16, device=x.device)
    y = torch.empty(R, H, dtype=torch.bfloat16, device=x.device)
    N.call("pa_moe_rows_f8", N.ptr(x), _ld(x), N.ptr(gate_up.q), N.ptr(gate_up.scale), N.ptr(down.q),
           N.ptr(down.scale), N.ptr(offs), N.ptr(a), N.ptr(y), R, H, I, E, N.stream())
    return y


@torch.no_grad()
def grouped_fp8w_kernel(x, gate_up, down, counts):
    """The kernels themselves wherever they cover the problem, whatever the routing policy and the
    flag say: for tests and benchmarks.  Raises where they do not."""
    R, H, I, E, counts = _shapes(x, gate_up, down, counts)
    if not _problem(x, gate_up, down, policy=False):
        raise ValueError("grouped_fp8w_kernel: the kernels do not cover this problem")
    return _launch(x, gate_up, down, _offsets(counts, x.device))


@torch.no_grad()
def grouped_swiglu_mlp_fp8w(x, gate_up, down, counts):
    """``x [R, H]`` sorted by expert, ``gate_up`` / ``down``: :class:`Fp8ExpertWeights`, ``counts
    [E]`` -> ``y [R, H]``; see the module docstring."""
    R, H, I, E, counts = _shapes(x, gate_up, down, counts)
    if R == 0:
        return x.clone()
    if _problem(x, gate_up, down):
        return _launch(x, gate_up, down, _offsets(counts, x.device))
    return _ref(x, gate_up, down, counts)
