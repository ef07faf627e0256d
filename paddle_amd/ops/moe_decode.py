"""MoE FFN for decode steps (``csrc/kernels/moe_decode.hip``): routing and the selected experts'
SwiGLU MLPs for at most 16 rows, streaming only the experts the rows picked, once each.

``moe_decode_route`` / ``moe_decode_ffn`` are inference ops (``torch.no_grad()``, nothing on the
tape).  The plain-torch functions below are the CPU path, the fallback wherever
:func:`moe_decode_ok` is false, and the definition of the contract:

* **routing** -- logits ``x . gate_w`` in fp32 in a summation order fixed by (H, E) alone; NaN
  counts as ``-inf``; the k largest logits win, among equal logits the lower expert index;
  the selection is listed in descending-logit order; the weights are the softmax over the k
  selected logits (``renorm``: gshard / switch with k > 1, as ``TopKGate._route`` decides) or
  the full-softmax probabilities.  For any input the k indices are in ``[0, E)`` and pairwise
  distinct; the weights are unspecified when the logits are not finite.
* **FFN** -- per (row t, choice j, expert e): ``g, u = x_t . gate_up[e]`` accumulated in fp32,
  ``a = round(silu(g) * u)``, ``y_t = round(sum_j w_tj * (a . down[e]))`` with fp32 accumulation
  and j ascending: two roundings (to ``x.dtype``) per call.
* **invariance** -- row t of an M-row call equals the 1-row call on that row bit for bit, in
  ``idx``, ``w`` and ``y``; two runs give the same bits; a row's result does not depend on which
  experts other rows chose.

On the GPU a call is four launches (route, gate|up, down, combine) whose grids come from
M, k, E, H, I alone; nothing is read back from the device, so a call can be captured into a
HIP graph.  ``gate_up`` keeps the model's ``[gate | up]`` column layout; no second image of the
weights is made.
"""
from __future__ import annotations

import torch

from ..utils import flags as _flags
from . import _native as N
from . import fused as F
from .skinny import MAX_ROWS

__all__ = ["moe_decode_ok", "moe_decode_route", "moe_decode_ffn", "moe_decode_default_splits"]

MAX_EXPERTS = 256
MAX_TOP_K = 16
# What the ops route to the kernels (measured, profiles/moe_decode_bench.md: faster than
# MoELayer.forward on grouped experts by more than its spread at every row count up to 16).
ROUTED_ROWS = MAX_ROWS


def moe_decode_default_splits(H, I):
    """(gate|up, down) K slices: functions of H and I only, computed on the host
    (``pa_moe_decode_splits``; no GPU needed)."""
    L = N.lib()
    return int(L.pa_moe_decode_splits(0, int(H), int(I))), int(L.pa_moe_decode_splits(1, int(H), int(I)))


# ------------------------------------------------------------------ the definition (plain torch)
def _shapes(x, gate_w, gate_up, down, top_k):
    if not (torch.is_tensor(x) and x.dim() >= 1 and gate_w.dim() == 2):
        raise ValueError("moe_decode: x [..., H] and gate_w [H, E] expected")
    H, E = gate_w.shape
    if x.shape[-1] != H or x.numel() == 0:
        raise ValueError(f"moe_decode: x {tuple(x.shape)} does not match gate_w {tuple(gate_w.shape)}")
    M = x.numel() // H
    k = int(top_k)
    if M > MAX_ROWS:
        raise ValueError(f"moe_decode: {M} rows; a decode call has at most {MAX_ROWS}")
    if not 1 <= k <= min(E, MAX_TOP_K):
        raise ValueError(f"moe_decode: top_k {k} outside [1, min(E = {E}, {MAX_TOP_K})]")
    I = None
    if gate_up is not None:
        if gate_up.dim() != 3 or down.dim() != 3 or gate_up.shape[0] != E or gate_up.shape[1] != H \
                or gate_up.shape[2] % 2 or tuple(down.shape) != (E, gate_up.shape[2] // 2, H):
            raise ValueError(f"moe_decode: gate_up {tuple(gate_up.shape)} / down {tuple(down.shape)} do not match "
                             f"E = {E}, H = {H}")
        I = gate_up.shape[2] // 2
    return M, H, I, E, k


def _route_ref(x2, gate_w, k, renorm):
    # [M, H, E] products summed over H: an order that does not depend on M
    logits = (x2.float().unsqueeze(-1) * gate_w.float().unsqueeze(0)).sum(1)
    logits = torch.where(logits != logits, torch.full_like(logits, float("-inf")), logits)
    # a stable descending sort lists equal logits by ascending expert index
    sl, si = torch.sort(logits, dim=-1, descending=True, stable=True)
    idx, sel = si[:, :k], sl[:, :k]
    if renorm:
        w = torch.softmax(sel, -1)
    else:
        w = torch.softmax(logits, -1).gather(1, idx)
    return idx.to(torch.int32), w


def _ffn_ref(x2, gate_up, down, idx, w):
    M, k = idx.shape
    I = down.shape[1]
    ys = []
    for t in range(M):  # row by row: a row's result cannot depend on the other rows
        e = idx[t].long()
        gu = torch.einsum("h,khn->kn", x2[t].float(), gate_up[e].float())
        a = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]).to(x2.dtype)
        o = torch.einsum("ki,kih->kh", a.float(), down[e].float())
        acc = w[t, 0] * o[0]
        for j in range(1, k):
            acc = acc + w[t, j] * o[j]
        ys.append(acc.to(x2.dtype))
    return torch.stack(ys)


# ------------------------------------------------------------------ the kernels
def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _rows(x, gate_w, policy):
    """x as an [M, H] view with unit column stride when the router kernel takes it (and, with
    ``policy``, the ops route the call to the kernels), else None."""
    if policy and not _flags.get("moe_decode"):
        return None
    if not (x.is_cuda and torch.is_tensor(gate_w) and gate_w.is_cuda):
        return None
    if x.dtype != torch.bfloat16 or gate_w.dtype != torch.float32 or not gate_w.is_contiguous():
        return None
    H = gate_w.shape[0]
    M = x.numel() // H
    if policy and M > ROUTED_ROWS:
        return None
    x2 = x.reshape(M, H)  # a view for every layout the models produce
    return x2 if x2.stride(1) == 1 else None


def _route_problem(x, gate_w, top_k, policy=True):
    """x as [M, H] when ``pa_moe_decode_route`` takes this call, else None."""
    x2 = _rows(x, gate_w, policy)
    if x2 is None:
        return None
    M, H = x2.shape
    if not N.lib().pa_moe_decode_route_ok(M, H, gate_w.shape[1], int(top_k), _ld(x2), x2.data_ptr(),
                                          gate_w.data_ptr()):
        return None
    return x2


def _problem(x, gate_w, gate_up, down, top_k, policy=True):
    """x as [M, H] when the kernels take this call (and, with ``policy``, the ops route it
    there), else None."""
    x2 = _rows(x, gate_w, policy)
    if x2 is None:
        return None
    if not (gate_up.is_cuda and down.is_cuda and gate_up.dtype == torch.bfloat16 and down.dtype == torch.bfloat16
            and gate_up.is_contiguous() and down.is_contiguous()):
        return None
    M, H = x2.shape
    if not N.lib().pa_moe_decode_ok(M, H, gate_up.shape[2] // 2, gate_w.shape[1], int(top_k), _ld(x2), x2.data_ptr(),
                                    gate_w.data_ptr(), gate_up.data_ptr(), down.data_ptr()):
        return None
    return x2


def moe_decode_ok(x, gate_w, gate_up, down, top_k) -> bool:
    """Whether ``moe_decode_ffn`` runs the kernels for these arguments (else: the plain-torch
    definition).  False for CPU tensors, fp32 inputs and ``FLAGS_moe_decode=0``."""
    try:
        _shapes(x, gate_w, gate_up, down, top_k)
    except ValueError:
        return False
    return _problem(x, gate_w, gate_up, down, top_k) is not None


def _launch_route(x2, gate_w, k, renorm):
    """The one place the route kernel is launched from (tests wrap this to count)."""
    M, H = x2.shape
    idx = torch.empty(M, k, dtype=torch.int32, device=x2.device)
    w = torch.empty(M, k, dtype=torch.float32, device=x2.device)
    N.call("pa_moe_decode_route", N.ptr(x2), _ld(x2), N.ptr(gate_w), N.ptr(idx), N.ptr(w), M, H, gate_w.shape[1], k,
           int(bool(renorm)), N.stream())
    return idx, w


def _launch_ffn(x2, gate_up, down, idx, w, splits, out=None):
    """The one place the three FFN kernels are launched from.  ``out``: a [M, H] bf16 view with
    unit column stride to write instead of a fresh buffer."""
    M, H = x2.shape
    E, _, I2 = gate_up.shape
    I, k = I2 // 2, idx.shape[1]
    sg, sd = splits
    nws = int(N.lib().pa_moe_decode_ws_floats(M, H, I, k, sg, sd))
    if nws < 0:
        raise ValueError("moe_decode_ffn: the split counts need a workspace beyond 2^31 floats")
    ws = torch.empty(nws, dtype=torch.float32, device=x2.device)
    y = torch.empty(M, H, dtype=torch.bfloat16, device=x2.device) if out is None else out
    N.call("pa_moe_decode_ffn", N.ptr(x2), _ld(x2), N.ptr(gate_up), N.ptr(down), N.ptr(idx), N.ptr(w), N.ptr(ws),
           N.ptr(y), _ld(y), M, H, I, E, k, sg, sd, N.stream())
    return y


def _splits(num_splits, H, I):
    if num_splits is None:
        return moe_decode_default_splits(H, I)
    if isinstance(num_splits, (tuple, list)):
        sg, sd = num_splits
        return int(sg), int(sd)
    return int(num_splits), int(num_splits)


@torch.no_grad()
def moe_decode_kernel(x, gate_w, gate_up, down, top_k, renorm=True, num_splits=None):
    """The kernels themselves wherever they cover the problem (up to 16 rows), whatever the
    routing policy and the flag say: for tests and benchmarks.  Raises where they do not."""
    M, H, I, E, k = _shapes(x, gate_w, gate_up, down, top_k)
    x2 = _problem(x, gate_w, gate_up, down, k, policy=False)
    if x2 is None:
        raise ValueError("moe_decode_kernel: the kernels do not cover this problem")
    idx, w = _launch_route(x2, gate_w, k, renorm)
    return _launch_ffn(x2, gate_up, down, idx, w, _splits(num_splits, H, I)).view(x.shape)


@torch.no_grad()
def moe_decode_route(x, gate_w, top_k, renorm=True):
    """Router of a decode call: x [..., H] (at most 16 rows), gate_w [H, E] fp32 -> (idx [M, k]
    int32, w [M, k] fp32), see the module docstring."""
    M, H, _, E, k = _shapes(x, gate_w, None, None, top_k)
    x2 = _route_problem(x, gate_w, k)
    if x2 is not None:
        F.param_ready(gate_w)
        return _launch_route(x2, gate_w, k, renorm)
    return _route_ref(x.reshape(M, H), gate_w, k, bool(renorm))


@torch.no_grad()
def moe_decode_ffn(x, gate_w, gate_up, down, top_k, renorm=True, num_splits=None):
    """Top-k MoE FFN of a decode call: x [..., H] (at most 16 rows), gate_w [H, E] fp32, gate_up
    [E, H, 2I] (``[gate | up]`` columns) and down [E, I, H] -> y like x.  ``num_splits``: K
    slices of the two products (an int for both, or a pair; default
    :func:`moe_decode_default_splits`)."""
    M, H, I, E, k = _shapes(x, gate_w, gate_up, down, top_k)
    x2 = _problem(x, gate_w, gate_up, down, k)
    if x2 is not None:
        for p in (gate_w, gate_up, down):
            F.param_ready(p)
        idx, w = _launch_route(x2, gate_w, k, renorm)
        return _launch_ffn(x2, gate_up, down, idx, w, _splits(num_splits, H, I)).view(x.shape)
    x2 = x.reshape(M, H)
    idx, w = _route_ref(x2, gate_w, k, bool(renorm))
    return _ffn_ref(x2, gate_up, down, idx, w).view(x.shape)
