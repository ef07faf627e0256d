"""MXFP4 (OCP MX: e2m1 codes, e8m0 group scales) weight-only storage for the decode-step GEMMs
(``csrc/kernels/gemm_skinny_mxfp4.hip``).

``quantize_weight_mxfp4(w)`` turns a ``[K, N]`` weight (``K % 32 == 0``) into an
:class:`Mxfp4Weight`: one 4-bit code per element and one power-of-two scale per group of 32
consecutive ``k`` of one output column ``n``,

    scale[g, n] = 2 ** clamp(ceil(log2(amax_group / 6)), -100, 100)    (1 for an all-zero group)
    code        = e2m1(round_to_nearest_even(w / scale), clamped to +-6)

stored as the e8m0 byte ``exponent + 127`` in ``scale_e8m0 [K/32, N]``.  An e2m1 code is a sign
(bit 3) and one of the magnitudes ``0, .5, 1, 1.5, 2, 3, 4, 6`` (bits 0..2); a zero result gets
code 0.  ``code * scale`` is exact in bf16, so a quantised layer *is* the bf16 layer whose
weight is ``w.dequant()``: every path that does not run the mxfp4 kernel evaluates the existing
expression on ``w.dequant()`` and loses nothing.  ``|w - dq| <= max(|w|, scale) / 4``: with
``a = |w| / scale <= 6`` the grid's step is 1/2 up to 2, 1 up to 4 and 2 up to 6, so half a step
is at most 1/4 in the first range and at most a / 4 in the other two.  Storage is 4 + 8 / 32 =
4.25 bits per element.

Packed image (``packed``, uint8, the kernel's streaming order; the canonical code tensor is not
kept): ``[ceil(N / 16) strips][K / 32 groups][16 columns][16 bytes]``, N padded to a multiple of
16 with zero codes, K not padded.  The 16 bytes at ``((ct * K / 32 + g) * 16 + c) * 16`` hold the
32 codes of one scale group, ``k = 32 g .. 32 g + 31`` of column ``16 ct + c``: byte ``b`` has
``k + 2 b`` in its low nibble and ``k + 2 b + 1`` in its high one.  Four consecutive groups of a
strip are one 1 KiB load of a wave (16 columns x 128 ``k``, lane ``kb * 16 + c`` taking its 16
bytes), and the loads of a strip are contiguous in ascending ``k``.

``ops.skinny_linear(x, w, ...)`` accepts an ``Mxfp4Weight`` for ``w``: on the GPU with bf16 ``x``,
at most ``ROUTED_ROWS`` rows and ``N % 16 == 0`` the MFMA weight-streaming kernel (fp32
accumulation, bias, activation, one rounding); otherwise (CPU, fp32, more rows, shapes the
kernel does not cover, ``FLAGS_skinny_mxfp4=0``) the usual expression on ``w.dequant()``.

The split count is a function of (N, K) only and the K terms of an output element are added
in one fixed order: a row's result does not depend on the other rows of the call, and two
runs give the same bits.
"""
from __future__ import annotations

import torch

from ..utils import flags as _flags
from . import _native as N
from . import fused as F

__all__ = ["Mxfp4Weight", "quantize_weight_mxfp4", "skinny_mxfp4_ok", "skinny_mxfp4_default_splits"]

E2M1_MAX = 6.0
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
GROUP = 32
TILE_N = 16
MAX_ROWS = 16  # what the kernel covers
# What skinny_linear routes to it: one instantiation and one pass over the weight for every row
# count (profiles/skinny_mxfp4_bench.md has the measurements against dequant + ops.linear).
ROUTED_ROWS = 16

_EPI = {None: 0, "bias": 1, "gelu_tanh": 2, "swiglu_interleaved": 3}
_ACTS = (None, "gelu_tanh", "swiglu_interleaved")


def _table(device, dtype=torch.float32):
    v = torch.tensor(E2M1_VALUES, dtype=dtype, device=device)
    return torch.cat([v, -v])


def _pack(codes):
    """Codes ``[K, N]`` uint8 -> the packed image (see the module docstring)."""
    K, Nn = codes.shape
    NT = -(-Nn // TILE_N)
    full = torch.zeros(K, NT * TILE_N, dtype=torch.uint8, device=codes.device)
    full[:, :Nn] = codes
    # [g, b, nibble, ct, c] -> [ct, g, c, b, nibble]
    t = full.view(K // GROUP, 16, 2, NT, TILE_N).permute(3, 0, 4, 1, 2)
    return (t[..., 0] | (t[..., 1] << 4)).contiguous().view(-1)


def _unpack(packed, K, Nn):
    NT = -(-Nn // TILE_N)
    t = packed.view(NT, K // GROUP, TILE_N, 16)
    t = torch.stack([t & 15, t >> 4], -1)  # [ct, g, c, b, nibble]
    return t.permute(1, 3, 4, 0, 2).reshape(K, NT * TILE_N)[:, :Nn].contiguous()


class Mxfp4Weight(torch.nn.Module):
    """A ``[K, N]`` weight held as the packed e2m1 image ``packed`` and the e8m0 group scales
    ``scale_e8m0 [K/32, N]`` (buffers of a module, so ``model.to(...)`` moves them and
    ``buffers()`` counts them)."""

    def __init__(self, packed, scale_e8m0):
        super().__init__()
        if not (torch.is_tensor(scale_e8m0) and scale_e8m0.dtype == torch.uint8 and scale_e8m0.dim() == 2):
            raise ValueError("Mxfp4Weight: scale_e8m0 must be a 2-D uint8 tensor [K/32, N]")
        G, Nn = scale_e8m0.shape
        want = G * -(-Nn // TILE_N) * 256
        if not (torch.is_tensor(packed) and packed.dtype == torch.uint8 and packed.dim() == 1
                and packed.numel() == want and packed.is_contiguous()):
            raise ValueError(f"Mxfp4Weight: packed must be a contiguous uint8 tensor of {want} bytes")
        self.register_buffer("packed", packed, persistent=False)
        self.register_buffer("scale_e8m0", scale_e8m0, persistent=False)

    @property
    def shape(self):
        G, Nn = self.scale_e8m0.shape
        return torch.Size((G * GROUP, Nn))

    @property
    def device(self):
        return self.packed.device

    @property
    def nbytes(self):
        return self.packed.numel() + self.scale_e8m0.numel()

    def codes(self):
        """The e2m1 codes ``[K, N]`` uint8 (values 0..15), unpacked in plain torch."""
        return _unpack(self.packed, *self.shape)

    @torch.no_grad()
    def dequant(self, dtype=torch.bfloat16):
        """A fresh ``[K, N]`` tensor ``code * scale`` (exact in bf16 and fp32).  Never a cached
        or reused buffer: ops cache derived images on the tensor objects they are given."""
        pk, sc = self.packed, self.scale_e8m0
        K, Nn = self.shape
        if dtype == torch.bfloat16 and pk.is_cuda and Nn % 16 == 0 and K > 0 and sc.is_contiguous() \
                and pk.data_ptr() % 16 == 0:
            out = torch.empty(K, Nn, dtype=torch.bfloat16, device=pk.device)
            N.call("pa_mxfp4w_dequant", N.ptr(pk), N.ptr(sc), N.ptr(out), K, Nn, Nn, N.stream())
            return out
        vals = _table(pk.device)[self.codes().long()]
        scale = torch.ldexp(torch.ones((), device=pk.device), sc.to(torch.int32) - 127)
        return (vals.view(K // GROUP, GROUP, Nn) * scale[:, None, :]).view(K, Nn).to(dtype)

    def extra_repr(self):
        K, Nn = self.shape
        return f"K={K}, N={Nn}, e2m1 codes + e8m0 scales per 32 k"


@torch.no_grad()
def quantize_weight_mxfp4(w) -> Mxfp4Weight:
    """``w [K, N]`` (any float dtype, in the layout the layer holds; ``K % 32 == 0``) ->
    :class:`Mxfp4Weight`.  Plain torch, the same code on the CPU and the GPU.  Raises
    ``ValueError`` for a K that is no multiple of 32 and for a non-finite value."""
    if not (torch.is_tensor(w) and w.dim() == 2 and w.is_floating_point()):
        raise ValueError("quantize_weight_mxfp4: a 2-D floating-point weight is expected")
    K, Nn = w.shape
    if K == 0 or K % GROUP or Nn == 0:
        raise ValueError(f"quantize_weight_mxfp4: K = {K} is not a positive multiple of {GROUP}")
    wf = w.detach().float()
    if not torch.isfinite(wf).all():
        raise ValueError("quantize_weight_mxfp4: the weight has a non-finite value")
    wg = wf.view(K // GROUP, GROUP, Nn)
    amax = wg.abs().amax(1)
    # frexp: amax / 6 = m * 2^e with m in [0.5, 1), so ceil(log2(.)) is e, or e - 1 at m == 0.5
    m, e = torch.frexp(amax / E2M1_MAX)
    e = torch.where(m == 0.5, e - 1, e).clamp(-100, 100)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    scale = torch.ldexp(torch.ones_like(amax), e)
    a = (wg / scale[:, None, :]).abs().clamp(max=E2M1_MAX)
    # round to nearest even on the grid: steps of .5 below 2, of 1 below 4, of 2 above
    # (torch.round rounds halves to even, and an even count of steps is an even e2m1 mantissa)
    a = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
    mag = torch.bucketize(a, torch.tensor(E2M1_VALUES, device=a.device))  # a is on the grid: its index
    codes = (mag | ((wg < 0) & (mag > 0)).long() << 3).to(torch.uint8).view(K, Nn)
    return Mxfp4Weight(_pack(codes), (e + 127).to(torch.uint8).contiguous())


def skinny_mxfp4_default_splits(N_, K):
    """K slices for a [K, N] mxfp4 weight: a function of N and K only, computed on the host
    (``pa_gemm_skinny_mxfp4_splits``; no GPU needed)."""
    return int(N.lib().pa_gemm_skinny_mxfp4_splits(int(N_), int(K)))


def _epi(bias, act):
    if act is None:
        return 0 if bias is None else 1
    return _EPI[act]


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _problem(x, w, bias, act, num_splits=None, policy=True):
    """(x2, packed, scale, M, N, K, epi, splits) when the mxfp4 kernel takes this call (and,
    with ``policy``, the ops route it there), else None."""
    if act not in _ACTS or (policy and not _flags.get("skinny_mxfp4")) or not isinstance(w, Mxfp4Weight):
        return None
    pk, sc = w.packed, w.scale_e8m0  # once: a module's buffers are looked up through __getattr__
    if not (torch.is_tensor(x) and x.is_cuda and pk.is_cuda and sc.is_cuda and x.dim() >= 1
            and x.dtype == torch.bfloat16 and sc.is_contiguous()):
        return None
    K, Nn = sc.shape[0] * GROUP, sc.shape[1]
    if x.shape[-1] != K or x.numel() == 0:
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
    splits = skinny_mxfp4_default_splits(Nn, K) if num_splits is None else int(num_splits)
    nout = Nn // 2 if epi == 3 else Nn
    # the output is a fresh contiguous [M, nout] buffer: a stand-in with the allocator's alignment
    if not N.lib().pa_gemm_skinny_mxfp4_ok(M, Nn, K, _ld(x2), nout, epi, splits, _ptr(x2), _ptr(pk), 256, _ptr(bias),
                                           _ptr(sc)):
        return None
    return x2, pk, sc, M, Nn, K, epi, splits


def skinny_mxfp4_ok(x, w, bias=None, act=None) -> bool:
    """Whether ``skinny_linear(x, w, bias, act)`` runs the mxfp4 kernel for the ``Mxfp4Weight``
    w (else: the usual expression on ``w.dequant()``)."""
    return _problem(x, w, bias, act) is not None


def _launch(x2, pk, sc, out, bias, ws, M, Nn, K, epi, splits):
    """The one place the mxfp4 skinny kernel is launched from (tests wrap this to count)."""
    rc = N.lib().pa_gemm_skinny_mxfp4(N.ptr(x2), N.ptr(pk), N.ptr(sc), N.ptr(out), N.ptr(bias),
                                      int(bias is not None and bias.dtype == torch.float32), N.ptr(ws), M, Nn, K,
                                      _ld(x2), _ld(out), epi, splits, N.stream())
    N.check(rc, "pa_gemm_skinny_mxfp4")
    return out


def _run(prob, x, bias):
    x2, pk, sc, M, Nn, K, epi, splits = prob
    if bias is not None:
        F.param_ready(bias)
    nout = Nn // 2 if epi == 3 else Nn
    out = torch.empty(M, nout, dtype=torch.bfloat16, device=x.device)
    nws = int(N.lib().pa_gemm_skinny_mxfp4_ws_floats(M, Nn, splits))
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    _launch(x2, pk, sc, out, bias, ws, M, Nn, K, epi, splits)
    return out.view(*x.shape[:-1], nout)


@torch.no_grad()
def skinny_kernel(x, w, *, bias=None, act=None, num_splits=None):
    """The mxfp4 kernel itself wherever it covers the problem (up to 16 rows), whatever the
    routing policy and the flag say: for tests and benchmarks.  Raises where it does not."""
    prob = _problem(x, w, bias, act, num_splits, policy=False)
    if prob is None:
        raise ValueError("skinny_mxfp4.skinny_kernel: the kernel does not cover this problem")
    return _run(prob, x, bias)


def linear(x, w, bias, act, num_splits):
    """``skinny_linear`` for an ``Mxfp4Weight``: the kernel where it is routed, else None (the
    caller evaluates its usual expression on ``w.dequant()``)."""
    prob = _problem(x, w, bias, act, num_splits)
    return None if prob is None else _run(prob, x, bias)


def dequant_for(x, w):
    """``w.dequant()`` in ``x``'s dtype, as the parent expression wants it (bf16 and fp32 hold
    ``code * scale`` exactly)."""
    return w.dequant(x.dtype if x.is_floating_point() else torch.bfloat16)
