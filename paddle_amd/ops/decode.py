"""KV-cache decode ops: the cache object, ``kv_append``, ``decode_attention`` (one new token
per row) and ``extend_attention`` (T new tokens per row, causal inside the chunk).

GPU bf16 tensors run the gfx950 kernels of ``csrc/kernels/attn_decode.hip`` (and
``csrc/kernels/attn_extend.hip``: the MFMA kernel behind ``extend_attention``); CPU
tensors, other dtypes and shapes the kernels do not cover run the plain-torch
definitions below (the fp32 oracle of the GPU tests).  These are inference ops: they
record nothing on the tape and run under ``torch.no_grad()``.

Cache layout: per layer ``k`` / ``v`` ``[B, max_len, Hk, D]`` (token-major, the layout
the packed QKV projection already has, so an append is a row copy), and one int32
device tensor ``lens[B]`` shared by all layers: the number of valid tokens per row.
Rows may have different lengths (right-padded prompts); nothing on the decode path
reads ``lens`` back to the host.

``PagedKVCache`` (:mod:`paddle_amd.ops.paged`) stores the same tokens in fixed-size blocks
from a shared pool; ``kv_append`` and ``decode_attention`` take either cache.

``kv_dtype="fp8_e4m3"`` (either cache) stores e4m3 codes in the same layout plus one
power-of-two fp32 scale per (token, kv head) in ``k_scale`` / ``v_scale`` ``[B, max_len, Hk]``:
the contract of :mod:`paddle_amd.ops.kv_fp8`.  ``kv_append`` quantises what the bf16 cache
would have stored; ``decode_attention`` computes what it computes over a bf16 cache that
holds ``cache.dequant(layer)``, bit for bit on the GPU kernels.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from .fused import _attn_ref, _check_scale, _fa_strides, ctypes_long_array
from .kv_fp8 import _FP8, check_kv_dtype, dequantize_kv_fp8, quantize_kv_fp8

__all__ = ["KVCache", "PagedKVCache", "kv_append", "decode_attention", "extend_attention",
           "default_extend_splits"]


class KVCache:
    """Per-layer key / value storage for incremental decoding.

    ``lens`` (int32, device) holds each row's valid length; ``max_len`` and an upper
    bound of ``lens`` live on the host, so an append past the end raises without a
    device read.  One step is: ``kv_append`` + ``decode_attention`` per layer (both see
    the same ``lens``), then one ``advance(T)``."""

    def __init__(self, num_layers, batch, max_len, num_kv_heads, head_dim, dtype=torch.bfloat16, device=None,
                 kv_dtype=None):
        self.kv_dtype = check_kv_dtype(kv_dtype)
        self.num_layers, self.batch, self.max_len = int(num_layers), int(batch), int(max_len)
        self.num_kv_heads, self.head_dim = int(num_kv_heads), int(head_dim)
        self.dtype, self.device = dtype, torch.device(device if device is not None else "cpu")
        shape = (self.batch, self.max_len, self.num_kv_heads, self.head_dim)
        store = _FP8 if self.quantized else dtype  # dtype stays what q, the output and dequant() have
        self.k = [torch.zeros(shape, dtype=store, device=self.device) for _ in range(self.num_layers)]
        self.v = [torch.zeros(shape, dtype=store, device=self.device) for _ in range(self.num_layers)]
        if self.quantized:  # zero scales: a slot never written dequantises to 0
            self.k_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=self.device)
                            for _ in range(self.num_layers)]
            self.v_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=self.device)
                            for _ in range(self.num_layers)]
        self.lens = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self._bound = 0  # host-side upper bound of lens
        self._epoch = 0  # bumped by reset(): a captured decode graph of an earlier epoch is stale

    @property
    def bound(self) -> int:
        return self._bound

    @property
    def quantized(self) -> bool:
        return self.kv_dtype is not None

    @property
    def nbytes(self) -> int:
        """Bytes of key / value storage: the elements (codes) plus, when quantised, the scales."""
        ts = self.k + self.v + (self.k_scale + self.v_scale if self.quantized else [])
        return sum(t.numel() * t.element_size() for t in ts)

    def dequant(self, layer: int):
        """(k, v) of ``layer`` as ``[B, max_len, Hk, D]`` in ``dtype``: ``codes * scale`` (exact) of
        a quantised cache, the stored tensors otherwise."""
        if not self.quantized:
            return self.k[layer], self.v[layer]
        return (dequantize_kv_fp8(self.k[layer], self.k_scale[layer], self.dtype),
                dequantize_kv_fp8(self.v[layer], self.v_scale[layer], self.dtype))

    def reset(self):
        """Forget every cached token (the storage is kept)."""
        self.lens.zero_()
        self._bound = 0
        self._epoch += 1

    # the host mirror of lens, for a decode step that is captured (recorded, not run) and
    # replayed (run without its Python side): models/generation.py DecodeGraph
    def _mirror(self):
        return self._bound

    def _set_mirror(self, m):
        self._bound = int(m)

    def _advance_mirror(self, T: int = 1):
        self._bound += int(T)

    def check_room(self, T: int):
        if self._bound + int(T) > self.max_len:
            raise ValueError(f"KV cache overflow: {self._bound} cached + {int(T)} new tokens > max_len {self.max_len}")

    def advance(self, T: int = 1):
        """lens += T for every row (in place, on the stream: no host read)."""
        self.check_room(T)
        if self.lens.is_cuda:
            N.call("pa_i32_add", N.ptr(self.lens), self.batch, int(T), N.stream())
        else:
            self.lens += int(T)
        self._bound += int(T)

    def advance_each(self, new_lens):
        """lens[b] += new_lens[b] from a host list: the ragged advance after a right-padded
        chunk (no device read).  The host bound moves by the largest count; it raises when
        ``bound + max(new_lens)`` passes ``max_len`` -- the rule of ``check_room``, because the
        padding tokens of a short row are written too (and later overwritten)."""
        host = [int(x) for x in (new_lens.tolist() if torch.is_tensor(new_lens) else new_lens)]
        if len(host) != self.batch or min(host) < 0:
            raise ValueError(f"advance_each: need {self.batch} counts >= 0, got {host}")
        self.check_room(max(host))
        _add_rows(self.lens, host)
        self._bound += max(host)

    def rewind_each(self, counts, bound=None):
        """lens[b] -= counts[b] from a host list (counts >= 0): take the last tokens of each row
        back out, e.g. the rejected candidates of a speculative round (no device read).  The
        host knows only an upper bound of ``lens``, so the caller passes the new exact maximum
        as ``bound`` (it may only lower the bound); without it the bound stays where it is.
        The slots beyond ``lens`` keep their stale contents: every kernel masks by ``lens``,
        and the next append overwrites them."""
        host = [int(x) for x in (counts.tolist() if torch.is_tensor(counts) else counts)]
        if len(host) != self.batch or min(host) < 0 or max(host) > self._bound:
            raise ValueError(f"rewind_each: need {self.batch} counts in [0, {self._bound}], got {host}")
        if bound is not None and not 0 <= int(bound) <= self._bound:
            raise ValueError(f"rewind_each: bound must be in [0, {self._bound}], got {bound}")
        _add_rows(self.lens, [-n for n in host])
        if bound is not None:
            self._bound = int(bound)

    def set_lens(self, lens):
        """lens = the given per-row lengths (host list or tensor), e.g. the prompt lengths
        after a right-padded prefill; the host bound becomes their maximum."""
        host = [int(x) for x in (lens.tolist() if torch.is_tensor(lens) else lens)]
        if len(host) != self.batch or min(host) < 0 or max(host) > self.max_len:
            raise ValueError(f"set_lens: need {self.batch} lengths in [0, {self.max_len}], got {host}")
        self.lens.copy_(torch.tensor(host, dtype=torch.int32))
        self._bound = max(host)


def _add_rows(lens, host):
    """lens (int32, device or CPU) += the host list, on the current stream without a
    synchronising call (the staging buffer comes from torch's caching host allocator, which
    does not hand it out again before the copy has finished)."""
    inc = torch.tensor(host, dtype=torch.int32)
    if not lens.is_cuda:
        lens += inc
        return
    staging = torch.empty(inc.shape, dtype=torch.int32, pin_memory=True)
    staging.copy_(inc)
    dev = torch.empty_like(lens)
    dev.copy_(staging, non_blocking=True)
    N.call("pa_i32_add_rows", N.ptr(lens), N.ptr(dev), lens.numel(), N.stream())


def _rope_at(x, cos, sin, positions):
    """neox rotation of x [B, T, H, D] at table rows positions [B, T]:
    [a|b] -> [a*c - b*s, b*c + a*s] (``fused._rope_ref`` at a position offset)."""
    D = x.shape[-1]
    c = cos[positions].unsqueeze(2)
    s = sin[positions].unsqueeze(2)
    a, b = x[..., : D // 2].float(), x[..., D // 2:].float()
    return torch.cat([a * c - b * s, b * c + a * s], -1).to(x.dtype)


def _kv_append_ref(q4, cache, layer, Hq, Hk, cos, sin):
    B, T = q4.shape[:2]
    pos = cache.lens.long()
    positions = pos.unsqueeze(1) + torch.arange(T, device=q4.device)
    q, k, v = q4[:, :, :Hq], q4[:, :, Hq:Hq + Hk], q4[:, :, Hq + Hk:]
    if cos is not None:
        q, k = _rope_at(q, cos, sin, positions), _rope_at(k, cos, sin, positions)
    bidx = torch.arange(B, device=q4.device).unsqueeze(1).expand(B, T)
    _store_slots(cache, layer, (bidx, positions), k.to(cache.dtype), v.to(cache.dtype))
    return q.contiguous()


def _store_slots(cache, layer, index, k, v):
    """k / v [..., Hk, D] (what a cache in ``cache.dtype`` stores) into the slots ``index`` of
    the [slots..., Hk, D] storage of ``layer``: as they are, or quantised by the contract."""
    if not cache.quantized:
        cache.k[layer][index] = k
        cache.v[layer][index] = v
        return
    for x, codes, scales in ((k, cache.k[layer], cache.k_scale[layer]), (v, cache.v[layer], cache.v_scale[layer])):
        c, s = quantize_kv_fp8(x)
        codes.view(torch.uint8)[index] = c.view(torch.uint8)  # bytes: indexing is not defined on fp8
        scales[index] = s


def _aligned16(t):
    return t.data_ptr() % 16 == 0


def _append_kernel_ok(q4, cache, cos, sin):
    D = q4.shape[-1]
    if not (q4.is_cuda and q4.dtype == torch.bfloat16 and cache.dtype == torch.bfloat16 and D % 16 == 0):
        return False
    if cache.quantized and not N.lib().pa_kv_append_f8_ok(int(D)):
        return False
    if q4.stride(-1) != 1 or any(s % 8 for s in q4.stride()[:3]) or not _aligned16(q4):
        return False
    if cos is not None and not (cos.is_cuda and cos.dtype == torch.float32 and sin.dtype == torch.float32
                                and cos.is_contiguous() and sin.is_contiguous() and cos.shape[-1] == D // 2
                                and sin.shape == cos.shape):
        return False
    return True


@torch.no_grad()
def kv_append(qkv, cache, layer: int, num_heads: int, num_kv_heads: int | None = None, cos=None, sin=None,
              rows=None):
    """Write the T new tokens of a packed projection ``qkv`` [B, T, (Hq+2Hk)*D] into
    layer ``layer`` of ``cache`` at rows ``cache.lens[b] + t`` and return q [B, T, Hq, D].

    With ``cos`` / ``sin`` (the fp32 tables of ``rope_tables``) q and k are rotated at
    their true positions ``lens[b] + t``; v is always copied bit for bit.  ``lens`` is
    not advanced: call ``cache.advance(T)`` once after the last layer.  Raises
    ``ValueError`` when the host-side bound says the append would pass ``max_len`` (or
    the rotary table).

    ``rows`` (paged cache only): a host list that maps the input's batch rows onto cache
    rows, so that ``qkv`` [len(rows), T, ...] fills a subset of the cache's rows."""
    Hq, Hk = int(num_heads), int(num_kv_heads or num_heads)
    B, T, W = qkv.shape
    D = W // (Hq + 2 * Hk)
    paged = getattr(cache, "paged", False)
    if rows is not None and not paged:
        raise ValueError("kv_append: rows= needs a paged cache (a contiguous cache appends to every row)")
    if W != (Hq + 2 * Hk) * D or (B != cache.batch and not paged) or Hk != cache.num_kv_heads \
            or D != cache.head_dim:
        raise ValueError(f"kv_append: qkv {tuple(qkv.shape)} does not match the cache "
                         f"(B={cache.batch}, Hk={cache.num_kv_heads}, D={cache.head_dim}) with {Hq} heads")
    if (cos is None) != (sin is None):
        raise ValueError("kv_append: cos and sin go together")
    if paged:
        return _paged.kv_append_paged(qkv, cache, layer, Hq, Hk, cos, sin, rows)
    cache.check_room(T)
    if cos is not None and cache.bound + T > cos.shape[0]:
        raise ValueError(f"kv_append: position {cache.bound + T - 1} is beyond the rotary table ({cos.shape[0]} rows)")
    if qkv.stride(-1) != 1:
        qkv = qkv.contiguous()
    q4 = qkv.unflatten(-1, (Hq + 2 * Hk, D))  # a view: the last dim has unit stride
    if not _append_kernel_ok(q4, cache, cos, sin):
        return _kv_append_ref(q4, cache, layer, Hq, Hk, cos, sin)
    q = torch.empty(B, T, Hq, D, dtype=qkv.dtype, device=qkv.device)
    if cache.quantized:
        N.call("pa_kv_append_f8", N.ptr(q4), ctypes_long_array(_fa_strides(q4)), N.ptr(cache.lens), N.ptr(cos),
               N.ptr(sin), int(cos.shape[0]) if cos is not None else 0, N.ptr(cache.k[layer]), N.ptr(cache.v[layer]),
               N.ptr(cache.k_scale[layer]), N.ptr(cache.v_scale[layer]), cache.max_len, N.ptr(q), B, T, Hq, Hk, D,
               N.stream())
        return q
    N.call("pa_kv_append", N.ptr(q4), ctypes_long_array(_fa_strides(q4)), N.ptr(cache.lens), N.ptr(cos), N.ptr(sin),
           int(cos.shape[0]) if cos is not None else 0, N.ptr(cache.k[layer]), N.ptr(cache.v[layer]), cache.max_len,
           N.ptr(q), B, T, Hq, Hk, D, N.stream())
    return q


def _decode_attention_ref(q, k, v, kv_len, scale):
    """fp32 attention of one query token per row over the first kv_len[b] cached keys
    (``fused._attn_ref`` per row; a row with no key gives zeros)."""
    outs = []
    for b, n in enumerate(kv_len.tolist()):
        if n <= 0:
            outs.append(torch.zeros_like(q[b:b + 1]))
        else:
            outs.append(_attn_ref(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], False, scale))
    return torch.cat(outs, 0)


def default_num_splits(batch: int, num_kv_heads: int, max_len: int) -> int:
    """The split count the host picks from the launch shape alone (never from the
    lengths): enough workgroups for two per compute unit, at least 256 keys per split."""
    return int(N.lib().pa_attn_decode_splits(int(batch), int(num_kv_heads), int(max_len)))


@torch.no_grad()
def decode_attention(q, cache, layer: int, scale: float | None = None, num_splits: int | None = None,
                     kv_len=None):
    """Attention of one new token per row, q [B, 1, Hq, D], over layer ``layer`` of the
    cache.  Row b attends to its first ``kv_len[b]`` cached tokens; ``kv_len`` defaults
    to ``cache.lens + 1`` -- the token ``kv_append`` has just written, before
    ``cache.advance()``.  Returns o [B, 1, Hq, D].

    On the GPU (bf16, D in {64, 128}, Hq/Hk in {1, 2, 4, 8}) the key axis is cut into
    ``num_splits`` ranges that run as separate workgroups and are merged by a second
    kernel; the result is bit-identical from run to run for a given ``num_splits``.  A
    quantised cache runs the e4m3 instantiation of the same kernel (the bits of the bf16 one
    over ``cache.dequant(layer)``); elsewhere it is the reference over ``cache.dequant(layer)``."""
    B, Tq, Hq, D = q.shape
    if Tq != 1 or B != cache.batch or D != cache.head_dim:
        raise ValueError(f"decode_attention: q {tuple(q.shape)} does not match the cache")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    _check_scale(scale, "decode_attention")
    if kv_len is None:
        kv_len = cache.lens + 1
    if getattr(cache, "paged", False):
        return _paged.decode_attention_paged(q, cache, layer, float(scale), num_splits, kv_len)
    k, v = cache.k[layer], cache.v[layer]
    Hk, S_max = cache.num_kv_heads, cache.max_len
    if q.is_cuda and q.dtype == torch.bfloat16 and cache.dtype == torch.bfloat16 and q.stride(-1) == 1 \
            and _aligned16(q) and kv_len.is_cuda and kv_len.dtype == torch.int32 and kv_len.is_contiguous():
        ns = default_num_splits(B, Hk, S_max) if num_splits is None else int(num_splits)
        qst = ctypes_long_array([q.stride(0), q.stride(2)])
        if cache.quantized:
            if N.lib().pa_attn_decode_f8_ok(B, S_max, Hq, Hk, D, ns, qst):
                o = torch.empty(B, 1, Hq, D, dtype=q.dtype, device=q.device)
                ws = torch.empty(B * Hq * ns * (D + 2), dtype=torch.float32, device=q.device)
                N.call("pa_attn_decode_f8", N.ptr(q), qst, N.ptr(k), N.ptr(v), N.ptr(cache.k_scale[layer]),
                       N.ptr(cache.v_scale[layer]), N.ptr(kv_len), N.ptr(o), N.ptr(ws), B, S_max, Hq, Hk, D,
                       float(scale), ns, N.stream())
                return o
        elif N.lib().pa_attn_decode_ok(B, S_max, Hq, Hk, D, ns, qst):
            o = torch.empty(B, 1, Hq, D, dtype=q.dtype, device=q.device)
            ws = torch.empty(B * Hq * ns * (D + 2), dtype=torch.float32, device=q.device)
            N.call("pa_attn_decode", N.ptr(q), qst, N.ptr(k), N.ptr(v), N.ptr(kv_len), N.ptr(o), N.ptr(ws),
                   B, S_max, Hq, Hk, D, float(scale), ns, N.stream())
            return o
    k, v = cache.dequant(layer)
    return _decode_attention_ref(q, k, v, kv_len, float(scale))


def _extend_attention_ref(q, k, v, base_len, scale):
    """fp32 attention of T query tokens per row over the cached keys: token t of row b sees
    the keys n < min(max(base_len[b], 0) + t + 1, S_max) (``fused._attn_ref`` per row, causal
    inside the chunk)."""
    T, S_max = q.shape[1], k.shape[1]
    outs = []
    for b, n in enumerate(base_len.tolist()):
        n = max(int(n), 0)
        if n + T <= S_max:
            outs.append(_attn_ref(q[b:b + 1], k[b:b + 1, :n + T], v[b:b + 1, :n + T], True, scale))
        else:  # the end of the cache cuts the chunk: token by token
            outs.append(torch.cat([_attn_ref(q[b:b + 1, t:t + 1], k[b:b + 1, :min(n + t + 1, S_max)],
                                             v[b:b + 1, :min(n + t + 1, S_max)], False, scale)
                                   for t in range(T)], 1))
    return torch.cat(outs, 0)


def default_extend_splits(batch: int, num_kv_heads: int, T: int, max_len: int) -> int:
    """The split count ``extend_attention`` picks from the launch shape alone (never from the
    lengths), for either cache layout."""
    return int(N.lib().pa_attn_extend_splits(int(batch), int(num_kv_heads), int(T), int(max_len)))


def _extend_kernel(q, cache, layer, scale, num_splits, base_len, rows_t, out=None):
    """Launch pa_attn_extend when it takes the problem; None otherwise.  ``out``: a contiguous
    [B, T, Hq, D] buffer to write (the tests border it with a sentinel)."""
    B, T, Hq, D = q.shape
    Hk, S_max = cache.num_kv_heads, cache.max_len
    paged = getattr(cache, "paged", False)
    if not (q.is_cuda and q.dtype == torch.bfloat16 and cache.dtype == torch.bfloat16 and q.stride(-1) == 1
            and _aligned16(q) and base_len.is_cuda and base_len.dtype == torch.int32 and base_len.is_contiguous()
            and Hk > 0 and Hq % Hk == 0):
        return None
    ns = default_extend_splits(B, Hk, T, S_max) if num_splits is None else int(num_splits)
    qst = ctypes_long_array(_fa_strides(q))
    geom = (cache.block_size, cache.max_blocks, cache.num_blocks) if paged else (0, 0, 0)
    if not N.lib().pa_attn_extend_ok(B, T, S_max, Hq, Hk, D, ns, qst, *geom):
        return None
    o = torch.empty(B, T, Hq, D, dtype=q.dtype, device=q.device) if out is None else out
    ws = torch.empty(B * T * Hq * ns * (D + 2), dtype=torch.float32, device=q.device) if ns > 1 else None
    ksc = cache.k_scale[layer] if cache.quantized else None
    vsc = cache.v_scale[layer] if cache.quantized else None
    N.call("pa_attn_extend", N.ptr(q), qst, N.ptr(cache.k[layer]), N.ptr(cache.v[layer]), N.ptr(ksc), N.ptr(vsc),
           N.ptr(cache.block_table) if paged else None, geom[1], geom[2], geom[0], N.ptr(rows_t), N.ptr(base_len),
           N.ptr(o), N.ptr(ws), B, cache.batch, T, S_max, Hq, Hk, D, float(scale), ns, N.stream())
    return o


@torch.no_grad()
def extend_attention(q, cache, layer: int, scale: float | None = None, num_splits: int | None = None,
                     base_len=None, rows=None):
    """Attention of T new tokens per row, q [B, T, Hq, D] (what ``kv_append`` returns), over
    layer ``layer`` of either cache.  Token t of row b attends to the cached keys
    ``n < min(max(base_len[b], 0) + t + 1, max_len)``: the row's earlier tokens plus the chunk
    itself up to t.  The chunk is already in the cache -- ``kv_append`` ran first and the
    lengths have not advanced -- so ``base_len`` defaults to ``cache.lens``.  Returns o
    [B, T, Hq, D].

    ``rows`` (paged cache only, the rule and the error of ``kv_append``): q row i reads cache
    row ``rows[i]``; inside ``cache.prefilling(rows)`` the mapping comes from the scope.  An
    explicit ``base_len`` is indexed by q row.

    On the GPU (bf16 q, D in {64, 128}, Hq/Hk in {1, 2, 4, 8}) this is ``pa_attn_extend`` of
    ``csrc/kernels/attn_extend.hip``: both products on the bf16 MFMA, the key range cut into
    ``num_splits`` ranges (``default_extend_splits``: from the launch shape only), bit-identical
    from run to run.  The paged instantiation returns the bits of the contiguous one for equal
    tokens, ``base_len`` and ``num_splits``; the e4m3 one the bits of the bf16 one over
    ``cache.dequant(layer)``.  At T = 1 it is *not* bit-equal to ``decode_attention`` (different
    arithmetic), and different chunkings of the same tokens are not bit-equal to each other.
    CPU tensors, other dtypes, other shapes and a misaligned q run the plain-torch reference
    over ``cache.dequant(layer)``."""
    if q.dim() != 4:
        raise ValueError(f"extend_attention: q must be [B, T, Hq, D], got {tuple(q.shape)}")
    B, T, Hq, D = q.shape
    paged = getattr(cache, "paged", False)
    if rows is not None and not paged:
        raise ValueError("extend_attention: rows= needs a paged cache (a contiguous cache has every row)")
    rows_t = None
    nrows = cache.batch
    if paged:
        if cache._in_prefill:
            if rows is not None:
                raise ValueError("extend_attention: rows= inside PagedKVCache.prefilling() (the scope maps the rows)")
            rows_t = cache._prefill_rows
        elif rows is not None:
            rows_t = cache._index_tensor(cache._check_rows(rows))
        if rows_t is not None:
            nrows = rows_t.numel()
    Hk = cache.num_kv_heads
    if T < 1 or B != nrows or D != cache.head_dim or Hq % Hk:
        raise ValueError(f"extend_attention: q {tuple(q.shape)} does not match the cache "
                         f"({nrows} rows, Hk={Hk}, D={cache.head_dim})")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    _check_scale(scale, "extend_attention")
    if base_len is None:
        base_len = cache.lens if rows_t is None else cache.lens.index_select(0, rows_t.long()).contiguous()
    elif base_len.numel() != B:
        raise ValueError(f"extend_attention: base_len has {base_len.numel()} entries for {B} q rows")
    o = _extend_kernel(q, cache, layer, float(scale), num_splits, base_len, rows_t)
    if o is not None:
        return o
    k, v = cache.dequant(layer)
    if rows_t is not None:
        k, v = k.index_select(0, rows_t.long()), v.index_select(0, rows_t.long())
    return _extend_attention_ref(q, k, v, base_len, float(scale))


from . import paged as _paged  # noqa: E402  (paged.py uses the helpers above)
from .paged import PagedKVCache  # noqa: E402,F401
