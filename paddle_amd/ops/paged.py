"""Paged KV cache: tokens live in fixed-size blocks drawn from one pool shared by all rows.

Layout: per layer ``k[l]`` / ``v[l]`` ``[num_blocks, block_size, Hk, D]`` (a block is
token-major like the contiguous slab, so an append is still a row copy), one int32 device
``block_table [B, max_blocks]`` (``-1``: no block) and one int32 device ``lens[B]``, both
shared by all layers.  Token ``n`` of row ``b`` is at
``pool[block_table[b][n // block_size]][n % block_size]``.

The host owns the bookkeeping: an exact mirror of ``lens``, a mirror of the table and a
LIFO free list.  No method reads the device; the table is uploaded only in the steps
that changed it.  ``ops.kv_append`` and ``ops.decode_attention`` dispatch here for a
``PagedKVCache`` (``pa_kv_append_paged`` / ``pa_attn_decode_paged`` of
``csrc/kernels/attn_decode.hip`` on the GPU in bf16, plain torch otherwise).

``kv_dtype="fp8_e4m3"``: the pool holds e4m3 codes and a second pool ``k_scale[l]`` /
``v_scale[l]`` ``[num_blocks, block_size, Hk]`` the fp32 scales, addressed through the same
table (:mod:`paddle_amd.ops.kv_fp8`; ``pa_kv_append_paged_f8`` / ``pa_attn_decode_paged_f8``).
The bookkeeping below does not know about the storage type.
"""
from __future__ import annotations

import contextlib

import torch

from . import _native as N
from . import decode as _D
from .fused import _fa_strides, ctypes_long_array
from .kv_fp8 import _FP8, check_kv_dtype, dequantize_kv_fp8

__all__ = ["PagedKVCache", "BLOCK_SIZES", "DEFAULT_BLOCK_SIZE"]

BLOCK_SIZES = (16, 32, 64, 128, 256)
# Measured (benchmarks/paged_decode_bench.py, profiles/paged_decode_bench.md): no block size
# is within the contiguous kernel's run-to-run spread at every 8192-token shape; this one is
# the fastest (at worst 5.5 % behind the contiguous kernel, the others 5.9-6.8 %).
DEFAULT_BLOCK_SIZE = 64


def _host_ints(x):
    return [int(v) for v in (x.tolist() if torch.is_tensor(x) else x)]


class PagedKVCache:
    """Block-table key / value storage for incremental decoding (see the module docstring).

    The interface of :class:`KVCache` (``reset``, ``check_room``, ``advance``, ``set_lens``,
    ``bound``, ``lens``, ...) plus ``reserve``, ``free_rows`` and ``gather``.  ``check_room``
    also reserves, so ``decode_step`` and a hand-written ``kv_append`` loop run unchanged.
    When the pool cannot cover a reservation, ``ValueError`` is raised before any launch and
    nothing has changed."""

    paged = True

    def __init__(self, num_layers, batch, max_len, num_kv_heads, head_dim, dtype=torch.bfloat16, device=None,
                 block_size=None, num_blocks=None, zero_fill=True, kv_dtype=None):
        self.kv_dtype = check_kv_dtype(kv_dtype)
        block_size = DEFAULT_BLOCK_SIZE if block_size is None else int(block_size)
        if block_size not in BLOCK_SIZES:
            raise ValueError(f"block_size must be one of {BLOCK_SIZES}, got {block_size}")
        self.num_layers, self.batch, self.max_len = int(num_layers), int(batch), int(max_len)
        self.num_kv_heads, self.head_dim = int(num_kv_heads), int(head_dim)
        self.dtype, self.device = dtype, torch.device(device if device is not None else "cpu")
        self.block_size = block_size
        self.max_blocks = -(-self.max_len // block_size)
        self.num_blocks = self.batch * self.max_blocks if num_blocks is None else int(num_blocks)
        if self.batch < 1 or self.max_len < 1 or self.num_blocks < 1:
            raise ValueError(f"PagedKVCache: need batch, max_len and num_blocks >= 1, got {self.batch}, "
                             f"{self.max_len}, {self.num_blocks}")
        # one backing allocation, per-layer views
        alloc = torch.zeros if zero_fill else torch.empty
        self._pool = alloc((2, self.num_layers, self.num_blocks, block_size, self.num_kv_heads, self.head_dim),
                           dtype=_FP8 if self.quantized else dtype, device=self.device)
        self.k = [self._pool[0, i] for i in range(self.num_layers)]
        self.v = [self._pool[1, i] for i in range(self.num_layers)]
        if self.quantized:  # always zero: a slot never written dequantises to 0
            self._scale_pool = torch.zeros((2, self.num_layers, self.num_blocks, block_size, self.num_kv_heads),
                                           dtype=torch.float32, device=self.device)
            self.k_scale = [self._scale_pool[0, i] for i in range(self.num_layers)]
            self.v_scale = [self._scale_pool[1, i] for i in range(self.num_layers)]
        self.lens = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.block_table = torch.full((self.batch, self.max_blocks), -1, dtype=torch.int32, device=self.device)
        # host state
        self._lens = [0] * self.batch                                  # exact mirror of lens
        self._table = torch.full((self.batch, self.max_blocks), -1, dtype=torch.int32)  # mirror of block_table
        self._owned = [[] for _ in range(self.batch)]                  # block ids per row, in token order
        self._free = list(range(self.num_blocks - 1, -1, -1))          # LIFO: pop() hands out 0, 1, 2, ...
        self._prefill_rows = None  # set inside prefilling(): kv_append maps rows and reserves nothing
        self._in_prefill = False
        self._slack = None  # cached: tokens every row can still take in the blocks it owns
        self._bound = None  # cached: max of _lens
        self._epoch = 0  # bumped when rows lose their blocks: a captured decode graph is stale then

    # ------------------------------------------------------------------ host views
    @property
    def bound(self) -> int:
        if self._bound is None:
            self._bound = max(self._lens)
        return self._bound

    @property
    def quantized(self) -> bool:
        return self.kv_dtype is not None

    @property
    def nbytes(self) -> int:
        """Bytes of key / value storage: the pool plus, when quantised, the scales."""
        ts = [self._pool] + ([self._scale_pool] if self.quantized else [])
        return sum(t.numel() * t.element_size() for t in ts)

    def _changed(self):
        """The lengths or the ownership changed: drop what was derived from them."""
        self._slack = self._bound = None

    # the host mirror of lens, for a decode step that is captured (recorded, not run) and
    # replayed (run without its Python side): models/generation.py DecodeGraph
    def _mirror(self):
        return list(self._lens)

    def _set_mirror(self, m):
        self._lens = [int(n) for n in m]
        self._changed()

    def _advance_mirror(self, T: int = 1):
        self._lens = [n + int(T) for n in self._lens]
        self._changed()

    @property
    def host_lens(self):
        """The host's exact copy of ``lens`` (a new list)."""
        return list(self._lens)

    @property
    def host_table(self):
        """The host's copy of ``block_table`` (a new int32 CPU tensor)."""
        return self._table.clone()

    @property
    def blocks_free(self) -> int:
        return len(self._free)

    @property
    def blocks_used(self) -> int:
        return self.num_blocks - len(self._free)

    @property
    def free_blocks(self):
        """The free list (a new list); the last entry is handed out next."""
        return list(self._free)

    def row_blocks(self, row: int):
        """The block ids row ``row`` owns, in token order."""
        return list(self._owned[row])

    # ------------------------------------------------------------------ uploads
    def _upload(self, dst, host):
        """dst (device) = host (CPU tensor) on the current stream, without a synchronising
        call.  Staging: a fresh pinned buffer per upload.  It comes from torch's caching
        host allocator, which records the copy's stream on the buffer and does not hand the
        memory out again before that copy has finished, so the next step's upload can never
        rewrite a buffer still in flight."""
        if dst.is_cuda:
            staging = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
            staging.copy_(host)
            dst.copy_(staging, non_blocking=True)
        else:
            dst.copy_(host)

    def _upload_table(self):
        self._upload(self.block_table, self._table)

    def _upload_lens(self):
        self._upload(self.lens, torch.tensor(self._lens, dtype=torch.int32))

    def _index_tensor(self, rows):
        t = torch.empty(len(rows), dtype=torch.int32, device=self.device)
        self._upload(t, torch.tensor(rows, dtype=torch.int32))
        return t

    # ------------------------------------------------------------------ allocator
    def _check_rows(self, rows):
        rows = list(range(self.batch)) if rows is None else _host_ints(rows)
        if not rows or len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= self.batch:
            raise ValueError(f"rows must be distinct values in [0, {self.batch}), got {rows}")
        return rows

    def reserve(self, new_lens, rows=None):
        """Give every row (or each of ``rows``) the blocks to hold ``lens[b] + T`` tokens
        (``new_lens`` an int T) or the given per-row lengths (a list / tensor of host
        values).  Never shrinks a row.  Raises ``ValueError``, with nothing changed, when a
        length passes ``max_len`` or the pool runs out."""
        if rows is None and isinstance(new_lens, int) and new_lens >= 0:
            # the common call, once per layer and step: every row still has room in its blocks
            if self._slack is None:
                self._slack = min(len(o) * self.block_size - n for o, n in zip(self._owned, self._lens))
            if new_lens <= self._slack and self.bound + new_lens <= self.max_len:
                return
        rows = self._check_rows(rows)
        if isinstance(new_lens, int):
            want = [self._lens[r] + new_lens for r in rows]
        else:
            want = _host_ints(new_lens)
            if len(want) != len(rows):
                raise ValueError(f"reserve: need {len(rows)} lengths, got {want}")
        if min(want) < 0 or max(want) > self.max_len:
            raise ValueError(f"KV cache overflow: lengths {want} are not in [0, max_len = {self.max_len}]")
        extra = [max(0, -(-w // self.block_size) - len(self._owned[r])) for r, w in zip(rows, want)]
        if sum(extra) > len(self._free):
            raise ValueError(f"paged KV cache: out of blocks ({sum(extra)} more needed, {len(self._free)} free of "
                             f"{self.num_blocks}, block_size {self.block_size})")
        if not any(extra):
            return
        for r, n in zip(rows, extra):
            for _ in range(n):
                blk = self._free.pop()
                self._table[r, len(self._owned[r])] = blk
                self._owned[r].append(blk)
        self._changed()
        self._upload_table()

    def check_room(self, T: int, rows=None):
        """Raise when ``T`` more tokens would pass ``max_len`` (or the pool); otherwise
        make sure every row has the blocks for them."""
        if self._in_prefill:
            return  # prefill has reserved each row's own length already
        self.reserve(int(T), rows)

    def free_rows(self, rows):
        """Return the rows' blocks to the pool; their table entries become -1 and their
        lengths 0.  Every other row is untouched."""
        rows = self._check_rows(rows)
        for r in rows:
            self._free.extend(reversed(self._owned[r]))  # the next reservation gets them back in order
            self._owned[r] = []
            self._table[r].fill_(-1)
            self._lens[r] = 0
        self._changed()
        self._epoch += 1
        self._upload_table()
        self._upload_lens()

    def reset(self):
        """Forget every cached token and return every block: the state of a new cache (the
        pool's contents are kept)."""
        self._free = list(range(self.num_blocks - 1, -1, -1))
        self._owned = [[] for _ in range(self.batch)]
        self._table.fill_(-1)
        self._lens = [0] * self.batch
        self._changed()
        self._epoch += 1
        self.block_table.fill_(-1)
        self.lens.zero_()

    def advance(self, T: int = 1):
        """lens += T for every row (in place, on the stream: no host read)."""
        self.check_room(T)
        if self.lens.is_cuda:
            N.call("pa_i32_add", N.ptr(self.lens), self.batch, int(T), N.stream())
        else:
            self.lens += int(T)
        self._lens = [n + int(T) for n in self._lens]
        self._changed()

    def advance_each(self, new_lens, rows=None):
        """lens[b] += new_lens[b] from a host list, for every row or for ``rows`` only: the
        ragged advance after a right-padded chunk (no device read).  Each row's
        ``lens[b] + new_lens[b]`` is reserved first: when the pool (or ``max_len``) is short,
        ``ValueError`` is raised before any launch and nothing has changed."""
        rows = self._check_rows(rows)
        host = _host_ints(new_lens)
        if len(host) != len(rows) or min(host) < 0:
            raise ValueError(f"advance_each: need {len(rows)} counts >= 0, got {host}")
        self.reserve([self._lens[r] + n for r, n in zip(rows, host)], rows)
        inc = [0] * self.batch
        for r, n in zip(rows, host):
            inc[r] = n
        _D._add_rows(self.lens, inc)
        for r, n in zip(rows, host):
            self._lens[r] += n
        self._changed()

    def rewind_each(self, counts, rows=None):
        """lens[b] -= counts[b] from a host list (counts >= 0), for every row or for ``rows``
        only: take the last tokens of a row back out, e.g. the rejected candidates of a
        speculative round (no device read).  The rows keep their blocks (the next tokens
        reuse them) and the table is neither touched nor uploaded; the slots beyond ``lens``
        keep their stale contents, which every kernel masks by ``lens`` and the next append
        overwrites.  A count above the row's length raises ``ValueError`` with nothing changed."""
        rows = self._check_rows(rows)
        host = _host_ints(counts)
        if len(host) != len(rows) or min(host) < 0:
            raise ValueError(f"rewind_each: need {len(rows)} counts >= 0, got {host}")
        for r, n in zip(rows, host):
            if n > self._lens[r]:
                raise ValueError(f"rewind_each: row {r} holds {self._lens[r]} tokens, cannot take back {n}")
        dec = [0] * self.batch
        for r, n in zip(rows, host):
            dec[r] = -n
        _D._add_rows(self.lens, dec)
        for r, n in zip(rows, host):
            self._lens[r] -= n
        self._changed()

    def set_lens(self, lens, rows=None):
        """lens = the given lengths (host list or tensor) for every row, or for ``rows``
        only.  Each row must already own the blocks for its length (``reserve``)."""
        rows = self._check_rows(rows)
        host = _host_ints(lens)
        if len(host) != len(rows) or min(host) < 0 or max(host) > self.max_len:
            raise ValueError(f"set_lens: need {len(rows)} lengths in [0, {self.max_len}], got {host}")
        for r, n in zip(rows, host):
            if n > len(self._owned[r]) * self.block_size:
                raise ValueError(f"set_lens: row {r} has blocks for {len(self._owned[r]) * self.block_size} tokens, "
                                 f"not {n}: reserve first")
        for r, n in zip(rows, host):
            self._lens[r] = n
        self._changed()
        self._upload_lens()

    def load_block_table(self, table):
        """Adopt an explicit assignment: ``table`` [B, max_blocks] of block ids, each row a
        run of distinct ids followed by -1.  For restoring a snapshot and for tests and
        benchmarks that want a particular (e.g. shuffled) placement.  Lengths become 0;
        the free list holds the remaining ids, lowest handed out first."""
        t = torch.as_tensor(table, dtype=torch.int32).cpu().reshape(self.batch, self.max_blocks)
        owned, seen = [], set()
        for r in range(self.batch):
            ids = t[r].tolist()
            n = next((i for i, x in enumerate(ids) if x < 0), len(ids))
            if any(x >= 0 for x in ids[n:]) or any(x >= self.num_blocks or x in seen for x in ids[:n]) \
                    or len(set(ids[:n])) != n:
                raise ValueError(f"load_block_table: row {r} is not a run of distinct free block ids then -1: {ids}")
            seen.update(ids[:n])
            owned.append(ids[:n])
        self._owned = owned
        self._table = torch.where(t < 0, torch.full_like(t, -1), t).contiguous()
        self._free = [b for b in range(self.num_blocks - 1, -1, -1) if b not in seen]
        self._lens = [0] * self.batch
        self._changed()
        self._epoch += 1
        self._upload_table()
        self._upload_lens()

    @contextlib.contextmanager
    def prefilling(self, rows=None):
        """Inside: ``kv_append`` writes input row i to cache row ``rows[i]`` (default: the
        identity) and reserves nothing -- the caller has reserved each row's own prompt
        length, and padding beyond a row's blocks is dropped by the kernel."""
        if self._in_prefill:
            raise RuntimeError("PagedKVCache.prefilling() does not nest")
        self._prefill_rows = None if rows is None else self._index_tensor(self._check_rows(rows))
        self._in_prefill = True
        try:
            yield self
        finally:
            self._in_prefill = False
            self._prefill_rows = None

    # ------------------------------------------------------------------ reference view
    def gather(self, layer: int):
        """(k, v) of ``layer`` as ``[B, max_len, Hk, D]``, zeros where no block is assigned
        (plain torch over the device table; what the reference paths and the tests read).
        A quantised cache returns the dequantised values in ``dtype``."""
        t = self.block_table.long()
        ok = (t >= 0) & (t < self.num_blocks)
        idx = torch.where(ok, t, torch.zeros_like(t))
        outs = []
        for n, pool in enumerate((self.k[layer], self.v[layer])):
            if self.quantized:  # bytes: indexing is not defined on fp8
                scales = (self.k_scale, self.v_scale)[n][layer]
                g = dequantize_kv_fp8(pool.view(torch.uint8)[idx].view(_FP8), scales[idx], self.dtype)
            else:
                g = pool[idx]  # [B, max_blocks, bs, Hk, D]
            g = torch.where(ok[:, :, None, None, None], g, torch.zeros((), dtype=g.dtype, device=g.device))
            outs.append(g.reshape(self.batch, self.max_blocks * self.block_size, self.num_kv_heads,
                                  self.head_dim)[:, :self.max_len])
        return outs[0], outs[1]

    def dequant(self, layer: int):
        """(k, v) of ``layer`` as ``[B, max_len, Hk, D]`` in ``dtype``, through the table: what
        ``gather`` returns."""
        return self.gather(layer)


# ---------------------------------------------------------------------- kv_append
def _kv_append_paged_ref(q4, cache, layer, Hq, Hk, cos, sin, rows_t):
    """Index arithmetic on the pool: the definition pa_kv_append_paged is tested against."""
    B, T = q4.shape[:2]
    dev = q4.device
    crow = torch.arange(B, device=dev) if rows_t is None else rows_t.long()
    positions = cache.lens.long()[crow].unsqueeze(1) + torch.arange(T, device=dev)  # [B, T]
    q, k, v = q4[:, :, :Hq], q4[:, :, Hq:Hq + Hk], q4[:, :, Hq + Hk:]
    ok = positions < cache.max_len
    if cos is not None:
        ok = ok & (positions < cos.shape[0])
        safe = positions.clamp(max=cos.shape[0] - 1)
        q, k = _D._rope_at(q, cos, sin, safe), _D._rope_at(k, cos, sin, safe)
    q = torch.where(ok[:, :, None, None], q, torch.zeros((), dtype=q.dtype, device=dev))  # no position: zeros
    bs = cache.block_size
    bidx = (positions // bs).clamp(max=cache.max_blocks - 1)
    blk = cache.block_table.long()[crow.unsqueeze(1).expand(B, T), bidx]
    ok = ok & (blk >= 0) & (blk < cache.num_blocks)
    slot = (blk * bs + positions % bs)[ok]  # dropped tokens leave no slot
    _D._store_slots(_FlatPool(cache), layer, slot, k[ok].to(cache.dtype), v[ok].to(cache.dtype))
    return q.contiguous()


class _FlatPool:
    """A paged cache's storage as [num_blocks * block_size, Hk, ...] views, for ``_store_slots``."""

    def __init__(self, cache):
        Hk, D = cache.num_kv_heads, cache.head_dim
        self.quantized = cache.quantized
        self.k = [t.view(-1, Hk, D) for t in cache.k]
        self.v = [t.view(-1, Hk, D) for t in cache.v]
        if cache.quantized:
            self.k_scale = [t.view(-1, Hk) for t in cache.k_scale]
            self.v_scale = [t.view(-1, Hk) for t in cache.v_scale]


def kv_append_paged(qkv, cache: PagedKVCache, layer, Hq, Hk, cos, sin, rows):
    """``ops.kv_append`` for a paged cache (shapes already parsed by the caller)."""
    B, T, W = qkv.shape
    D = cache.head_dim
    if cache._in_prefill:
        if rows is not None:
            raise ValueError("kv_append: rows= inside PagedKVCache.prefilling() (the scope maps the rows)")
        rows_t = cache._prefill_rows
        nrows = cache.batch if rows_t is None else rows_t.numel()
        rows_h = None
    else:
        rows_h = None if rows is None else cache._check_rows(rows)
        rows_t = None if rows_h is None else cache._index_tensor(rows_h)
        nrows = cache.batch if rows_h is None else len(rows_h)
    if B != nrows:
        raise ValueError(f"kv_append: qkv has {B} rows for {nrows} cache rows")
    cache.check_room(T, rows_h)
    if cos is not None and not cache._in_prefill:
        top = (cache.bound if rows_h is None else max(cache._lens[r] for r in rows_h)) + T
        if top > cos.shape[0]:
            raise ValueError(f"kv_append: position {top - 1} is beyond the rotary table ({cos.shape[0]} rows)")
    if qkv.stride(-1) != 1:
        qkv = qkv.contiguous()
    q4 = qkv.unflatten(-1, (Hq + 2 * Hk, D))
    if not _D._append_kernel_ok(q4, cache, cos, sin):
        return _kv_append_paged_ref(q4, cache, layer, Hq, Hk, cos, sin, rows_t)
    q = torch.empty(B, T, Hq, D, dtype=qkv.dtype, device=qkv.device)
    if cache.quantized:
        N.call("pa_kv_append_paged_f8", N.ptr(q4), ctypes_long_array(_fa_strides(q4)), N.ptr(cache.lens),
               N.ptr(rows_t), N.ptr(cos), N.ptr(sin), int(cos.shape[0]) if cos is not None else 0,
               N.ptr(cache.k[layer]), N.ptr(cache.v[layer]), N.ptr(cache.k_scale[layer]), N.ptr(cache.v_scale[layer]),
               N.ptr(cache.block_table), cache.max_blocks, cache.num_blocks, cache.block_size, cache.max_len, N.ptr(q),
               B, cache.batch, T, Hq, Hk, D, N.stream())
        return q
    N.call("pa_kv_append_paged", N.ptr(q4), ctypes_long_array(_fa_strides(q4)), N.ptr(cache.lens), N.ptr(rows_t),
           N.ptr(cos), N.ptr(sin), int(cos.shape[0]) if cos is not None else 0, N.ptr(cache.k[layer]),
           N.ptr(cache.v[layer]), N.ptr(cache.block_table), cache.max_blocks, cache.num_blocks, cache.block_size,
           cache.max_len, N.ptr(q), B, cache.batch, T, Hq, Hk, D, N.stream())
    return q


# ---------------------------------------------------------------------- decode attention
def decode_attention_paged(q, cache: PagedKVCache, layer, scale, num_splits, kv_len):
    """``ops.decode_attention`` for a paged cache: for equal q, cached tokens, kv_len and
    num_splits the GPU kernel returns the bits of the contiguous one."""
    B, Tq, Hq, D = q.shape
    Hk, S_max = cache.num_kv_heads, cache.max_len
    if q.is_cuda and q.dtype == torch.bfloat16 and cache.dtype == torch.bfloat16 and q.stride(-1) == 1 \
            and _D._aligned16(q) and kv_len.is_cuda and kv_len.dtype == torch.int32 and kv_len.is_contiguous():
        ns = _D.default_num_splits(B, Hk, S_max) if num_splits is None else int(num_splits)
        qst = ctypes_long_array([q.stride(0), q.stride(2)])
        if cache.quantized:
            if N.lib().pa_attn_decode_paged_f8_ok(B, S_max, Hq, Hk, D, ns, qst, cache.block_size, cache.max_blocks,
                                                  cache.num_blocks):
                o = torch.empty(B, 1, Hq, D, dtype=q.dtype, device=q.device)
                ws = torch.empty(B * Hq * ns * (D + 2), dtype=torch.float32, device=q.device)
                N.call("pa_attn_decode_paged_f8", N.ptr(q), qst, N.ptr(cache.k[layer]), N.ptr(cache.v[layer]),
                       N.ptr(cache.k_scale[layer]), N.ptr(cache.v_scale[layer]), N.ptr(cache.block_table),
                       cache.max_blocks, cache.num_blocks, cache.block_size, N.ptr(kv_len), N.ptr(o), N.ptr(ws),
                       B, S_max, Hq, Hk, D, float(scale), ns, N.stream())
                return o
        elif N.lib().pa_attn_decode_paged_ok(B, S_max, Hq, Hk, D, ns, qst, cache.block_size, cache.max_blocks,
                                             cache.num_blocks):
            o = torch.empty(B, 1, Hq, D, dtype=q.dtype, device=q.device)
            ws = torch.empty(B * Hq * ns * (D + 2), dtype=torch.float32, device=q.device)
            N.call("pa_attn_decode_paged", N.ptr(q), qst, N.ptr(cache.k[layer]), N.ptr(cache.v[layer]),
                   N.ptr(cache.block_table), cache.max_blocks, cache.num_blocks, cache.block_size, N.ptr(kv_len),
                   N.ptr(o), N.ptr(ws), B, S_max, Hq, Hk, D, float(scale), ns, N.stream())
            return o
    k, v = cache.gather(layer)
    return _D._decode_attention_ref(q, k, v, kv_len, float(scale))
