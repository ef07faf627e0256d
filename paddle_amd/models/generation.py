"""Autoregressive text generation with a KV cache for the dense LM models.

``GenerationMixin`` gives a model ``init_cache`` / ``prefill`` / ``decode_step`` /
``generate``.  The model supplies two hooks:

  ``_prefill_hidden(input_ids, cache)``  the existing layer code over the whole
        (right-padded) prompt, which also fills the cache -> hidden states [B, S, H];
  ``_decode_hidden(tokens, cache)``      one new token per row against the cache
        -> hidden states [B, 1, H];

plus ``_lm_logits(y)`` for the LM head.  Prefill reuses the training kernels (under the
causal mask right padding cannot influence a valid position); a decode step runs
``ops.kv_append`` + ``ops.decode_attention`` per layer (``csrc/kernels/attn_decode.hip``).

Cache layout: see :mod:`paddle_amd.ops.decode` (one slab per layer, the default) and
:mod:`paddle_amd.ops.paged` (blocks from a shared pool: ``init_cache(..., paged=True)``,
``generate(..., cache="paged")``; ``prefill(..., rows=...)`` replaces single rows).  A
row's first decoded token overwrites the first padding slot of a short prompt: positions
are per row (``cache.lens``).

``extend`` feeds T more tokens per row on top of a filled cache -- a further turn, a chunk of
a long prompt, T candidates to score -- through a third hook,

  ``_extend_hidden(input_ids, cache)``   T new tokens per row at the row's own positions
        -> hidden states [B, T, H]: per layer norm -> QKV -> ``ops.kv_append`` ->
        ``ops.extend_attention`` (``csrc/kernels/attn_extend.hip``) -> the rest,

followed by one ragged ``cache.advance_each``.  ``prefill(chunk=C)`` /
``generate(prefill_chunk=C)`` run a prompt C columns at a time on it.

``generate(graph=True)`` samples with the device kernel of :mod:`paddle_amd.ops.sampling`
and replays one captured decode step (:class:`DecodeGraph`: step, sampler and ``advance``
in one HIP graph) instead of launching it from Python every token.

``kv_dtype="fp8_e4m3"`` (``init_cache`` / ``generate``) keeps either cache in e4m3 codes with
one power-of-two scale per (token, kv head): ops/kv_fp8.py.

``quantize_weights()`` turns the decoder layers' matrices into ``ops.Fp8Weight``s (e4m3 codes,
power-of-two column scales): decode steps run them on the fp8 weight-streaming kernel,
prefill on an exact dequantised image (ops/skinny_fp8.py).
"""
from __future__ import annotations

import math
import os

import torch

from .. import ops
from ..autograd import tape as _tape
from ..ops import _native as N
from ..ops import fused as F
from ..ops import gemm as _G
from ..ops.decode import KVCache
from ..ops.paged import DEFAULT_BLOCK_SIZE, PagedKVCache


@torch.no_grad()
def prefill_qkv_attention(y, w, bias, cos, sin, Hq, Hk):
    """QKV projection (+ rotary when ``cos`` is given) and causal attention over a whole
    prompt y [B, S, H], on the kernels the training forward uses.  Returns
    (packed, o): the packed, already-rotated q|k|v [B, S, (Hq+2Hk)*D] (what the cache
    stores) and the attention output [B, S, Hq*D]."""
    B, S, K = y.shape
    W = w.shape[1]
    nh = Hq + 2 * Hk
    D = W // nh
    scale = 1.0 / math.sqrt(D)
    if cos is not None and bias is None and F._qkv_rope_fused_ok(y, w, cos, Hq, Hk):
        # rotary in the projection GEMM's epilogue (as ops.qkv_rope_attention)
        T = B * S
        packed = torch.empty(T, W, dtype=y.dtype, device=y.device)
        _G.gemm_epi(_G.EPI_ROPE, F._c(y.reshape(T, K)), F._weight_t(w, T), T, W, K, out=packed, cos=cos, sin=sin,
                    rope_cols=(Hq + Hk) * D, rope_S=S)
        packed = packed.view(B, S, W)
    else:
        qkv = F._c(ops.linear(y, w, bias))
        if cos is None:
            packed = qkv
        elif qkv.is_cuda and qkv.dtype == torch.bfloat16 and D in (64, 128):
            packed = torch.empty_like(qkv)
            N.call("pa_rope", 1, 1, N.ptr(qkv), W, N.ptr(packed), W, N.ptr(cos), N.ptr(sin), None,
                   B, S, nh, Hq + Hk, D, 0, N.stream())
        else:
            x = qkv.view(B, S, nh, D)
            packed = torch.cat([F._rope_ref(x[:, :, :Hq + Hk], cos, sin), x[:, :, Hq + Hk:]], 2).view(B, S, W)
    p4 = packed.view(B, S, nh, D)
    q, k, v = p4[:, :, :Hq], p4[:, :, Hq:Hq + Hk], p4[:, :, Hq + Hk:]
    if packed.is_cuda and packed.dtype == torch.bfloat16 and D in (64, 128):
        o, _ = F._fa_fwd(q, k, v, True, scale)
    else:
        o = F._attn_ref(q, k, v, True, scale)
    return packed, o.reshape(B, S, Hq * D)


def filter_logits(logits, temperature=1.0, top_k=0, top_p=1.0):
    """The fp32 logits ``sample_next`` draws from: scaled by the temperature, with ``-inf``
    where top-k / top-p (nucleus) filtering drops a token."""
    logits = logits.float()
    if temperature != 1.0:
        logits = logits / max(float(temperature), 1e-6)
    V = logits.shape[-1]
    if top_k and 0 < int(top_k) < V:
        kth = logits.topk(int(top_k), -1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p < 1.0:
        sl, si = logits.sort(-1, descending=True)
        sp = torch.softmax(sl, -1)
        # drop a token when the mass before it already reaches top_p (the first always stays)
        drop = (sp.cumsum(-1) - sp) >= float(top_p)
        sl = sl.masked_fill(drop, float("-inf"))
        logits = torch.full_like(logits, float("-inf")).scatter(-1, si, sl)
    return logits


def sample_next(logits, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, generator=None):
    """Next token per row from logits [B, V] (fp32 math): greedy, or temperature /
    top-k / top-p (nucleus) sampling with ``generator`` driving the draws."""
    if not do_sample:
        return logits.float().argmax(-1)
    probs = torch.softmax(filter_logits(logits, temperature, top_k, top_p), -1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


def dense_weight(w, x):
    """A layer weight as the dense tensor the training / prefill kernels take: ``w`` itself,
    or for an ``ops.Fp8Weight`` a transient dequantised image in ``x``'s dtype (exact: see
    ops/skinny_fp8.py), which is inference only."""
    if not isinstance(w, ops.Fp8Weight):
        return w
    if torch.is_grad_enabled() or _tape.current() is not None:
        raise RuntimeError("a model with quantised weights is inference only: run it under torch.no_grad() "
                           "and without the autograd tape")
    return w.dequant(x.dtype)


def _quantized_state_error(*args, **kwargs):
    raise NotImplementedError("state_dict() / load_state_dict() of a model with quantised weights is not "
                              "implemented: load the bf16 checkpoint first, then call quantize_weights()")


class DecodeGraph:
    """One decode step -- ``embed(state.tok)`` -> layers -> logits -> ``ops.sample_step`` ->
    ``cache.advance`` -- captured once into a HIP graph and replayed by :meth:`step`.

    ``state`` is an ``ops.SamplerState`` whose ``tok`` holds the token to feed (seed it with one
    eager ``ops.sample_step`` on the prefill logits).  ``logits`` is the static [B, V] buffer
    of the last replay.  The object keeps the cache, the state and the graph's private memory
    pool alive.  The capture runs on one stream, so the graph is a linear chain of the
    launches of ``decode_step`` + ``sample_step``, with their split counts: a replay computes
    the bits of the launch loop.

    Capture records the launches without running them, but the Python side of the step runs,
    so the host mirrors of the cache lengths are put back after the capture and advanced by
    one per replay.  A paged cache reserves the blocks of ``steps`` more tokens per row before
    the capture (``ValueError`` with nothing changed when the pool is short): the block table
    is constant from then on, and no upload happens inside the capture or between replays.

    On the CPU (or any cache that is not on a GPU) there is no graph: :meth:`step` runs the
    same sequence eagerly on the same state."""

    def __init__(self, model, cache, state, steps=None, seed=0, do_sample=False, temperature=1.0, top_k=0,
                 top_p=1.0):
        model._check_generation_supported()
        if state.batch != cache.batch:
            raise ValueError(f"decode_graph: a state of {state.batch} rows for a cache of {cache.batch}")
        self.model, self.cache, self.state = model, cache, state
        self._sampling = (int(seed), bool(do_sample), float(temperature), int(top_k or 0), float(top_p))
        self._paged = getattr(cache, "paged", False)
        room = cache.max_len - cache.bound
        self.steps = min(state.max_new_tokens, room) if steps is None else int(steps)
        if self.steps < 1:
            raise ValueError(f"KV cache overflow: {cache.bound} cached + 1 new tokens > max_len {cache.max_len}")
        if self._paged:
            cache.reserve(self.steps)  # raises, with nothing changed, when the pool (or max_len) is short
        self._left = self.steps
        self._epoch = cache._epoch
        self.replays = 0
        self.graph = None
        self.logits = None
        if cache.lens.is_cuda:
            self._capture()

    def _body(self):
        logits = self.model.decode_step(self.state.tok, self.cache)
        ops.sample_step(logits, self.state, *self._sampling)
        return logits

    def _capture(self):
        model, cache, st = self.model, self.cache, self.state
        mirror = cache._mirror()
        # warm-up, eagerly and off the capture: everything the step creates on first use (code
        # objects, cached buffers) exists before the capture.  It leaves no trace: the keys and
        # values it writes land in the slots the first replay rewrites, lens and state stay.
        side = torch.cuda.Stream(device=cache.lens.device)
        side.wait_stream(torch.cuda.current_stream(cache.lens.device))
        with torch.cuda.stream(side):
            logits = model._lm_logits(model._decode_hidden(st.tok.reshape(-1, 1), cache).reshape(st.batch, -1))
            N.call("pa_i32_add", N.ptr(cache.lens), cache.batch, 0, N.stream())
            ops.sample_tokens(logits, *self._sampling[:1], st.step, *self._sampling[1:])
            del logits
        torch.cuda.current_stream(cache.lens.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph):
                self.logits = self._body()
        finally:
            cache._set_mirror(mirror)  # recorded, not run: the device lengths have not moved

    def _check_usable(self):
        cache = self.cache
        if cache._epoch != self._epoch:
            raise RuntimeError("DecodeGraph: the cache was reset or rows were freed after the capture; "
                               "capture a new graph")
        if cache.bound + 1 > cache.max_len:
            raise ValueError(f"KV cache overflow: {cache.bound} cached + 1 new tokens > max_len {cache.max_len}")
        if self._paged and self._left < 1:
            raise ValueError(f"DecodeGraph: the blocks of {self.steps} steps were reserved at capture and are used up")

    def step(self):
        """One decode step: replay the graph (no launch from Python) and advance the host
        mirrors by one.  Raises before anything runs when the cache is full, when the steps
        reserved at capture are used up (paged) or when the cache was reset since."""
        self._check_usable()
        if self.graph is None:
            self.logits = self._body()
        else:
            self.graph.replay()
            self.cache._advance_mirror(1)
        self._left -= 1
        self.replays += 1
        return self.state.tok


class GenerationMixin:
    """KV-cache inference for a causal LM (see the module docstring for the hooks)."""

    # per decoder layer, the names of the matrices quantize_weights() converts (set by the model)
    _quant_weights = ()

    @torch.no_grad()
    def quantize_weights(self, fmt="fp8_e4m3", include_head=False):
        """Weight-only quantisation for generation: every decoder layer's matrices (and with
        ``include_head`` an untied ``lm_head``) become ``ops.Fp8Weight``s -- e4m3 codes plus
        one power-of-two fp32 scale per output column -- and the bf16 parameters are dropped.
        Embeddings, norms, biases and a tied head stay as they are.  ``decode_step`` then runs
        the same ops with those products on the e4m3 weight-streaming kernel; prefill and
        ``model(ids)`` run the usual kernels on a transient dequantised image of one layer
        matrix (the two MLP matrices of a fused SwiGLU block) at a time, which is exact.
        The model is inference only afterwards.  Returns ``self``."""
        if fmt != "fp8_e4m3":
            raise ValueError(f"quantize_weights: unknown fmt {fmt!r} (supported: 'fp8_e4m3')")
        if getattr(self, "_pa_quantized", None) is not None:
            raise RuntimeError(f"quantize_weights: the weights are already quantised ({self._pa_quantized})")
        if getattr(self, "tp", None) is not None:
            raise NotImplementedError("quantize_weights() with tensor parallelism is not implemented")
        if not self._quant_weights:
            raise NotImplementedError(f"quantize_weights() is not implemented for {type(self).__name__}")
        if include_head and getattr(self, "lm_head", None) is None:
            raise ValueError("quantize_weights: include_head=True needs an untied lm_head")
        targets = [(layer, n) for layer in self.layers for n in self._quant_weights]
        if include_head:
            targets.append((self, "lm_head"))
        for mod, n in targets:  # before anything is changed
            if not torch.isfinite(getattr(mod, n)).all():
                raise ValueError(f"quantize_weights: {n} has a non-finite value")
        for mod, n in targets:
            w8 = ops.quantize_weight_fp8(getattr(mod, n).detach())
            delattr(mod, n)  # the parameter (and whatever ops cached on it) goes
            setattr(mod, n, w8)
        self._pa_quantized = fmt
        self.state_dict = self.load_state_dict = self.set_state_dict = _quantized_state_error
        return self.eval()

    def _check_generation_supported(self):
        if getattr(self, "tp", None) is not None:
            raise NotImplementedError("generate() with tensor parallelism is not implemented")

    def _gen_device(self):
        return next(self.parameters()).device

    def init_cache(self, batch: int, max_len: int, paged: bool = False, block_size=None, num_blocks=None,
                   kv_dtype=None):
        """An empty cache for ``batch`` rows of up to ``max_len`` tokens each: one slab per
        layer, or with ``paged=True`` a pool of ``num_blocks`` blocks of ``block_size``
        tokens (default: ``batch * ceil(max_len / block_size)``, the slab's capacity).
        ``kv_dtype="fp8_e4m3"``: either layout stores e4m3 codes and one power-of-two scale
        per (token, kv head) (ops/kv_fp8.py); ``None``: the model's dtype."""
        self._check_generation_supported()
        cfg = self.cfg
        if max_len > cfg.max_position_embeddings:
            raise ValueError(f"cache of {max_len} tokens exceeds max_position_embeddings "
                             f"({cfg.max_position_embeddings})")
        kvh = getattr(cfg, "kv_heads", cfg.num_attention_heads)
        p = next(self.parameters())
        if paged:
            return PagedKVCache(cfg.num_hidden_layers, batch, max_len, kvh, cfg.head_dim, p.dtype, p.device,
                                block_size=block_size, num_blocks=num_blocks, kv_dtype=kv_dtype)
        if block_size is not None or num_blocks is not None:
            raise ValueError("init_cache: block_size / num_blocks need paged=True")
        return KVCache(cfg.num_hidden_layers, batch, max_len, kvh, cfg.head_dim, p.dtype, p.device, kv_dtype=kv_dtype)

    @torch.no_grad()
    def prefill(self, input_ids, cache, prompt_lens=None, rows=None, chunk=None):
        """Run the right-padded prompt [B, S] through the model, fill ``cache`` and return
        the logits [B, V] of each row's last valid position (``prompt_lens[b] - 1``;
        default: every row has S tokens).

        A paged cache reserves each row's own prompt length, not S: padding in the tail of
        a row's last block is written (and overwritten by the row's next tokens), padding
        beyond it is dropped.  With ``rows`` (paged only) ``input_ids`` is
        ``[len(rows), S]``: those cache rows are freed, reserved and refilled and every
        other row keeps its blocks, its length and its tokens; the logits are
        ``[len(rows), V]``.

        ``chunk=C`` bounds the activations to C columns at a time: the first ``min(C, S)``
        columns run the one-shot kernels, every further slice of C columns the ``extend``
        path (``ops.kv_append`` + ``ops.extend_attention``) on top of the columns already
        cached.  ``chunk >= S`` is the one-shot call, bit for bit; a smaller chunk computes
        the same function in another summation order.  One difference: with an fp8 cache
        later chunks attend to the *quantised* earlier chunks, one-shot prefill to the
        unquantised prompt.  With quantised weights every chunk of more than
        ``ops.skinny.MAX_ROWS`` rows pays one dequantisation per matrix."""
        self._check_generation_supported()
        B, S = input_ids.shape
        paged = getattr(cache, "paged", False)
        if rows is not None and not paged:
            raise ValueError("prefill: rows= needs a paged cache")
        if chunk is not None:
            chunk = int(chunk)
            if chunk < 1:
                raise ValueError(f"prefill: chunk must be at least 1, got {chunk}")
            if chunk >= S:
                chunk = None
        lens = [S] * B if prompt_lens is None else [int(x) for x in (
            prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
        if len(lens) != B or min(lens) < 1 or max(lens) > S:
            raise ValueError(f"prompt_lens must be {B} values in [1, {S}], got {lens}")
        if paged:
            y = self._prefill_paged(input_ids, cache, lens, rows, chunk)
        elif chunk is None:
            cache.reset()
            cache.check_room(S)
            y = self._prefill_hidden(input_ids, cache)
            cache.set_lens(lens)
        else:
            cache.reset()
            cache.check_room(S)
            y = self._prefill_chunks(input_ids, cache, lens, None, chunk)
        if chunk is not None:
            return self._lm_logits(y)  # [B, H]: each row's last valid position already
        H = y.shape[-1]
        last = torch.tensor([b * S + n - 1 for b, n in enumerate(lens)], dtype=torch.long, device=y.device)
        return self._lm_logits(ops.row_gather(y.reshape(B * S, H), last))

    def _prefill_chunks(self, input_ids, cache, lens, rows, chunk):
        """The prompt in slices of ``chunk`` columns (the cache is empty and, when paged,
        reserved and inside ``prefilling(rows)``): the first slice through the one-shot
        kernels, the others through the extend path.  After a slice row b has
        ``min(columns so far, lens[b])`` tokens, so a finished row's padding lands behind
        its own tokens (where the next decode step overwrites it, or in no block at all)
        and never on them.  Returns the hidden state [B, H] of each row's last valid token."""
        B, S = input_ids.shape
        dev = input_ids.device
        last_h = None
        for c0 in range(0, S, chunk):
            c1 = min(c0 + chunk, S)
            ids = input_ids[:, c0:c1]
            if c0 == 0:
                y = self._prefill_hidden(ids, cache)
                if rows is None:
                    cache.set_lens([min(c1, n) for n in lens])
                else:
                    cache.set_lens([min(c1, n) for n in lens], rows)
            else:
                y = self._extend_hidden(ids, cache)
                inc = [min(max(n - c0, 0), c1 - c0) for n in lens]
                if rows is None:
                    cache.advance_each(inc)
                else:
                    cache.advance_each(inc, rows)
            # the rows whose last valid token is in this slice
            here = [c0 <= n - 1 < c1 for n in lens]
            if any(here):
                idx = torch.tensor([b * (c1 - c0) + (n - 1 - c0 if h else 0) for b, (n, h) in enumerate(zip(lens, here))],
                                   dtype=torch.long, device=dev)
                got = ops.row_gather(y.reshape(B * (c1 - c0), y.shape[-1]), idx)
                if last_h is None:  # a row not in this slice is in a later one and is replaced there
                    last_h = got
                else:
                    last_h = torch.where(torch.tensor(here, device=dev).view(B, 1), got, last_h)
        return last_h

    @torch.no_grad()
    def extend(self, input_ids, cache, new_lens=None, all_logits=False, rows=None):
        """Feed T more tokens per row, ``input_ids`` [B, T] right-padded with ``new_lens[b]``
        in [1, T] valid ones (default T), on top of what ``cache`` holds: a further turn of a
        conversation, a chunk of a long prompt, or T candidate tokens to score in one pass.
        Row b's tokens go in at its own positions ``lens[b] + t`` and attend to the row's
        cached tokens plus the chunk itself up to t; afterwards ``lens[b] += new_lens[b]``.

        Returns the logits [B, V] at each row's last valid new token, or with ``all_logits``
        [B, T, V] (positions ``t >= new_lens[b]`` are unspecified).  ``rows`` (paged only):
        ``input_ids`` is ``[len(rows), T]`` and every other cache row is untouched.

        Overflow of ``max_len`` (a contiguous cache: the conservative ``bound + T``, since the
        padding of a short row is written too; a paged one: each row's ``lens[b] +
        new_lens[b]``, and the pool), of the rotary table or of ``max_position_embeddings``
        raises ``ValueError`` on the host before any launch, with nothing changed."""
        self._check_generation_supported()
        B, T = input_ids.shape
        paged = getattr(cache, "paged", False)
        if rows is not None and not paged:
            raise ValueError("extend: rows= needs a paged cache")
        nl = [T] * B if new_lens is None else [int(x) for x in (
            new_lens.tolist() if torch.is_tensor(new_lens) else new_lens)]
        if T < 1 or len(nl) != B or min(nl) < 1 or max(nl) > T:
            raise ValueError(f"new_lens must be {B} values in [1, {T}], got {nl}")
        if paged:
            rl = cache._check_rows(rows)
            if len(rl) != B:
                raise ValueError(f"extend: {B} rows of tokens for cache rows {rl}")
            top = max(cache.host_lens[r] for r in rl) + T
        else:
            if B != cache.batch:
                raise ValueError(f"extend: {B} rows of tokens for a cache of {cache.batch} rows")
            top = cache.bound + T
        if top > self._max_positions():
            raise ValueError(f"extend: position {top - 1} is beyond the model's {self._max_positions()} positions")
        if paged:
            # each row's own new length, not lens + T: padding past a row's blocks is dropped
            cache.reserve([cache.host_lens[r] + n for r, n in zip(rl, nl)], rl)
            with cache.prefilling(rl):
                y = self._extend_hidden(input_ids, cache)
            cache.advance_each(nl, rl)
        else:
            cache.check_room(T)
            y = self._extend_hidden(input_ids, cache)
            cache.advance_each(nl)
        H = y.shape[-1]
        if all_logits:
            return self._lm_logits(y.reshape(B * T, H)).view(B, T, -1)
        last = torch.tensor([b * T + n - 1 for b, n in enumerate(nl)], dtype=torch.long, device=y.device)
        return self._lm_logits(ops.row_gather(y.reshape(B * T, H), last))

    def _prefill_paged(self, input_ids, cache, lens, rows, chunk=None):
        B, S = input_ids.shape
        if S > cache.max_len:
            raise ValueError(f"KV cache overflow: a prompt of {S} tokens > max_len {cache.max_len}")
        if rows is None:
            if B != cache.batch:
                raise ValueError(f"prefill: {B} prompts for a cache of {cache.batch} rows")
            cache.reset()
        else:
            rows = cache._check_rows(rows)
            if len(rows) != B:
                raise ValueError(f"prefill: {B} prompts for rows {rows}")
            # the rows' own blocks come back first: raise now, with nothing freed, if even so the pool is short
            bs = cache.block_size
            if sum(-(-n // bs) - len(cache.row_blocks(r)) for r, n in zip(rows, lens)) > cache.blocks_free:
                raise ValueError(f"paged KV cache: out of blocks for prompts of {lens} tokens in rows {rows}")
            cache.free_rows(rows)
        cache.reserve(lens, rows)
        if chunk is not None:  # the lengths move slice by slice and end at lens
            with cache.prefilling(rows):
                return self._prefill_chunks(input_ids, cache, lens, rows, chunk)
        with cache.prefilling(rows):
            y = self._prefill_hidden(input_ids, cache)
        cache.set_lens(lens, rows)
        return y

    @torch.no_grad()
    def decode_step(self, tokens, cache):
        """Feed one token per row (``tokens`` [B]) at each row's own position
        ``cache.lens[b]``; returns the logits [B, V] for the next token and advances the
        cache by one.  ``generate`` is a loop over this."""
        self._check_generation_supported()
        cache.check_room(1)
        y = self._decode_hidden(tokens.reshape(-1, 1), cache)
        cache.advance(1)
        return self._lm_logits(y.reshape(y.shape[0], -1))

    @torch.no_grad()
    def decode_graph(self, cache, state, steps=None, seed=0, do_sample=False, temperature=1.0, top_k=0, top_p=1.0):
        """Capture one decode step on ``cache`` and ``state`` (an ``ops.SamplerState``) for
        ``steps`` replays (default: what ``state`` and the cache have room for); see
        :class:`DecodeGraph`."""
        return DecodeGraph(self, cache, state, steps, seed, do_sample, temperature, top_k, top_p)

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, prompt_lens=None, do_sample=False, temperature=1.0, top_k=0,
                 top_p=1.0, eos_token_id=None, pad_token_id=0, seed=None, cache="contiguous", block_size=None,
                 graph=False, sampler=None, kv_dtype=None, prefill_chunk=None, draft=None, num_draft=4):
        """Generate ``max_new_tokens`` tokens after the right-padded prompts ``input_ids``
        [B, S] (``prompt_lens``: valid length per row, default S).

        Returns ``(tokens [B, max_new_tokens] int64, lengths [B])``.  A row that has
        emitted ``eos_token_id`` keeps emitting ``pad_token_id``; ``lengths`` counts the
        tokens up to and including EOS.

        ``cache="paged"`` keeps the keys and values in blocks of ``block_size`` tokens from
        a pool of ``sum_b ceil((prompt_len_b + max_new_tokens) / block_size)`` blocks --
        what the rows can reach, not ``B * (S + max_new_tokens)`` slots; the tokens are the
        same.

        ``kv_dtype="fp8_e4m3"`` keeps either cache in e4m3 with one scale per (token, kv
        head): half the bytes, and the tokens of a run whose cache holds the dequantised
        values (ops/kv_fp8.py).  Prefill attends to the unquantised prompt.

        ``prefill_chunk=C`` runs the prompt through ``prefill(chunk=C)``: C columns at a time,
        everything after the prefill unchanged.

        ``sampler``: ``"torch"`` (``sample_next`` with a ``torch.Generator``; the default) or
        ``"philox"`` (``ops.sample_step``: the device kernel, the counter-based generator and
        the bookkeeping on the device, no ATen launches between steps; with ``seed=None`` a
        random seed).  ``graph=True`` captures one decode step after the prefill and replays
        it for the remaining tokens (:class:`DecodeGraph`); it needs, and defaults to, the
        ``"philox"`` sampler.  Greedy tokens are the same on every path; sampled tokens differ
        between the two samplers, which draw different random numbers.

        ``draft=model`` turns on speculative decoding (models/speculative.py): the draft proposes
        ``num_draft`` (1..16) tokens per row and round, this model scores them in one ``extend``
        pass and ``ops.spec_verify`` keeps the longest accepted run plus one token of its own.
        Greedy tokens are this model's greedy tokens, sampled tokens are distributed as its
        filtered distribution.  The sampler is ``"philox"``; ``graph=True`` is not supported.
        Both caches hold ``S + max_new_tokens + num_draft`` tokens; the decoder, with its
        counters, stays at ``self.last_speculation``."""
        self._check_generation_supported()
        if draft is not None:
            from .speculative import SpeculativeDecoder

            dec = SpeculativeDecoder(self, draft, num_draft)
            self.last_speculation = dec
            return dec.generate(input_ids, max_new_tokens, prompt_lens, do_sample, temperature, top_k, top_p,
                                eos_token_id, pad_token_id, seed, cache, block_size, graph, sampler, kv_dtype,
                                prefill_chunk)
        if sampler is None:
            sampler = "philox" if graph else "torch"
        if sampler not in ("torch", "philox"):
            raise ValueError(f"generate: sampler must be 'torch' or 'philox', got {sampler!r}")
        if graph and sampler != "philox":
            raise ValueError("generate: graph=True needs sampler='philox' (a torch.Generator draw does not replay)")
        if cache not in ("contiguous", "paged"):
            raise ValueError(f"generate: cache must be 'contiguous' or 'paged', got {cache!r}")
        if block_size is not None and cache != "paged":
            raise ValueError("generate: block_size needs cache='paged'")
        ops.kv_fp8.check_kv_dtype(kv_dtype)
        B, S = input_ids.shape
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        if S + max_new_tokens > self.cfg.max_position_embeddings:
            raise ValueError(f"prompt ({S}) + max_new_tokens ({max_new_tokens}) exceeds max_position_embeddings "
                             f"({self.cfg.max_position_embeddings})")
        dev = input_ids.device
        gen = None
        if do_sample and sampler == "torch":
            gen = torch.Generator(device=dev)
            if seed is not None:
                gen.manual_seed(int(seed))
            else:
                gen.seed()
        if cache == "paged":
            bs = DEFAULT_BLOCK_SIZE if block_size is None else int(block_size)
            plens = [S] * B if prompt_lens is None else [int(x) for x in (
                prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
            cache = self.init_cache(B, S + max_new_tokens, paged=True, block_size=bs,
                                    num_blocks=sum(-(-(n + max_new_tokens) // bs) for n in plens), kv_dtype=kv_dtype)
        else:
            cache = self.init_cache(B, S + max_new_tokens, kv_dtype=kv_dtype)
        if sampler == "philox":
            seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
            how = (seed, do_sample, temperature, top_k, top_p)
            st = ops.SamplerState(B, max_new_tokens, dev, eos_token_id, pad_token_id)
            ops.sample_step(self.prefill(input_ids, cache, prompt_lens, chunk=prefill_chunk), st, *how)
            if max_new_tokens > 1 and graph:
                g = self.decode_graph(cache, st, max_new_tokens, *how)
                for _ in range(max_new_tokens - 1):
                    g.step()
            else:
                for _ in range(max_new_tokens - 1):
                    ops.sample_step(self.decode_step(st.tok, cache), st, *how)
            return st.out, st.lengths
        out = torch.full((B, max_new_tokens), int(pad_token_id), dtype=torch.long, device=dev)
        lengths = torch.full((B,), max_new_tokens, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        logits = self.prefill(input_ids, cache, prompt_lens, chunk=prefill_chunk)
        for step in range(max_new_tokens):
            nxt = sample_next(logits, do_sample, temperature, top_k, top_p, gen)
            nxt = torch.where(done, torch.full_like(nxt, int(pad_token_id)), nxt)
            out[:, step] = nxt
            if eos_token_id is not None:
                hit = (nxt == int(eos_token_id)) & ~done
                lengths = torch.where(hit, torch.full_like(lengths, step + 1), lengths)
                done = done | hit
            if step + 1 < max_new_tokens:
                logits = self.decode_step(nxt, cache)
        return out, lengths
