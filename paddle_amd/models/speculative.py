"""Speculative decoding: a small draft model proposes ``num_draft`` tokens per row, the target
scores them in one ``extend`` pass, ``ops.spec_verify`` decides on the device which survive,
and both caches take the rejected tokens back out (``rewind_each``).

Lossless: greedy output is the target's own greedy output, sampled output is distributed as
the target's filtered distribution (the contract is :mod:`paddle_amd.ops.speculative`).

One round, with ``x0`` the row's last emitted token (not yet in either cache):

* the draft runs ``G + 1`` ``decode_step``s fed ``x0, d_0 .. d_{G-1}`` (the last one only caches
  ``d_{G-1}``); ``d_j`` is ``ops.sample_tokens`` of step ``1 + round * G + j`` on the draft's
  logits, which in sampled mode are kept in one ``[B, G, V]`` buffer for the judge;
* ``target.extend([x0, d_0 .. d_{G-1}], all_logits=True)``, then ``ops.spec_verify``;
* one device-to-host read of ``kept`` [B] -- the only one in the loop: the exact host lengths
  of a paged cache and the loop's end need it;
* both caches are rewound by ``G + 1 - kept[b]`` with the exact bound.

Rows that are done keep riding along, fed ``pad``, and are rewound in full every round.  The
loop ends when every row is done: it has reached ``max_new_tokens`` (known on the host from
``kept``) or reports ``kept = 0`` (a row that hit EOS emits nothing from the next round on).
"""
from __future__ import annotations

import os

import torch

from .. import ops
from ..ops.paged import DEFAULT_BLOCK_SIZE
from ..ops.speculative import MAX_DRAFT

__all__ = ["SpeculativeDecoder"]


class SpeculativeDecoder:
    """``SpeculativeDecoder(target, draft, num_draft).generate(...)`` takes ``generate()``'s
    arguments and returns what it returns.  Counters of the last call: ``rounds``,
    ``proposed`` (candidates that had room to be emitted, over the rows still generating),
    ``accepted`` (those that were) and ``emitted`` (all tokens written, the first included)."""

    def __init__(self, target, draft, num_draft=4):
        for m in (target, draft):
            m._check_generation_supported()
        if int(draft.cfg.vocab_size) != int(target.cfg.vocab_size):
            raise ValueError(f"speculative decoding: the draft's vocab_size ({draft.cfg.vocab_size}) is not the "
                             f"target's ({target.cfg.vocab_size})")
        num_draft = int(num_draft)
        if not 1 <= num_draft <= MAX_DRAFT:
            raise ValueError(f"speculative decoding: num_draft must be in 1..{MAX_DRAFT}, got {num_draft}")
        self.target, self.draft, self.num_draft = target, draft, num_draft
        self.rounds = self.proposed = self.accepted = self.emitted = 0

    def _init_cache(self, model, B, S, plens, max_new_tokens, cache, block_size, kv_dtype):
        G = self.num_draft
        if cache == "paged":
            bs = DEFAULT_BLOCK_SIZE if block_size is None else int(block_size)
            return model.init_cache(B, S + max_new_tokens + G, paged=True, block_size=bs,
                                    num_blocks=sum(-(-(n + max_new_tokens + G) // bs) for n in plens),
                                    kv_dtype=kv_dtype)
        return model.init_cache(B, S + max_new_tokens + G, kv_dtype=kv_dtype)

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, prompt_lens=None, do_sample=False, temperature=1.0, top_k=0,
                 top_p=1.0, eos_token_id=None, pad_token_id=0, seed=None, cache="contiguous", block_size=None,
                 graph=False, sampler=None, kv_dtype=None, prefill_chunk=None):
        target, draft, G = self.target, self.draft, self.num_draft
        for m in (target, draft):
            m._check_generation_supported()
        if graph:
            raise ValueError("generate: graph=True with a draft model is not implemented")
        if sampler is None:
            sampler = "philox"
        if sampler != "philox":
            raise ValueError(f"generate: a draft model needs sampler='philox', got {sampler!r}")
        if cache not in ("contiguous", "paged"):
            raise ValueError(f"generate: cache must be 'contiguous' or 'paged', got {cache!r}")
        if block_size is not None and cache != "paged":
            raise ValueError("generate: block_size needs cache='paged'")
        ops.kv_fp8.check_kv_dtype(kv_dtype)
        B, S = input_ids.shape
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        for m, who in ((target, "the target"), (draft, "the draft")):
            if S + max_new_tokens + G > m.cfg.max_position_embeddings:
                raise ValueError(f"prompt ({S}) + max_new_tokens ({max_new_tokens}) + num_draft ({G}) exceeds "
                                 f"max_position_embeddings ({m.cfg.max_position_embeddings}) of {who}")
        dev = input_ids.device
        plens = [S] * B if prompt_lens is None else [int(x) for x in (
            prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
        tcache = self._init_cache(target, B, S, plens, max_new_tokens, cache, block_size, kv_dtype)
        dcache = self._init_cache(draft, B, S, plens, max_new_tokens, cache, block_size, kv_dtype)
        seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
        how = (do_sample, temperature, top_k, top_p)
        st = ops.SpecState(B, max_new_tokens, G, dev, eos_token_id, pad_token_id)
        self.state = st
        self.rounds = self.proposed = self.accepted = 0
        self.emitted = B

        logits = target.prefill(input_ids, tcache, prompt_lens, chunk=prefill_chunk)
        draft.prefill(input_ids, dcache, prompt_lens, chunk=prefill_chunk)
        ops.sample_step(logits, st, seed, *how)
        V = logits.shape[-1]
        dlog = torch.empty(B, G, V, dtype=logits.dtype, device=dev) if do_sample else None
        cand = torch.empty(B, G, dtype=torch.long, device=dev)
        feed = torch.empty(B, G + 1, dtype=torch.long, device=dev)
        lens = list(plens)          # exact cache lengths of both caches
        pos = [1] * B               # tokens written per row
        live = [max_new_tokens > 1] * B
        while any(live):
            rnd = self.rounds
            x = st.tok
            feed[:, 0] = x
            for j in range(G):
                lg = draft.decode_step(x, dcache)
                if dlog is not None:  # the judge sees the very numbers the candidate was drawn from
                    dlog[:, j] = lg
                    lg = dlog[:, j]
                x = ops.sample_tokens(lg, seed, 1 + rnd * G + j, *how)
                cand[:, j] = x
            draft.decode_step(x, dcache)  # caches d_{G-1}: after a full acceptance the draft is in step
            feed[:, 1:] = cand
            tl = target.extend(feed, tcache, all_logits=True)
            ops.spec_verify(tl, cand, dlog, st, seed, rnd, *how)
            kept = st.kept.tolist()  # the one host read of a round
            self.rounds += 1
            for b in range(B):
                if live[b] and kept[b] > 0:
                    self.proposed += min(G, max_new_tokens - pos[b])
                pos[b] += kept[b]
                lens[b] += kept[b]
                live[b] = live[b] and kept[b] > 0 and pos[b] < max_new_tokens
            back = [G + 1 - k for k in kept]
            if cache == "paged":
                tcache.rewind_each(back)
                dcache.rewind_each(back)
            else:
                tcache.rewind_each(back, bound=max(lens))
                dcache.rewind_each(back, bound=max(lens))
        self.emitted = sum(pos)
        self.accepted = int(st.accepted.sum())
        return st.out, st.lengths
