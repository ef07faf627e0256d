"""Paged KV cache on the reference (CPU, fp32) paths: the block allocator, pool exhaustion,
append / generation against the contiguous cache, and replacing one row of a running batch."""
import pytest
import torch

from paddle_amd import ops
from test_generation_cpu import MODELS, model_and_prompt, recompute_greedy


def paged(B, max_len, bs=16, num_blocks=None, Hk=2, D=16, layers=1):
    return ops.PagedKVCache(layers, B, max_len, Hk, D, torch.float32, "cpu", block_size=bs, num_blocks=num_blocks)


def owned(cache):
    return [len(cache.row_blocks(r)) for r in range(cache.batch)]


def balanced(cache):
    used = sum(owned(cache))
    table_ids = cache.host_table[cache.host_table >= 0].tolist()
    return (cache.blocks_used == used and cache.blocks_used + cache.blocks_free == cache.num_blocks
            and sorted(table_ids + cache.free_blocks) == list(range(cache.num_blocks))
            and torch.equal(cache.block_table, cache.host_table))


# ------------------------------------------------------------------ allocator
def _allocator_script(cache):
    """One fixed call sequence; returns the table after every call."""
    seen = []
    cache.reserve([0, 1, 16, 17])
    cache.set_lens([0, 1, 16, 17])
    seen.append(cache.host_table)
    cache.advance(15)  # 15, 16, 31, 32: rows 0 and 2 take a block
    seen.append(cache.host_table)
    cache.advance(1)  # 16, 17, 32, 33: rows 1 and 3 cross a boundary
    seen.append(cache.host_table)
    cache.free_rows([1, 3])
    seen.append(cache.host_table)
    cache.reserve([40], rows=[1])
    seen.append(cache.host_table)
    return seen


def test_allocator_counts_and_reuse():
    cache = paged(4, 64)
    assert cache.max_blocks == 4 and cache.num_blocks == 16 and cache.blocks_free == 16
    cache.reserve([0, 1, 16, 17])
    cache.set_lens([0, 1, 16, 17])
    assert owned(cache) == [0, 1, 1, 2] and balanced(cache)
    assert cache.lens.tolist() == [0, 1, 16, 17] and cache.bound == 17
    cache.advance(15)  # lengths 15, 16, 31, 32: rows 0 and 2 cross a boundary, one block each
    assert owned(cache) == [1, 1, 2, 2] and balanced(cache)
    cache.advance(1)  # 16, 17, 32, 33: rows 1 and 3 cross one; rows 0 and 2 fill theirs exactly
    assert owned(cache) == [1, 2, 2, 3] and balanced(cache)
    assert cache.host_lens == [16, 17, 32, 33] and cache.lens.tolist() == [16, 17, 32, 33]
    row0, row2 = cache.row_blocks(0), cache.row_blocks(2)
    gone = cache.row_blocks(1) + cache.row_blocks(3)
    cache.free_rows([1, 3])
    assert owned(cache) == [1, 0, 2, 0] and cache.blocks_free == 13 and balanced(cache)
    assert cache.host_lens == [16, 0, 32, 0] and cache.lens.tolist() == [16, 0, 32, 0]
    assert (cache.block_table[1] == -1).all() and (cache.block_table[3] == -1).all()
    assert cache.row_blocks(0) == row0 and cache.row_blocks(2) == row2  # other rows untouched
    cache.reserve([40], rows=[1])  # 3 blocks: taken from the ones just returned
    assert set(cache.row_blocks(1)) <= set(gone) and balanced(cache)
    cache.reset()
    assert cache.blocks_free == 16 and cache.bound == 0 and balanced(cache)
    assert (cache.block_table == -1).all()


def test_allocator_is_deterministic():
    a, b = _allocator_script(paged(4, 64)), _allocator_script(paged(4, 64))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    cache = paged(4, 64)
    _allocator_script(cache)
    cache.reset()  # a reset cache is a new cache
    assert all(torch.equal(x, y) for x, y in zip(a, _allocator_script(cache)))


@pytest.mark.parametrize("how", ["reserve", "check_room", "advance", "kv_append"])
def test_exhaustion_leaves_state_untouched(how):
    # rows at 16 and 30 tokens hold 1 + 2 blocks; one more token needs a 4th block for row 0
    cache = paged(2, 64, num_blocks=3)
    cache.reserve([16, 30])
    cache.set_lens([16, 30])
    assert cache.blocks_free == 0
    before = (cache.host_lens, cache.host_table, cache.block_table.clone(), cache.free_blocks, cache.lens.clone())
    k0 = cache.k[0].clone()
    with pytest.raises(ValueError):
        if how == "reserve":
            cache.reserve([17, 30])
        elif how == "check_room":
            cache.check_room(1)
        elif how == "advance":
            cache.advance(1)
        else:
            ops.kv_append(torch.randn(2, 1, 6 * 16), cache, 0, 2, 2)
    assert cache.host_lens == before[0] and torch.equal(cache.host_table, before[1])
    assert torch.equal(cache.block_table, before[2]) and cache.free_blocks == before[3]
    assert torch.equal(cache.lens, before[4]) and torch.equal(cache.k[0], k0)
    # a pool with that one block more takes the same step
    roomy = paged(2, 64, num_blocks=4)
    roomy.reserve([16, 30])
    roomy.set_lens([16, 30])
    roomy.check_room(1)
    assert owned(roomy) == [2, 2]


def test_errors():
    with pytest.raises(ValueError):
        paged(2, 64, bs=24)
    with pytest.raises(ValueError):
        paged(2, 64, bs=8)
    with pytest.raises(ValueError):
        paged(2, 64, bs=512)
    slab = ops.KVCache(1, 2, 64, 2, 16, torch.float32, "cpu")
    with pytest.raises(ValueError):
        ops.kv_append(torch.randn(2, 1, 6 * 16), slab, 0, 2, 2, rows=[0, 1])
    model, ids = model_and_prompt("llama")
    with pytest.raises(ValueError):
        model.prefill(ids, model.init_cache(2, 16), rows=[0, 1])
    with pytest.raises(ValueError):
        model.init_cache(2, 16, block_size=16)  # block_size without paged=True
    with pytest.raises(ValueError):
        model.generate(ids, 2, cache="blocked")
    cache = paged(2, 64)
    with pytest.raises(ValueError):
        cache.set_lens([17, 0])  # no blocks reserved for 17 tokens
    with pytest.raises(ValueError):
        cache.reserve([65, 0])  # beyond max_len
    with pytest.raises(ValueError):
        cache.free_rows([0, 0])


# ------------------------------------------------------------------ append
SENTINEL = -7.5


def _append_pair(T, rope, lens, max_len=48, bs=16):
    torch.manual_seed(0)
    B, Hq, Hk, D = len(lens), 4, 2, 16
    cos, sin = ops.rope_tables(64, D) if rope else (None, None)
    slab = ops.KVCache(1, B, max_len, Hk, D, torch.float32, "cpu")
    pg = paged(B, max_len, bs=bs, Hk=Hk, D=D)
    pg.reserve(lens)
    for c in (slab, pg):
        c.k[0].fill_(SENTINEL)
        c.v[0].fill_(SENTINEL)
        c.set_lens(lens)
    qkv = torch.randn(B, T, (Hq + 2 * Hk) * D)
    return slab, pg, qkv, (Hq, Hk, cos, sin)


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("T", [1, 5])
def test_append_matches_contiguous(T, rope):
    lens = [0, 13, 37]  # 13 + 5 and 37 + 5 cross a block boundary; row 0 starts empty
    slab, pg, qkv, args = _append_pair(T, rope, lens)
    q_slab = ops.kv_append(qkv, slab, 0, *args)
    q_pg = ops.kv_append(qkv, pg, 0, *args)
    assert torch.equal(q_pg, q_slab)
    assert pg.host_lens == lens and pg.lens.tolist() == lens  # kv_append does not advance
    assert owned(pg) == [-(-(n + T) // 16) for n in lens] and balanced(pg)
    gk, gv = pg.gather(0)
    for b, n in enumerate(lens):
        assert torch.equal(gk[b, :n + T], slab.k[0][b, :n + T])  # the sentinel below n, the new tokens above
        assert torch.equal(gv[b, :n + T], slab.v[0][b, :n + T])
    # everything else in the pool is untouched: written slots are exactly the appended tokens
    written = torch.zeros(pg.num_blocks * 16, dtype=torch.bool)
    for b, n in enumerate(lens):
        for t in range(n, n + T):
            written[pg.row_blocks(b)[t // 16] * 16 + t % 16] = True
    for pool in (pg.k[0], pg.v[0]):
        flat = pool.reshape(pg.num_blocks * 16, -1)
        assert (flat[~written] == SENTINEL).all() and not (flat[written] == SENTINEL).all(-1).any()
    # gather: zeros where no block is assigned
    for b in range(3):
        assert (gk[b, len(pg.row_blocks(b)) * 16:] == 0).all()


def test_append_drops_a_token_without_a_block():
    slab, pg, qkv, args = _append_pair(5, True, [0, 13, 37])
    pg.check_room(5)
    # take row 1's second block away behind the allocator's back: tokens 16, 17 have no slot
    stale = pg.block_table.clone()
    lost = int(stale[1, 1])
    pg.block_table[1, 1] = -1
    ops.kv_append(qkv, pg, 0, *args)
    ops.kv_append(qkv, slab, 0, *args)
    assert (pg.k[0][lost] == SENTINEL).all() and (pg.v[0][lost] == SENTINEL).all()
    gk, _ = pg.gather(0)
    assert torch.equal(gk[1, 13:16], slab.k[0][1, 13:16]) and (gk[1, 16:32] == 0).all()
    assert torch.equal(gk[2, 37:42], slab.k[0][2, 37:42])
    # a poisoned entry is dropped the same way
    pg.block_table[1, 1] = pg.num_blocks + 7
    ops.kv_append(qkv, pg, 0, *args)
    assert (pg.k[0][lost] == SENTINEL).all()


def test_append_rows_maps_input_rows():
    slab, pg, qkv, args = _append_pair(5, True, [0, 13, 37])
    ops.kv_append(qkv, slab, 0, *args)
    sub = qkv[[2, 0]]
    q = ops.kv_append(sub, pg, 0, *args, rows=[2, 0])
    assert q.shape[0] == 2 and owned(pg) == [1, 1, 3]  # row 1 neither written nor grown
    gk, gv = pg.gather(0)
    assert torch.equal(gk[2, 37:42], slab.k[0][2, 37:42]) and torch.equal(gv[0, 0:5], slab.v[0][0, 0:5])
    assert (pg.k[0][pg.row_blocks(1)[0]] == SENTINEL).all()


# ------------------------------------------------------------------ models
def _teacher_forced(model, ids, P, **cache_kw):
    B, S = ids.shape
    cache = model.init_cache(B, S, **cache_kw)
    out = [model.prefill(ids[:, :P], cache)]
    for t in range(P, S):
        out.append(model.decode_step(ids[:, t], cache))
    return torch.stack(out, 1), cache


@pytest.mark.parametrize("kind", MODELS)
def test_models_paged_equals_contiguous(kind):
    model, ids = model_and_prompt(kind)
    V = model.cfg.vocab_size
    # greedy
    want, want_len = model.generate(ids, 8)
    got, got_len = model.generate(ids, 8, cache="paged", block_size=16)
    assert torch.equal(got, want) and torch.equal(got_len, want_len)
    # ragged prompts
    g = torch.Generator().manual_seed(1)
    padded = torch.randint(1, V, (2, 7), generator=g)
    padded[0, 3:] = 0
    want, _ = model.generate(padded, 8, prompt_lens=[3, 7])
    got, _ = model.generate(padded, 8, prompt_lens=[3, 7], cache="paged", block_size=16)
    assert torch.equal(got, want)
    # seeded sampling with EOS (row 0's first sampled token ends row 0 at once)
    kw = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.95, seed=123)
    free, _ = model.generate(ids, 8, **kw)
    kw.update(eos_token_id=int(free[0, 0]), pad_token_id=3)
    want, want_len = model.generate(ids, 8, **kw)
    got, got_len = model.generate(ids, 8, cache="paged", block_size=16, **kw)
    assert want_len[0].item() == 1
    assert torch.equal(got, want) and torch.equal(got_len, want_len)
    # teacher-forced logits, bit for bit
    torch.manual_seed(3)
    seq = torch.randint(1, V, (2, 24))
    want, _ = _teacher_forced(model, seq, 8)
    got, cache = _teacher_forced(model, seq, 8, paged=True, block_size=16)
    assert torch.equal(got, want)
    assert cache.host_lens == [24, 24] and owned(cache) == [2, 2]


def test_generate_pool_size(monkeypatch):
    """generate(cache="paged") asks for sum_b ceil((prompt_len_b + max_new_tokens) / block_size)
    blocks, and that pool is enough."""
    model, _ = model_and_prompt("llama")
    asked = []
    real = type(model).init_cache

    def spy(self, *a, **kw):
        cache = real(self, *a, **kw)
        asked.append(cache)
        return cache

    monkeypatch.setattr(type(model), "init_cache", spy)
    g = torch.Generator().manual_seed(2)
    padded = torch.randint(1, model.cfg.vocab_size, (3, 30), generator=g)
    model.generate(padded, 12, prompt_lens=[3, 20, 30], cache="paged", block_size=16)
    cache = asked[-1]
    assert cache.num_blocks == 1 + 2 + 3  # ceil(15 / 16) + ceil(32 / 16) + ceil(42 / 16)
    assert cache.num_blocks < 3 * cache.max_blocks  # the slab's capacity would be 9 blocks
    assert cache.host_lens == [3 + 11, 20 + 11, 30 + 11] and owned(cache) == [1, 2, 3]


# ------------------------------------------------------------------ admission
@pytest.mark.parametrize("kind", MODELS)
def test_admission_replaces_one_row(kind):
    """Prefill two rows, decode 3 steps, replace row 0 by a new prompt, decode 5 more.

    Row 0 then decodes the new prompt's greedy continuation; row 1's logits are bit-equal
    to a run in which row 0 was never replaced.  (Checked when this was written: on CPU
    fp32 every op of the decode step computes a batch row from that row alone, so row 1
    cannot see what row 0 holds.)"""
    model, ids = model_and_prompt(kind)
    g = torch.Generator().manual_seed(7)
    new_prompt = torch.randint(1, model.cfg.vocab_size, (1, 9), generator=g)

    def run(replace):
        cache = model.init_cache(2, 40, paged=True, block_size=16)
        logits = model.prefill(ids, cache)
        row1, row0 = [logits[1]], []
        for step in range(8):
            if step == 3 and replace:
                held = cache.row_blocks(1)
                first = model.prefill(new_prompt, cache, rows=[0])
                assert first.shape == (1, logits.shape[1])
                assert cache.row_blocks(1) == held and cache.host_lens == [9, 5 + 3]
                logits = torch.cat([first, logits[1:]], 0)
            tok = logits.argmax(-1)
            if step >= 3:
                row0.append(tok[0])
            logits = model.decode_step(tok, cache)
            row1.append(logits[1])
        return torch.stack(row1), torch.stack(row0), cache

    kept1, _, _ = run(False)
    got1, got0, cache = run(True)
    assert torch.equal(got1, kept1)
    assert torch.equal(got0, recompute_greedy(model, new_prompt, 5)[0])
    assert cache.host_lens == [9 + 5, 5 + 8] and cache.lens.tolist() == [14, 13]
