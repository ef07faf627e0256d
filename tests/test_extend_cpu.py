"""Multi-token extend over the KV cache on the CPU (fp32 tiny models, the plain-torch paths):
``ops.extend_attention``, the caches' ragged advance, ``model.extend``, chunked ``prefill`` and
``generate(prefill_chunk=)``, over both cache layouts."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import decode as D_
from test_generation_cpu import MODELS, make_model, recompute_greedy
from test_kv_fp8_cpu import recorded_logits, same_bits, twin_append

LAYOUTS = ["contiguous", "paged"]
PROMPT_LENS = [3, 7, 5]
S = 7

_models = {}


def model_and_prompts(kind):
    """One model and one ragged right-padded [3, 7] prompt batch per kind, shared, read-only."""
    if kind not in _models:
        m = make_model(kind)
        g = torch.Generator().manual_seed(11)
        ids = torch.zeros(3, S, dtype=torch.long)
        for b, n in enumerate(PROMPT_LENS):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        _models[kind] = (m, ids)
    return _models[kind]


def new_cache(model, layout, batch=3, max_len=48, **kw):
    if layout == "paged":
        return model.init_cache(batch, max_len, paged=True, block_size=16, **kw)
    return model.init_cache(batch, max_len, **kw)


def gen_kw(layout):
    return dict(cache="paged", block_size=16) if layout == "paged" else dict(cache="contiguous")


# ---------------------------------------------------------------------- the op
@pytest.mark.parametrize("layout", LAYOUTS)
def test_extend_attention_is_causal_attention_over_the_cache(layout):
    """Against a hand-written mask: token t of row b sees keys n < base_len[b] + t + 1."""
    torch.manual_seed(0)
    B, T, Hq, Hk, D, S_max, lens = 3, 5, 4, 2, 16, 40, [0, 9, 30]
    if layout == "paged":
        cache = ops.PagedKVCache(1, B, S_max, Hk, D, torch.float32, block_size=16)
    else:
        cache = ops.KVCache(1, B, S_max, Hk, D, torch.float32)
    ops.kv_append(torch.randn(B, 36, (Hq + 2 * Hk) * D), cache, 0, Hq, Hk)  # lens stay 0: contents only
    q = torch.randn(B, T, Hq, D)
    base = torch.tensor(lens, dtype=torch.int32)
    o = ops.extend_attention(q, cache, 0, base_len=base)
    assert o.shape == (B, T, Hq, D)
    k, v = cache.dequant(0)
    ke, ve = k.repeat_interleave(Hq // Hk, 2), v.repeat_interleave(Hq // Hk, 2)
    s = torch.einsum("bthd,bnhd->bhtn", q, ke) * D ** -0.5
    n = torch.arange(S_max)
    vis = n[None, None, :] < (base.long()[:, None, None] + torch.arange(T)[None, :, None] + 1)  # [B, T, n]
    s = s.masked_fill(~vis[:, None], float("-inf"))
    want = torch.einsum("bhtn,bnhd->bthd", torch.softmax(s, -1), ve)
    assert torch.allclose(o, want, rtol=1e-5, atol=1e-6)
    # T = 1 at base_len = kv_len - 1 is the decode definition
    o1 = ops.extend_attention(q[:, :1], cache, 0, base_len=base)
    assert torch.allclose(o1, ops.decode_attention(q[:, :1], cache, 0, kv_len=base + 1), rtol=1e-5, atol=1e-6)


def test_extend_attention_at_the_end_of_the_cache():
    """A chunk that reaches max_len: every token sees at most max_len keys."""
    torch.manual_seed(1)
    B, T, H, D, S_max = 1, 4, 1, 16, 8
    cache = ops.KVCache(1, B, S_max, H, D, torch.float32)
    ops.kv_append(torch.randn(B, S_max, 3 * H * D), cache, 0, H, H)
    q = torch.randn(B, T, H, D)
    o = ops.extend_attention(q, cache, 0, base_len=torch.tensor([6], dtype=torch.int32))
    for t in range(T):
        lim = min(6 + t + 1, S_max)
        want = D_._attn_ref(q[:, t:t + 1], cache.k[0][:, :lim], cache.v[0][:, :lim], False, D ** -0.5)
        assert torch.allclose(o[:, t:t + 1], want, rtol=1e-5, atol=1e-6)


def test_extend_attention_rows_and_guards():
    torch.manual_seed(2)
    B, T, H, D, S_max = 3, 3, 2, 16, 32
    cache = ops.PagedKVCache(1, B, S_max, H, D, torch.float32, block_size=16)
    ops.kv_append(torch.randn(B, 20, 3 * H * D), cache, 0, H, H)
    cache.set_lens([4, 9, 12])
    q = torch.randn(B, T, H, D)
    full = ops.extend_attention(q, cache, 0)
    sub = ops.extend_attention(q[[2, 0]], cache, 0, rows=[2, 0])
    assert torch.equal(sub, full[[2, 0]])
    with cache.prefilling([2, 0]):
        assert torch.equal(ops.extend_attention(q[[2, 0]], cache, 0), sub)
        with pytest.raises(ValueError):
            ops.extend_attention(q[[2, 0]], cache, 0, rows=[2, 0])
    with pytest.raises(ValueError):
        ops.extend_attention(q[:2], cache, 0)  # two q rows for three cache rows
    with pytest.raises(ValueError):
        ops.extend_attention(q[..., :8], cache, 0)  # head size
    with pytest.raises(ValueError):
        ops.extend_attention(q[:, 0], cache, 0)  # not [B, T, Hq, D]
    with pytest.raises(ValueError):
        ops.extend_attention(q, cache, 0, rows=[0, 0, 1])
    with pytest.raises(ValueError):
        ops.extend_attention(q, cache, 0, base_len=torch.zeros(2, dtype=torch.int32))
    flat = ops.KVCache(1, B, S_max, H, D, torch.float32)
    with pytest.raises(ValueError):
        ops.extend_attention(q, flat, 0, rows=[0, 1, 2])


# ---------------------------------------------------------------------- ragged advance
def test_ragged_advance_contiguous():
    cache = ops.KVCache(1, 3, 16, 1, 16, torch.float32)
    cache.set_lens([1, 5, 2])
    cache.advance_each([3, 1, 0])
    assert cache.lens.tolist() == [4, 6, 2] and cache.bound == 8  # the conservative bound: 5 + 3
    with pytest.raises(ValueError):
        cache.advance_each([9, 1, 1])  # bound + 9 > 16
    with pytest.raises(ValueError):
        cache.advance_each([1, 1])
    with pytest.raises(ValueError):
        cache.advance_each([1, -1, 1])
    assert cache.lens.tolist() == [4, 6, 2] and cache.bound == 8


def test_ragged_advance_paged():
    cache = ops.PagedKVCache(1, 3, 64, 1, 16, torch.float32, block_size=16, num_blocks=5)
    cache.reserve([10, 16, 1])
    cache.set_lens([10, 16, 1])
    assert cache.blocks_used == 3
    cache.advance_each([7, 1, 2])  # rows 0 and 1 need one more block each
    assert cache.host_lens == [17, 17, 3] and cache.lens.tolist() == [17, 17, 3] and cache.blocks_used == 5
    cache.advance_each([5], rows=[2])
    assert cache.host_lens == [17, 17, 8] and cache.lens.tolist() == [17, 17, 8]
    table, free = cache.host_table, cache.free_blocks
    with pytest.raises(ValueError):
        cache.advance_each([1, 1, 9])  # row 2 would need a sixth block
    with pytest.raises(ValueError):
        cache.advance_each([48, 0, 0])  # 65 > max_len
    assert cache.host_lens == [17, 17, 8] and cache.lens.tolist() == [17, 17, 8]
    assert torch.equal(cache.host_table, table) and cache.free_blocks == free
    assert torch.equal(cache.block_table, table)


# ---------------------------------------------------------------------- chunked prefill
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", MODELS)
def test_chunked_generate_tokens(kind, layout):
    model, ids = model_and_prompts(kind)
    kw = gen_kw(layout)
    with recorded_logits(model) as seen:
        want, want_len = model.generate(ids, 8, prompt_lens=PROMPT_LENS, **kw)
    for c in (1, 3, S - 1, S, S + 5):
        with recorded_logits(model) as got:
            toks, lengths = model.generate(ids, 8, prompt_lens=PROMPT_LENS, prefill_chunk=c, **kw)
        assert torch.equal(toks, want) and torch.equal(lengths, want_len), f"chunk {c}"
        if c >= S:
            assert same_bits(got[0], seen[0]), f"prefill logits, chunk {c}"
        else:
            assert torch.allclose(got[0], seen[0], rtol=1e-4, atol=1e-5), f"prefill logits, chunk {c}"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chunked_prefill_leaves_the_lengths_of_the_prompts(layout):
    model, ids = model_and_prompts("llama")
    cache = new_cache(model, layout)
    model.prefill(ids, cache, PROMPT_LENS, chunk=2)
    assert cache.lens.tolist() == PROMPT_LENS and cache.bound == max(PROMPT_LENS)
    if layout == "paged":
        assert cache.host_lens == PROMPT_LENS and cache.blocks_used == 3
    with pytest.raises(ValueError):
        model.prefill(ids, cache, PROMPT_LENS, chunk=0)


# ---------------------------------------------------------------------- extend
def turns(model, seed=5):
    """Per row: a prompt, and a second turn of ragged length."""
    g = torch.Generator().manual_seed(seed)
    V = model.cfg.vocab_size
    first = [torch.randint(1, V, (n,), generator=g) for n in PROMPT_LENS]
    second = [torch.randint(1, V, (n,), generator=g) for n in (4, 1, 6)]
    return first, second


def pad(rows, width=None):
    width = max(len(r) for r in rows) if width is None else width
    out = torch.zeros(len(rows), width, dtype=torch.long)
    for b, r in enumerate(rows):
        out[b, : len(r)] = r
    return out


@torch.no_grad()
def two_turns(model, layout, first, second, decode=3, after=5):
    """prefill -> ``decode`` greedy steps -> extend with the second turn -> ``after`` greedy
    steps.  Returns (the tokens of the first continuation, of the second, the cache)."""
    B = len(first)
    cache = new_cache(model, layout, batch=B)
    logits = model.prefill(pad(first), cache, [len(r) for r in first])
    got1 = []
    for _ in range(decode):
        nxt = logits.float().argmax(-1)
        got1.append(nxt)
        logits = model.decode_step(nxt, cache)
    logits = model.extend(pad(second), cache, [len(r) for r in second])
    got2 = []
    for i in range(after):
        nxt = logits.float().argmax(-1)
        got2.append(nxt)
        if i + 1 < after:
            logits = model.decode_step(nxt, cache)
    return torch.stack(got1, 1), torch.stack(got2, 1), cache


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", MODELS)
def test_multi_turn(kind, layout):
    model = model_and_prompts(kind)[0]
    first, second = turns(model)
    got1, got2, cache = two_turns(model, layout, first, second)
    for b in range(3):
        # decode's last token is fed by the step before the extend, so the sequence holds it
        seq = torch.cat([first[b], got1[b], second[b]])
        assert torch.equal(got1[b], recompute_greedy(model, first[b][None], 3)[0]), f"row {b}, first turn"
        assert torch.equal(got2[b], recompute_greedy(model, seq[None], 5)[0]), f"row {b}, second turn"
        alone1, alone2, _ = two_turns(model, layout, [first[b]], [second[b]])
        assert torch.equal(alone1[0], got1[b]) and torch.equal(alone2[0], got2[b]), f"row {b} alone"
    want = [len(first[b]) + 3 + len(second[b]) + 4 for b in range(3)]
    assert cache.lens.tolist() == want
    if layout == "paged":
        assert cache.host_lens == want
        assert cache.blocks_used == sum(-(-n // 16) for n in want)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", MODELS)
def test_all_logits(kind, layout):
    model = model_and_prompts(kind)[0]
    first, second = turns(model, seed=6)
    cache = new_cache(model, layout)
    model.prefill(pad(first), cache, PROMPT_LENS)
    nl = [len(r) for r in second]
    T = max(nl)
    logits = model.extend(pad(second), cache, nl, all_logits=True)
    assert logits.shape == (3, T, model.cfg.vocab_size)
    with torch.no_grad():
        for b in range(3):
            full = model(torch.cat([first[b], second[b]])[None])[0].float()
            base = len(first[b])
            for t in range(nl[b]):
                assert int(logits[b, t].float().argmax()) == int(full[base + t].argmax()), (b, t)
                assert torch.allclose(logits[b, t].float(), full[base + t], rtol=1e-4, atol=1e-4), (b, t)
    assert cache.lens.tolist() == [n + m for n, m in zip(PROMPT_LENS, nl)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", MODELS)
def test_fp8_cache_equals_the_twin(kind, layout):
    """extend and chunked prefill on an e4m3 cache against the same calls on a cache that holds
    the quantise-dequantise image of every appended token: the chunk is appended (quantised),
    then attended to."""
    model = model_and_prompts(kind)[0]
    first, second = turns(model, seed=7)
    nl = [len(r) for r in second]

    def run(**kw):
        cache = new_cache(model, layout, **kw)
        a = model.prefill(pad(first), cache, PROMPT_LENS, chunk=3)
        b = model.extend(pad(second), cache, nl, all_logits=True)
        c = model.decode_step(b[:, 0].float().argmax(-1), cache)
        return a, b, c, cache

    got = run(kv_dtype="fp8_e4m3")
    with twin_append():
        want = run()
    assert got[3].quantized and not want[3].quantized
    for name, a, b in zip(("chunked prefill", "extend", "next step"), got, want):
        if name == "extend":  # the positions past a row's new tokens are unspecified
            for r, n in enumerate(nl):
                assert same_bits(a[r, :n], b[r, :n]), f"{name}, row {r}"
        else:
            assert same_bits(a, b), name
    assert got[3].lens.tolist() == want[3].lens.tolist()


# ---------------------------------------------------------------------- bookkeeping
def pool_bits(cache):
    return cache._pool.clone()


def test_rows_leave_the_other_rows_alone():
    model = model_and_prompts("llama")[0]
    first, second = turns(model, seed=8)
    cache = new_cache(model, "paged")
    model.prefill(pad(first), cache, PROMPT_LENS)
    keep = [b for r in (0, 2) for b in cache.row_blocks(r)]
    before = pool_bits(cache)
    twin = new_cache(model, "paged")
    model.prefill(pad(first), twin, PROMPT_LENS)
    logits = model.extend(second[1][None], cache, rows=[1])
    assert logits.shape == (1, model.cfg.vocab_size)
    after = pool_bits(cache)
    assert torch.equal(before[:, :, keep], after[:, :, keep])
    assert cache.host_lens == [3, 8, 5] and cache.lens.tolist() == [3, 8, 5]
    assert [cache.row_blocks(r) for r in (0, 2)] == [twin.row_blocks(r) for r in (0, 2)]
    tok = torch.tensor([5, 6, 7])
    got, want = model.decode_step(tok, cache), model.decode_step(tok, twin)
    assert same_bits(got[[0, 2]], want[[0, 2]])
    # the row that was extended equals the same extend of every row
    full = new_cache(model, "paged")
    model.prefill(pad(first), full, PROMPT_LENS)
    all_rows = model.extend(pad([second[1]] * 3), full)
    assert torch.allclose(logits[0], all_rows[1], rtol=1e-5, atol=1e-6)


def test_pool_exhaustion_and_overflow_leave_the_state():
    model = model_and_prompts("llama")[0]
    first, _ = turns(model)
    ids = pad(first)
    cache = model.init_cache(3, 40, paged=True, block_size=16, num_blocks=4)
    model.prefill(ids, cache, PROMPT_LENS)
    state = (cache.host_lens, cache.host_table, cache.free_blocks, pool_bits(cache))
    chunk = torch.ones(3, 14, dtype=torch.long)

    def unchanged():
        return (cache.host_lens == state[0] and torch.equal(cache.host_table, state[1])
                and cache.free_blocks == state[2] and torch.equal(pool_bits(cache), state[3])
                and cache.lens.tolist() == state[0] and torch.equal(cache.block_table, state[1]))

    with pytest.raises(ValueError):
        model.extend(chunk, cache)  # 17, 21 and 19 tokens: three more blocks, one free
    assert unchanged()
    with pytest.raises(ValueError):
        model.extend(torch.ones(1, 38, dtype=torch.long), cache, rows=[0])  # 3 + 38 > max_len
    assert unchanged()
    model.extend(chunk, cache, new_lens=[13, 1, 1])  # the same chunk fits with these lengths
    assert cache.host_lens == [16, 8, 6] and cache.blocks_used == 3

    flat = model.init_cache(3, 16)
    model.prefill(ids, flat, PROMPT_LENS)
    k0 = flat.k[0].clone()
    with pytest.raises(ValueError):
        model.extend(torch.ones(3, 10, dtype=torch.long), flat, new_lens=[1, 1, 1])  # bound 7 + 10 > 16
    assert flat.lens.tolist() == PROMPT_LENS and flat.bound == 7 and torch.equal(flat.k[0], k0)


def test_extend_past_the_positions_raises():
    for kind in ("llama", "gpt"):
        model = make_model(kind)
        limit = model.cfg.max_position_embeddings
        cache = model.init_cache(1, limit)
        model.prefill(torch.ones(1, limit - 3, dtype=torch.long), cache)
        with pytest.raises(ValueError):
            model.extend(torch.ones(1, 4, dtype=torch.long), cache)
        assert cache.lens.tolist() == [limit - 3]
        model.extend(torch.ones(1, 3, dtype=torch.long), cache)
        assert cache.lens.tolist() == [limit]


def test_extend_guards():
    model, ids = model_and_prompts("llama")
    cache = new_cache(model, "contiguous")
    model.prefill(ids, cache, PROMPT_LENS)
    chunk = torch.ones(3, 4, dtype=torch.long)
    for bad in ([0, 1, 1], [5, 1, 1], [1, 1]):
        with pytest.raises(ValueError):
            model.extend(chunk, cache, new_lens=bad)
    with pytest.raises(ValueError):
        model.extend(chunk, cache, rows=[0, 1, 2])  # rows on a contiguous cache
    with pytest.raises(ValueError):
        model.extend(chunk[:2], cache)
    with pytest.raises(ValueError):
        model.prefill(ids, cache, PROMPT_LENS, chunk=0)
    with pytest.raises(ValueError):
        model.generate(ids, 2, prompt_lens=PROMPT_LENS, prefill_chunk=-1)
    assert cache.lens.tolist() == PROMPT_LENS
    paged = new_cache(model, "paged")
    model.prefill(ids, paged, PROMPT_LENS)
    with pytest.raises(ValueError):
        model.extend(chunk, paged, rows=[0, 1])  # three rows of tokens for two cache rows
    with pytest.raises(ValueError):
        model.extend(chunk, paged, rows=[0, 0, 1])
    assert paged.host_lens == PROMPT_LENS
