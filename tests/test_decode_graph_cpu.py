"""``generate(graph=True)`` / ``sampler="philox"`` on the CPU, where the graph path runs the
same sequence (reference sampler, one ``SamplerState``, ``DecodeGraph.step``) without a graph."""
import pytest
import torch

from paddle_amd import ops
from test_generation_cpu import MODELS, make_model

_models = {}


def model_and_prompts(kind):
    """One model and one ragged right-padded prompt batch per kind, shared and left unchanged."""
    if kind not in _models:
        m = make_model(kind)
        g = torch.Generator().manual_seed(3)
        ids = torch.zeros(3, 7, dtype=torch.long)
        for b, n in enumerate((3, 7, 5)):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        _models[kind] = (m, ids)
    return _models[kind]


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
@pytest.mark.parametrize("kind", MODELS)
def test_greedy_graph_equals_generate(kind, cache):
    model, ids = model_and_prompts(kind)
    kw = dict(prompt_lens=[3, 7, 5], cache=cache)
    if cache == "paged":
        kw["block_size"] = 16
    want, want_len = model.generate(ids, 12, **kw)
    toks, lengths = model.generate(ids, 12, graph=True, **kw)
    assert toks.dtype == torch.int64 and toks.shape == (3, 12)
    assert torch.equal(toks, want) and torch.equal(lengths, want_len)
    toks, lengths = model.generate(ids, 12, sampler="philox", **kw)
    assert torch.equal(toks, want) and torch.equal(lengths, want_len)


def test_one_new_token():
    model, ids = model_and_prompts("llama")
    want, _ = model.generate(ids, 1, prompt_lens=[3, 7, 5])
    toks, lengths = model.generate(ids, 1, prompt_lens=[3, 7, 5], graph=True)
    assert torch.equal(toks, want) and lengths.tolist() == [1, 1, 1]


@pytest.mark.parametrize("graph", [False, True])
def test_philox_sampling_is_a_function_of_the_seed(graph):
    model, ids = model_and_prompts("llama")
    kw = dict(prompt_lens=[3, 7, 5], do_sample=True, temperature=0.9, top_k=50, top_p=0.95, sampler="philox",
              graph=graph)
    a, _ = model.generate(ids, 10, seed=11, **kw)
    b, _ = model.generate(ids, 10, seed=11, **kw)
    c, _ = model.generate(ids, 10, seed=12, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.min().item() >= 0 and a.max().item() < model.cfg.vocab_size
    # the graph path and the launch loop draw the same tokens
    d, _ = model.generate(ids, 10, seed=11, **dict(kw, graph=not graph))
    assert torch.equal(a, d)
    # top_k = 1 is greedy whatever the seed
    greedy, _ = model.generate(ids, 10, prompt_lens=[3, 7, 5])
    k1, _ = model.generate(ids, 10, seed=5, **dict(kw, top_k=1))
    assert torch.equal(k1, greedy)


def test_eos_lengths_and_padding_match_todays_path():
    model, ids = model_and_prompts("llama")
    greedy, _ = model.generate(ids, 10, prompt_lens=[3, 7, 5])
    eos, pad = int(greedy[0, 2]), 3
    kw = dict(prompt_lens=[3, 7, 5], eos_token_id=eos, pad_token_id=pad)
    want, want_len = model.generate(ids, 10, **kw)
    assert want_len[0] <= 3 and want[0, int(want_len[0]):].tolist() == [pad] * (10 - int(want_len[0]))
    for how in (dict(graph=True), dict(sampler="philox")):
        toks, lengths = model.generate(ids, 10, **kw, **how)
        assert torch.equal(toks, want) and torch.equal(lengths, want_len)


def test_arguments():
    model, ids = model_and_prompts("llama")
    with pytest.raises(ValueError):
        model.generate(ids, 4, graph=True, sampler="torch")
    with pytest.raises(ValueError):
        model.generate(ids, 4, sampler="numpy")
    model.tp = object()
    try:
        with pytest.raises(NotImplementedError):
            model.generate(ids, 2, graph=True)
    finally:
        model.tp = None


@pytest.mark.parametrize("paged", [False, True])
def test_decode_graph_object_on_the_cpu(paged):
    model, ids = model_and_prompts("llama")
    B, S = ids.shape
    kw = dict(paged=True, block_size=16) if paged else {}
    cache = model.init_cache(B, S + 4, **kw)
    st = ops.SamplerState(B, 8, "cpu")
    ops.sample_step(model.prefill(ids, cache, [3, 7, 5]), st)
    g = model.decode_graph(cache, st, steps=4)
    want, _ = model.generate(ids, 8, prompt_lens=[3, 7, 5])
    for n in range(4):
        assert g.step() is st.tok
        assert cache.lens.tolist() == [3 + n + 1, 7 + n + 1, 5 + n + 1] and cache.bound == 7 + n + 1
        assert g.logits.shape == (B, model.cfg.vocab_size)
    assert torch.equal(st.out[:, :5], want[:, :5]) and int(st.step) == 5
    lens = cache.lens.clone()
    with pytest.raises(ValueError):  # the cache is full: raised before anything runs
        g.step()
    assert torch.equal(cache.lens, lens) and int(st.step) == 5
    cache.reset()
    with pytest.raises(RuntimeError):
        g.step()


def test_decode_graph_undersized_pool_raises_up_front():
    model, ids = model_and_prompts("llama")
    B, S = ids.shape
    cache = model.init_cache(B, 40, paged=True, block_size=16, num_blocks=3)  # one block per row
    st = ops.SamplerState(B, 16, "cpu")
    ops.sample_step(model.prefill(ids, cache, [3, 7, 5]), st)
    free, table, lens = cache.free_blocks, cache.host_table, cache.host_lens
    with pytest.raises(ValueError):
        model.decode_graph(cache, st, steps=16)  # row 1 would need a second block
    assert cache.free_blocks == free and torch.equal(cache.host_table, table) and cache.host_lens == lens
    assert torch.equal(cache.block_table, table)
    g = model.decode_graph(cache, st, steps=9)  # 7 + 9 = 16 still fits
    for _ in range(9):
        g.step()
    with pytest.raises(ValueError):
        g.step()
