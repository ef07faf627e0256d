"""KV-cache generation on the reference (CPU, fp32) paths: greedy decoding against
full recomputation, ragged prompts, the kv_append reference and sampling."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.models.gpt import GPTConfig, GPTForCausalLM
from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM
from paddle_amd.ops import fused as F

MODELS = ["llama", "llama-kv1", "gpt"]


def make_model(kind, device="cpu", dtype="float32"):
    torch.manual_seed(0)
    if kind == "gpt":
        cfg = GPTConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2, num_attention_heads=2,
                        max_position_embeddings=128, dtype=dtype)
        return GPTForCausalLM(cfg, device=device).eval()
    cfg = LlamaConfig(**LLAMA_CONFIGS["llama-tiny"], num_key_value_heads=1 if kind == "llama-kv1" else None,
                      dtype=dtype)
    return LlamaForCausalLM(cfg, device=device).eval()


_cache = {}


def model_and_prompt(kind):
    """One model and one random [2, 5] prompt per kind, shared and left unchanged."""
    if kind not in _cache:
        m = make_model(kind)
        ids = torch.randint(1, m.cfg.vocab_size, (2, 5))
        _cache[kind] = (m, ids)
    return _cache[kind]


@torch.no_grad()
def recompute_greedy(model, ids, steps):
    out = []
    for _ in range(steps):
        nxt = model(ids)[:, -1].float().argmax(-1)
        out.append(nxt)
        ids = torch.cat([ids, nxt[:, None]], 1)
    return torch.stack(out, 1)


@pytest.mark.parametrize("kind", MODELS)
def test_greedy_matches_recompute(kind):
    model, ids = model_and_prompt(kind)
    toks, lengths = model.generate(ids, 8, do_sample=False)
    assert toks.shape == (2, 8) and toks.dtype == torch.int64
    assert lengths.tolist() == [8, 8]
    assert torch.equal(toks, recompute_greedy(model, ids, 8))


@pytest.mark.parametrize("kind", MODELS)
def test_ragged_prompts(kind):
    model, _ = model_and_prompt(kind)
    g = torch.Generator().manual_seed(1)
    rows = [torch.randint(1, model.cfg.vocab_size, (n,), generator=g) for n in (3, 7)]
    padded = torch.zeros(2, 7, dtype=torch.long)
    for b, r in enumerate(rows):
        padded[b, : len(r)] = r
    toks, _ = model.generate(padded, 8, prompt_lens=[3, 7])
    for b, r in enumerate(rows):
        alone, _ = model.generate(r[None], 8)
        assert torch.equal(toks[b], alone[0]), f"row {b}"


@pytest.mark.parametrize("T", [1, 5])
def test_kv_append_reference(T):
    torch.manual_seed(0)
    B, Hq, Hk, D, S_max = 2, 4, 2, 16, 48
    pos = [0, 37]
    cos, sin = ops.rope_tables(64, D)
    cache = ops.KVCache(1, B, S_max, Hk, D, torch.float32, "cpu")
    sentinel = -7.5
    cache.k[0].fill_(sentinel)
    cache.v[0].fill_(sentinel)
    cache.set_lens(pos)
    qkv = torch.randn(B, T, (Hq + 2 * Hk) * D)
    q = ops.kv_append(qkv, cache, 0, Hq, Hk, cos, sin)
    x = qkv.view(B, T, Hq + 2 * Hk, D)
    assert q.shape == (B, T, Hq, D)
    for b in range(B):
        # _rope_ref rotates token t with table row t: hand it the rows pos[b] + t
        c, s = cos[pos[b]: pos[b] + T], sin[pos[b]: pos[b] + T]
        want_q = F._rope_ref(x[b: b + 1, :, :Hq], c, s)[0]
        want_k = F._rope_ref(x[b: b + 1, :, Hq:Hq + Hk], c, s)[0]
        assert (q[b] - want_q).abs().max().item() <= 1e-6
        assert (cache.k[0][b, pos[b]: pos[b] + T] - want_k).abs().max().item() <= 1e-6
        assert torch.equal(cache.v[0][b, pos[b]: pos[b] + T], x[b, :, Hq + Hk:])
        outside = torch.ones(S_max, dtype=torch.bool)
        outside[pos[b]: pos[b] + T] = False
        for t in (cache.k[0], cache.v[0]):
            assert torch.equal(t[b, outside], torch.full_like(t[b, outside], sentinel))
    assert cache.lens.tolist() == pos  # kv_append does not advance


def test_kv_append_overflow_raises():
    B, Hq, Hk, D = 2, 2, 2, 16
    cache = ops.KVCache(1, B, 40, Hk, D, torch.float32, "cpu")
    cache.set_lens([0, 37])
    ops.kv_append(torch.randn(B, 3, (Hq + 2 * Hk) * D), cache, 0, Hq, Hk)  # rows 37..39: fits
    with pytest.raises(ValueError):
        ops.kv_append(torch.randn(B, 4, (Hq + 2 * Hk) * D), cache, 0, Hq, Hk)
    cache.advance(3)
    with pytest.raises(ValueError):
        cache.advance(1)
    cache.reset()
    assert cache.lens.tolist() == [0, 0] and cache.bound == 0


def test_generate_guards():
    model, ids = model_and_prompt("llama")
    with pytest.raises(ValueError):
        model.generate(ids, model.cfg.max_position_embeddings)  # prompt + new tokens too long
    model.tp = object()
    try:
        with pytest.raises(NotImplementedError):
            model.generate(ids, 2)
    finally:
        model.tp = None


def test_sampling():
    model, ids = model_and_prompt("llama")
    kw = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.95)
    a, _ = model.generate(ids, 8, seed=123, **kw)
    b, _ = model.generate(ids, 8, seed=123, **kw)
    assert torch.equal(a, b)
    assert a.min().item() >= 0 and a.max().item() < model.cfg.vocab_size
    greedy, _ = model.generate(ids, 8)
    k1, _ = model.generate(ids, 8, do_sample=True, top_k=1, seed=5)
    assert torch.equal(k1, greedy)
    # EOS = row 0's first greedy token: row 0 stops at once and pads, row 1 is unaffected
    eos, pad = int(greedy[0, 0]), 3
    assert eos not in greedy[1].tolist(), "pick another seed: row 1 emits row 0's first token"
    toks, lengths = model.generate(ids, 8, eos_token_id=eos, pad_token_id=pad)
    assert lengths.tolist() == [1, 8]
    assert toks[0].tolist() == [eos] + [pad] * 7
    assert torch.equal(toks[1], greedy[1])
