"""``DecodeGraph`` / ``generate(graph=True)`` on the GPU: a replayed step gives the bits of the
launch loop (tokens, lengths, logits), the host mirrors follow the device, the paged table
stays constant with no upload, and the graph is replayed, not re-launched."""
import contextlib

import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import skinny
from test_generation_cpu import make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
KINDS = ["llama", "llama-kv1", "gpt", "llama-fp8"]
NEW = 12
_models = {}


def model_of(kind):
    """One bf16 model per kind on the GPU ("llama-fp8": quantised weights), shared, unchanged."""
    if kind not in _models:
        m = make_model(kind.replace("-fp8", ""), dev, "bfloat16")
        _models[kind] = m.quantize_weights() if kind.endswith("-fp8") else m
    return _models[kind]


def prompts(model, B, S=7, lens=(3, 7, 5)):
    g = torch.Generator().manual_seed(3)
    ids = torch.zeros(B, S, dtype=torch.long)
    lens = [min(n, S) for n in lens[:B]] if S == 7 else [S] * B
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, model.cfg.vocab_size, (n,), generator=g)
    return ids.to(dev), lens


class count_calls:
    """Counts the calls of ``owner.name`` while active."""

    def __init__(self, owner, name):
        self.owner, self.name = owner, name

    def __enter__(self):
        self.n = 0
        self._orig = getattr(self.owner, self.name)

        def wrapped(*a, **k):
            self.n += 1
            return self._orig(*a, **k)

        setattr(self.owner, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self._orig)


def run_loop(model, ids, lens, paged, how, n_steps):
    """Prefill + one eager sample_step, then n_steps of the launch loop; (state, cache, logits)."""
    B, S = ids.shape
    kw = dict(paged=True, block_size=16) if paged else {}
    cache = model.init_cache(B, S + NEW, **kw)
    st = ops.SamplerState(B, NEW, dev)
    ops.sample_step(model.prefill(ids, cache, lens), st, *how)
    logits = None
    for _ in range(n_steps):
        logits = model.decode_step(st.tok, cache)
        ops.sample_step(logits, st, *how)
    return st, cache, logits


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_replay_equals_the_launch_loop(kind, B, paged):
    """Greedy and sampled: tokens, lengths and the last logits bit-equal to the launch loop;
    host mirrors == device lengths == prompt lengths + n + 1 after every replay; no table
    upload and no skinny launch outside the capture.  The paged case feeds a 13-token prompt
    with 16-token blocks, so rows cross a block boundary inside the replayed range."""
    model = model_of(kind)
    ids, lens = prompts(model, B, 13) if paged else prompts(model, B)
    S = ids.shape[1]
    for how in ((0, False, 1.0, 0, 1.0), (77, True, 0.9, 50, 0.95)):
        want, _, want_logits = run_loop(model, ids, lens, paged, how, NEW - 1)
        kw = dict(paged=True, block_size=16) if paged else {}
        cache = model.init_cache(B, S + NEW, **kw)
        st = ops.SamplerState(B, NEW, dev)
        ops.sample_step(model.prefill(ids, cache, lens), st, *how)
        if paged:
            cache.reserve(NEW - 1)  # what decode_graph reserves: the spy then sees the capture and the replays only
        uploads = count_calls(cache, "_upload_table") if paged else contextlib.nullcontext()
        with uploads:
            with count_calls(skinny, "_launch") as captured:
                g = model.decode_graph(cache, st, NEW - 1, *how)
            assert captured.n > 0
            assert cache.lens.tolist() == lens and cache.bound == max(lens)  # capture moved nothing
            table = cache.block_table.clone() if paged else None
            with count_calls(skinny, "_launch") as replayed:
                for n in range(NEW - 1):
                    g.step()
                    dev_lens = cache.lens.tolist()
                    assert dev_lens == [x + n + 1 for x in lens] and cache.bound == max(dev_lens)
                    if paged:
                        assert cache.host_lens == dev_lens
            assert replayed.n == 0 and g.replays == NEW - 1
            if paged:
                assert uploads.n == 0
                assert torch.equal(cache.block_table, table) and torch.equal(cache.host_table.to(dev), table)
        assert torch.equal(st.out, want.out), how
        assert torch.equal(st.lengths, want.lengths) and int(st.step) == NEW
        assert torch.equal(g.logits, want_logits), how


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
@pytest.mark.parametrize("kind", KINDS)
def test_generate_graph(kind, cache):
    model = model_of(kind)
    ids, lens = prompts(model, 3)
    kw = dict(prompt_lens=lens, cache=cache)
    want, want_len = model.generate(ids, NEW, **kw)  # today's path: launch loop + sample_next
    a, la = model.generate(ids, NEW, graph=True, **kw)
    b, lb = model.generate(ids, NEW, graph=True, **kw)  # a second capture in the same process
    assert torch.equal(a, want) and torch.equal(la, want_len)
    assert torch.equal(b, want) and torch.equal(lb, want_len)
    eos, pad = int(want[0, 2]), 3
    kw.update(eos_token_id=eos, pad_token_id=pad)
    want, want_len = model.generate(ids, NEW, **kw)
    a, la = model.generate(ids, NEW, graph=True, **kw)
    assert torch.equal(a, want) and torch.equal(la, want_len) and int(la[0]) <= 3
    kw.update(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, seed=5)
    a, la = model.generate(ids, NEW, graph=True, **kw)
    b, lb = model.generate(ids, NEW, sampler="philox", **kw)
    assert torch.equal(a, b) and torch.equal(la, lb)
    with pytest.raises(ValueError):
        model.generate(ids, NEW, graph=True, sampler="torch")


def test_overflow_raises_before_the_replay():
    model = model_of("llama")
    ids, lens = prompts(model, 3)
    cache = model.init_cache(3, 7 + 3)
    st = ops.SamplerState(3, NEW, dev)
    ops.sample_step(model.prefill(ids, cache, lens), st)
    g = model.decode_graph(cache, st)
    for _ in range(3):
        g.step()
    before = (cache.lens.clone(), st.out.clone(), int(st.step))
    with pytest.raises(ValueError, match="overflow"):
        g.step()
    assert torch.equal(cache.lens, before[0]) and cache.bound == 10
    assert torch.equal(st.out, before[1]) and int(st.step) == before[2]


def test_undersized_pool_raises_at_decode_graph():
    model = model_of("llama")
    ids, lens = prompts(model, 3)
    cache = model.init_cache(3, 40, paged=True, block_size=16, num_blocks=3)  # one block per row
    st = ops.SamplerState(3, 16, dev)
    ops.sample_step(model.prefill(ids, cache, lens), st)
    free, table, hl = cache.free_blocks, cache.host_table, cache.host_lens
    dev_table, dev_lens = cache.block_table.clone(), cache.lens.clone()
    with pytest.raises(ValueError, match="out of blocks"):
        model.decode_graph(cache, st, 16)  # row 1 would need a second block
    assert cache.free_blocks == free and torch.equal(cache.host_table, table) and cache.host_lens == hl
    assert torch.equal(cache.block_table, dev_table) and torch.equal(cache.lens, dev_lens)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_stale_graph_raises(paged):
    model = model_of("llama")
    ids, lens = prompts(model, 3)
    cache = model.init_cache(3, 7 + NEW, **(dict(paged=True, block_size=16) if paged else {}))
    st = ops.SamplerState(3, NEW, dev)
    ops.sample_step(model.prefill(ids, cache, lens), st)
    g = model.decode_graph(cache, st)
    g.step()
    if paged:
        cache.free_rows([1])
    else:
        cache.reset()
    with pytest.raises(RuntimeError):
        g.step()
