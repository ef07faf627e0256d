"""Speculative decoding on the reference (CPU, fp32 / float64) paths: the three-word Philox,
losslessness of the accept / residual rule, the commit bookkeeping, ``rewind_each`` of both
caches, and ``generate(draft=...)`` against plain ``generate()`` on the tiny models."""
import copy
import math

import pytest
import torch
from scipy.stats import chi2

from paddle_amd import ops
from paddle_amd.models.speculative import SpeculativeDecoder
from paddle_amd.ops import sampling as S
from paddle_amd.ops import speculative as SP
from paddle_amd.models.gpt import GPTConfig, GPTForCausalLM
from test_generation_cpu import MODELS, make_model

SEED = 0x5EC0DE5EED


def test_philox_third_word_zero_is_the_samplers_philox():
    for seed, c0, row in [(0, 0, 0), (SEED, 5, 16), (2 ** 63 + 11, 2 ** 31 - 1, 300), (2 ** 32, 1, 3)]:
        assert SP.philox3_u(seed, c0, row, 0) == S.philox_u(seed, c0, row)
        assert SP.philox3_x0(seed, c0, row) == S.philox_x0(seed, c0, row)
    us = {SP.philox3_u(SEED, 3, 2, c2) for c2 in range(8)}
    assert len(us) == 8  # the third word matters


# ---------------------------------------------------------------------- losslessness
CFG = dict(temperature=0.8, top_k=5, top_p=0.9)
TRIALS = 4096
TARGET = [2.0, 0.5, 1.5, -1.0, 1.0, 0.0, -2.0, 0.8]
DRAFT = [0.3, 1.8, 1.2, 0.5, -0.5, 1.0, -1.0, -3.0]


def first_emitted(target_row, draft_row):
    """The first emitted token of TRIALS independent rounds (one candidate each, the row index
    is the Philox counter), and the number of accepted candidates."""
    t = torch.tensor(target_row).expand(TRIALS, 2, -1)
    d = torch.tensor(draft_row).expand(TRIALS, 1, -1)
    cand = ops.sample_tokens(d[:, 0], SEED, 1, True, **CFG)[:, None]
    accept, alt = ops.spec_judge(t, cand, d, SEED, 0, True, **CFG)
    return torch.where(accept[:, 0], cand[:, 0], alt[:, 0]), int(accept.sum())


def test_the_rule_is_lossless():
    V = len(TARGET)
    keep, c = S.reference_distribution(torch.tensor(TARGET), **CFG)
    p = torch.diff(c, prepend=torch.zeros(1, dtype=c.dtype))
    assert 1 < int(keep.sum()) < V and int((p > 0).sum()) == int(keep.sum())
    tok, accepted = first_emitted(TARGET, DRAFT)
    hist = torch.bincount(tok, minlength=V).double()
    assert hist[~keep].sum() == 0, "a token outside the target's survivor set was emitted"
    assert 0 < accepted < TRIALS  # both branches of the rule ran
    expect = p[keep] * TRIALS
    stat = float(((hist[keep] - expect) ** 2 / expect).sum())
    bound = float(chi2.ppf(1 - 1e-6, int(keep.sum()) - 1))
    print(f"chi-square {stat:.2f} at {int(keep.sum()) - 1} degrees of freedom (bound {bound:.1f}), "
          f"{accepted} of {TRIALS} accepted")
    assert stat < bound


def test_a_draft_equal_to_the_target_is_always_accepted():
    tok, accepted = first_emitted(TARGET, TARGET)
    assert accepted == TRIALS
    keep, _ = S.reference_distribution(torch.tensor(TARGET), **CFG)
    assert keep[tok].all()


def test_judge_edges_on_the_reference():
    V = 8
    t = torch.tensor(TARGET).expand(3, 3, V).clone()
    d = torch.tensor(DRAFT).expand(3, 2, V).clone()
    t[1] = float("nan")          # nothing to draw from: the greedy rule
    d[2] = float("-inf")         # Q is None: q is one-hot at the draft's greedy token, 0
    cand = torch.tensor([[-1, V], [0, 2 ** 40], [0, 3]])
    accept, alt = ops.spec_judge(t, cand, d, SEED, 2, True, **CFG)
    assert accept[0].tolist() == [False, False]
    assert accept[1].tolist() == [True, False] and alt[1].tolist() == [0, 0, 0]
    assert ((alt >= 0) & (alt < V)).all()
    # q one-hot at 0, p(0) > 0: accepted iff u < p(0); the residual never gives 0 again
    keep, c = S.reference_distribution(torch.tensor(TARGET), **CFG)
    assert bool(accept[2, 0]) == (SP.philox3_u(SEED, 2, 2, 1) < float(c[0]))
    assert int(alt[2, 0]) != 0 and not bool(accept[2, 1])  # p(3) = 0: rejected
    g_acc, g_alt = ops.spec_judge(t, cand, None, do_sample=False)
    assert g_alt[0].tolist() == [0, 0, 0] and g_acc.tolist() == [[False, False], [True, False], [True, False]]
    m, s = ops.spec_margins(t[:1], cand[2:3], d[:1], SEED, 2, True, **CFG)
    assert m.shape == (1, 2) and s.shape == (1, 2) and (s > 0).all()


# ---------------------------------------------------------------------- commit
G, MAX_NEW, EOS, PAD = 3, 8, 7, 9
# name, pos, done, accepted before | accept, cand, alt | out written, pos, done, lengths, kept, tok, accepted after
COMMIT_ROWS = [
    ("none rejected", 1, False, 0, [1, 1, 1], [1, 2, 3], [4, 4, 4, 5], [1, 2, 3, 5], 5, False, MAX_NEW, 4, 5, 3),
    ("rejected at 0", 1, False, 0, [0, 1, 1], [1, 2, 3], [6, 4, 4, 4], [6], 2, False, MAX_NEW, 1, 6, 0),
    ("eos accepted", 2, False, 1, [1, 1, 1], [1, EOS, 3], [4, 4, 4, 4], [1, EOS], 4, True, 4, 2, EOS, 3),
    ("eos replaces", 1, False, 0, [1, 0, 1], [1, 2, 3], [4, EOS, 4, 4], [1, EOS], 3, True, 3, 2, EOS, 1),
    ("cap mid-round", 6, False, 0, [1, 1, 1], [1, 2, 3], [4, 4, 4, 4], [1, 2], 8, True, MAX_NEW, 2, 2, 2),
    ("done row", 3, True, 2, [1, 1, 1], [1, 2, 3], [4, 4, 4, 4], [], 3, True, 5, 0, PAD, 2),
    ("rejected at 2", 0, False, 0, [1, 1, 0], [1, 2, 3], [4, 4, 6, 4], [1, 2, 6], 3, False, MAX_NEW, 3, 6, 2),
]


def commit_case(device):
    """(state before the commit, accept, alt, cand) of COMMIT_ROWS on ``device``."""
    B = len(COMMIT_ROWS)
    st = ops.SpecState(B, MAX_NEW, G, device, eos_token_id=EOS, pad_token_id=PAD)
    st.pos.copy_(torch.tensor([r[1] for r in COMMIT_ROWS], dtype=torch.int32))
    st.done.copy_(torch.tensor([r[2] for r in COMMIT_ROWS]))
    st.accepted.copy_(torch.tensor([r[3] for r in COMMIT_ROWS], dtype=torch.int32))
    st.lengths[5] = 5
    accept = torch.tensor([r[4] for r in COMMIT_ROWS], dtype=torch.bool, device=device)
    cand = torch.tensor([r[5] for r in COMMIT_ROWS], dtype=torch.long, device=device)
    alt = torch.tensor([r[6] for r in COMMIT_ROWS], dtype=torch.long, device=device)
    return st, accept, alt, cand


def check_commit(st):
    for b, (name, pos0, _, _, _, _, _, written, pos, done, length, kept, tok, accepted) in enumerate(COMMIT_ROWS):
        want = [PAD] * MAX_NEW
        want[pos0:pos0 + len(written)] = written
        assert st.out[b].tolist() == want, name
        got = (int(st.pos[b]), bool(st.done[b]), int(st.lengths[b]), int(st.kept[b]), int(st.tok[b]),
               int(st.accepted[b]))
        assert got == (pos, done, length, kept, tok, accepted), f"{name}: {got}"


def test_commit_bookkeeping():
    st, accept, alt, cand = commit_case("cpu")
    assert st.pos.dtype == st.kept.dtype == st.accepted.dtype == torch.int32
    assert ops.spec_commit(accept, alt, cand, st) is st.kept
    check_commit(st)


def test_sample_step_counts_the_first_token():
    st = ops.SpecState(2, 4, 2, "cpu", eos_token_id=1)
    logits = torch.zeros(2, 5)
    logits[0, 1] = logits[1, 3] = 1.0
    ops.sample_step(logits, st)
    assert st.pos.tolist() == [1, 1] and st.done.tolist() == [True, False] and st.tok.tolist() == [1, 3]
    with pytest.raises(ValueError):
        ops.SpecState(2, 4, 17, "cpu")


# ---------------------------------------------------------------------- rewind_each
def test_rewind_each_contiguous():
    Hq = Hk = 1
    D = 8
    cache = ops.KVCache(1, 3, 16, Hk, D, torch.float32, "cpu")
    cache.set_lens([5, 3, 4])
    for bad in ([1, 1], [-1, 0, 0], [6, 0, 0]):
        with pytest.raises(ValueError):
            cache.rewind_each(bad)
    with pytest.raises(ValueError):
        cache.rewind_each([1, 0, 0], bound=6)
    assert cache.lens.tolist() == [5, 3, 4] and cache.bound == 5
    cache.rewind_each([0, 0, 0])
    assert cache.lens.tolist() == [5, 3, 4] and cache.bound == 5
    cache.rewind_each([1, 0, 0])  # without bound= the host bound stays
    assert cache.lens.tolist() == [4, 3, 4] and cache.bound == 5
    cache.rewind_each(torch.tensor([1, 0, 2]), bound=3)
    assert cache.lens.tolist() == [3, 3, 2] and cache.bound == 3 and cache.lens.dtype == torch.int32
    cache.k[0].fill_(-7.5)
    qkv = torch.randn(3, 2, (Hq + 2 * Hk) * D)
    ops.kv_append(qkv, cache, 0, Hq, Hk)
    for b, n in enumerate([3, 3, 2]):
        assert torch.equal(cache.k[0][b, n:n + 2, 0], qkv[b, :, D:2 * D])
        assert (cache.k[0][b, :n] == -7.5).all() and (cache.k[0][b, n + 2:] == -7.5).all()


def test_rewind_each_paged():
    Hq = Hk = 1
    D = 8
    cache = ops.PagedKVCache(1, 3, 64, Hk, D, torch.float32, "cpu", block_size=16, num_blocks=8)
    cache.reserve([20, 3, 33])
    cache.set_lens([20, 3, 33])
    table, free, owned = cache.host_table, cache.free_blocks, [cache.row_blocks(r) for r in range(3)]
    dev_table = cache.block_table.clone()

    def unchanged():
        return (torch.equal(cache.host_table, table) and cache.free_blocks == free
                and [cache.row_blocks(r) for r in range(3)] == owned and torch.equal(cache.block_table, dev_table))

    for bad in ([1, 1], [-1, 0, 0], [0, 4, 0], [21, 0, 0]):
        with pytest.raises(ValueError):
            cache.rewind_each(bad)
    with pytest.raises(ValueError):
        cache.rewind_each([4], rows=[1])
    assert cache.host_lens == [20, 3, 33] and cache.lens.tolist() == [20, 3, 33] and unchanged()
    cache.rewind_each([5, 0, 2])  # row 0 falls back into its first block and keeps the second
    assert cache.host_lens == [15, 3, 31] and cache.lens.tolist() == [15, 3, 31] and cache.bound == 31 and unchanged()
    cache.rewind_each([3], rows=[2])
    assert cache.host_lens == [15, 3, 28] and cache.lens.tolist() == [15, 3, 28] and cache.bound == 28 and unchanged()
    qkv = torch.randn(3, 2, (Hq + 2 * Hk) * D)
    ops.kv_append(qkv, cache, 0, Hq, Hk)
    k, _ = cache.gather(0)
    for b, n in enumerate([15, 3, 28]):
        assert torch.equal(k[b, n:n + 2, 0], qkv[b, :, D:2 * D])
    assert unchanged()  # the kept blocks took the new tokens


# ---------------------------------------------------------------------- models
PROMPT_LENS = [3, 7, 5]
NEW = 24
SIGMA = {"llama": 1e-3, "llama-kv1": 1e-3, "gpt": 3e-3}  # the noise at which some, not all, proposals survive

_models = {}


def setup(kind):
    """(model, prompt, plain tokens, plain lengths) per kind, shared and left unchanged."""
    if kind not in _models:
        m = make_model(kind)
        g = torch.Generator().manual_seed(1)
        ids = torch.zeros(len(PROMPT_LENS), max(PROMPT_LENS), dtype=torch.long)
        for b, n in enumerate(PROMPT_LENS):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        toks, lengths = m.generate(ids, NEW, prompt_lens=PROMPT_LENS)
        _models[kind] = (m, ids, toks, lengths)
    return _models[kind]


def perturbed(model, sigma, seed=5):
    d = copy.deepcopy(model)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in d.parameters():
            p.add_(torch.randn(p.shape, generator=g) * sigma)
    return d


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
@pytest.mark.parametrize("kind", MODELS)
def test_greedy_tokens_equal_plain_generation(kind, cache):
    m, ids, want, want_len = setup(kind)
    exact, noisy = copy.deepcopy(m), perturbed(m, SIGMA[kind])
    for nd in (1, 4, 7):
        got, lengths = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, cache=cache, draft=exact, num_draft=nd)
        s = m.last_speculation
        assert isinstance(s, SpeculativeDecoder) and s.num_draft == nd
        assert torch.equal(got, want) and torch.equal(lengths, want_len)
        assert s.accepted == s.proposed > 0 and s.rounds == math.ceil((NEW - 1) / (nd + 1))
        assert s.emitted == NEW * len(PROMPT_LENS)
        got, lengths = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, cache=cache, draft=noisy, num_draft=nd)
        assert torch.equal(got, want) and torch.equal(lengths, want_len)
        if nd == 4:
            s = m.last_speculation
            assert 0 < s.accepted < s.proposed, (s.accepted, s.proposed)


@pytest.mark.parametrize("kind", MODELS)
def test_an_unrelated_draft_changes_nothing(kind):
    m, ids, want, want_len = setup(kind)
    torch.manual_seed(77)
    other = type(m)(m.cfg, device="cpu").eval()
    got, lengths = SpeculativeDecoder(m, other, 4).generate(ids, NEW, prompt_lens=PROMPT_LENS)
    assert torch.equal(got, want) and torch.equal(lengths, want_len)


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
def test_eos_mid_sequence(cache):
    m, ids, plain, _ = setup("llama")
    eos, pad = int(plain[1, 9]), 3
    want, want_len = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, eos_token_id=eos, pad_token_id=pad)
    assert want_len.min() < NEW
    got, lengths = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, eos_token_id=eos, pad_token_id=pad, cache=cache,
                              draft=perturbed(m, SIGMA["llama"]), num_draft=4)
    assert torch.equal(got, want) and torch.equal(lengths, want_len)
    assert m.last_speculation.emitted == int(want_len.sum())


E4M3_EQUAL_ON_CPU = True  # what the check below finds on the fp32 reference path


def test_fp8_cache_and_quantised_weights():
    m, ids, _, _ = setup("llama")
    noisy = perturbed(m, SIGMA["llama"])
    # an e4m3 cache: extend attends to quantised keys of its own chunk where decode_step attends to
    # them one at a time, the same values on the CPU reference -- checked here, asserted since it holds
    want, _ = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, kv_dtype="fp8_e4m3")
    got, _ = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, kv_dtype="fp8_e4m3", draft=noisy, num_draft=4)
    same = torch.equal(got, want)
    print(f"e4m3 cache: speculative tokens equal the plain e4m3 run's: {same}")
    if E4M3_EQUAL_ON_CPU:
        assert same
    assert ((got >= 0) & (got < m.cfg.vocab_size)).all()
    q = copy.deepcopy(m).quantize_weights()
    want, want_len = q.generate(ids, NEW, prompt_lens=PROMPT_LENS)
    got, lengths = q.generate(ids, NEW, prompt_lens=PROMPT_LENS, draft=copy.deepcopy(noisy).quantize_weights(),
                              num_draft=4)
    assert torch.equal(got, want) and torch.equal(lengths, want_len)
    got, lengths = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, draft=q, num_draft=4, prefill_chunk=3)
    _, _, plain, plain_len = setup("llama")
    assert torch.equal(got, plain) and torch.equal(lengths, plain_len)


def test_sampled_mode():
    m, ids, _, _ = setup("llama")
    noisy = perturbed(m, SIGMA["llama"])
    kw = dict(prompt_lens=PROMPT_LENS, do_sample=True, temperature=0.9, top_k=50, top_p=0.95, draft=noisy, num_draft=4)
    a, _ = m.generate(ids, NEW, seed=123, **kw)
    s = m.last_speculation
    assert 0 < s.accepted <= s.proposed and s.emitted == NEW * len(PROMPT_LENS)
    b, _ = m.generate(ids, NEW, seed=123, **kw)
    c, _ = m.generate(ids, NEW, seed=124, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.min().item() >= 0 and a.max().item() < m.cfg.vocab_size
    k1, _ = m.generate(ids, NEW, prompt_lens=PROMPT_LENS, do_sample=True, top_k=1, seed=5, draft=noisy, num_draft=3)
    assert torch.equal(k1, setup("llama")[2])  # top-k 1 leaves the greedy token alone


def test_guards():
    m, ids, _, _ = setup("llama")
    d = copy.deepcopy(m)
    other = GPTForCausalLM(GPTConfig(vocab_size=m.cfg.vocab_size + 1, hidden_size=64, num_hidden_layers=1,
                                     num_attention_heads=2, max_position_embeddings=128, dtype="float32")).eval()
    for kw in (dict(draft=other), dict(draft=d, num_draft=0), dict(draft=d, num_draft=17), dict(draft=d, graph=True),
               dict(draft=d, sampler="torch"), dict(draft=d, cache="ring"), dict(draft=d, block_size=16)):
        with pytest.raises(ValueError):
            m.generate(ids, 4, **kw)
    room = m.cfg.max_position_embeddings - ids.shape[1]
    m.generate(ids[:1], 2, draft=d, num_draft=2)
    with pytest.raises(ValueError):  # the candidates need positions of their own
        m.generate(ids, room - 3, draft=d, num_draft=4)
    d.tp = object()
    with pytest.raises(NotImplementedError):
        m.generate(ids, 4, draft=d)
    one, _ = m.generate(ids, 1, prompt_lens=PROMPT_LENS, draft=copy.deepcopy(m))
    assert torch.equal(one, setup("llama")[2][:, :1]) and m.last_speculation.rounds == 0
