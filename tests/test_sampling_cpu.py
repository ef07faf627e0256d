"""The sampling contract on its float64 reference (ops/sampling.py): the Philox uniform, the
filters against today's ``sample_next``, ties, degenerate rows and the ``sample_step``
bookkeeping against the loop body of ``generate()``."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.models.generation import filter_logits
from paddle_amd.ops import sampling as S


# ---------------------------------------------------------------------- Philox
def test_philox_known_answers():
    # Random123's known-answer vectors for philox4x32-10 (first output word)
    assert S.philox_x0(0, 0, 0) == 0x6627E8D5
    assert _philox_full(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == 0x408F276D
    assert _philox_full(0x299F31D0A4093822, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344) == 0xD16CFE09


def _philox_full(seed, c0, c1, c2, c3):
    """philox4x32-10 with a full counter, written independently of ops/sampling.py."""
    M = 0xFFFFFFFF
    k0, k1 = seed & M, seed >> 32
    x = [c0, c1, c2, c3]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x[0], 0xCD9E8D57 * x[2]
        x = [(p1 >> 32) ^ x[1] ^ k0, p1 & M, (p0 >> 32) ^ x[3] ^ k1, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return x[0]


def test_philox_matches_full_counter_form():
    for seed, step, row in [(0, 0, 0), (1, 2, 3), (2 ** 63 + 5, 77, 15), (2 ** 64 - 1, 2 ** 31 - 1, 1000)]:
        assert S.philox_x0(seed, step, row) == _philox_full(seed, step, row, 0, 0)


def test_philox_uniform_properties():
    u = ops.philox_uniform(7, 3, 64, "cpu")
    assert u.dtype == torch.float32 and u.shape == (64,)
    assert torch.equal(u, ops.philox_uniform(7, 3, 64, "cpu"))  # deterministic
    assert 0.0 <= float(u.min()) and float(u.max()) < 1.0
    assert len(set(u.tolist())) == 64  # differs per row
    assert not torch.equal(u, ops.philox_uniform(7, 4, 64, "cpu"))  # per step
    assert not torch.equal(u, ops.philox_uniform(8, 3, 64, "cpu"))  # per seed
    # the high seed word is part of the key
    assert not torch.equal(u, ops.philox_uniform(7 + 2 ** 32, 3, 64, "cpu"))
    assert torch.equal(ops.philox_uniform(7 + 2 ** 64, 3, 4, "cpu"), ops.philox_uniform(7, 3, 4, "cpu"))
    # u = (x0 >> 8) * 2^-24, and a step given as a tensor is the same step
    assert float(u[5]) == (S.philox_x0(7, 3, 5) >> 8) * 2.0 ** -24
    assert torch.equal(ops.philox_uniform(7, torch.tensor([3], dtype=torch.int32), 64, "cpu"), u)
    worst = max(S.philox_u(s, t, r) for s in range(4) for t in range(50) for r in range(16))
    assert worst < 1.0


# ---------------------------------------------------------------------- filters
@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 40, 0.8),
                                                      (0.9, 1, 1.0), (1.0, 0, 0.05)])
def test_survivors_match_sample_next(temperature, top_k, top_p):
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(6, 1003, generator=g, dtype=torch.float64).float() * 3  # fp32 randn: no ties
    assert all(r.unique().numel() == r.numel() for r in logits)
    want = torch.isfinite(filter_logits(logits, temperature, top_k, top_p))
    for b in range(logits.shape[0]):
        keep, c = S.reference_distribution(logits[b], temperature, top_k, top_p)
        assert torch.equal(keep, want[b]), f"row {b}"
        assert abs(float(c[-1]) - 1.0) < 1e-12
        # the draw is the first index whose running sum passes u, in index order
        for u in (0.0, 0.25, 0.999999):
            i = S.reference_pick((keep, c), u)
            assert keep[i] and c[i] > u and (i == 0 or c[i - 1] <= u)


def test_greedy_lowest_index_among_maxima():
    x = torch.tensor([[1.0, 5.0, 2.0, 5.0, 5.0], [3.0, 3.0, 3.0, 3.0, 3.0], [-0.0, 0.0, -1.0, 0.0, -2.0]])
    assert ops.sample_tokens(x).tolist() == [1, 0, 0]
    assert ops.sample_tokens(x.bfloat16()).tolist() == [1, 0, 0]


def test_top_k_ties_at_kth_value_all_kept():
    x = torch.tensor([4.0, 2.0, 3.0, 2.0, 1.0, 2.0, 0.0])
    keep, _ = S.reference_distribution(x, top_k=3)  # the 3rd largest is 2.0, three of them
    assert keep.tolist() == [True, True, True, True, False, True, False]
    keep, _ = S.reference_distribution(x, top_k=2)
    assert keep.tolist() == [True, False, True, False, False, False, False]


def test_top_p_ties_go_together():
    # p = [.4, .2, .2, .1, .1]: the mass strictly above the two .2s is .4
    x = torch.log(torch.tensor([0.4, 0.2, 0.2, 0.1, 0.1], dtype=torch.float64))
    x[2] = x[1]
    x[4] = x[3]
    assert S.reference_distribution(x, top_p=0.5)[0].tolist() == [True, True, True, False, False]
    assert S.reference_distribution(x, top_p=0.4 - 1e-9)[0].tolist() == [True, False, False, False, False]
    assert S.reference_distribution(x, top_p=0.85)[0].tolist() == [True] * 5
    assert S.reference_distribution(x, top_p=0.8 - 1e-9)[0].tolist() == [True, True, True, False, False]
    # the maximum always stays, ties at the maximum included
    y = torch.tensor([1.0, 3.0, 3.0, 0.0])
    assert S.reference_distribution(y, top_p=0.0)[0].tolist() == [False, True, True, False]


def test_noop_filters_and_single_token_vocabulary():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(257, generator=g)
    base = S.reference_distribution(x)
    for kw in (dict(top_k=257), dict(top_k=1000), dict(top_p=1.0), dict(top_k=0, top_p=1.0)):
        keep, c = S.reference_distribution(x, **kw)
        assert keep.all() and torch.equal(c, base[1])
    one = torch.tensor([[0.3], [float("-inf")], [float("nan")]])
    assert ops.sample_tokens(one).tolist() == [0, 0, 0]
    assert ops.sample_tokens(one, seed=1, step=2, do_sample=True, top_k=5, top_p=0.5).tolist() == [0, 0, 0]


def test_degenerate_rows_give_a_token_in_range():
    V = 33
    ninf, nan, inf = float("-inf"), float("nan"), float("inf")
    rows = torch.zeros(6, V)
    rows[0].fill_(ninf)
    rows[1].fill_(nan)
    rows[2] = torch.arange(V).float()
    rows[2, 7] = nan  # a NaN counts as -inf
    rows[3].fill_(ninf)
    rows[3, 20] = 1.0  # one survivor
    rows[4, 11] = inf
    rows[5, 5] = nan
    rows[5, 6] = ninf
    for kw in (dict(), dict(do_sample=True), dict(do_sample=True, top_k=4, top_p=0.5, temperature=1e-9)):
        for step in range(8):
            t = ops.sample_tokens(rows, seed=3, step=step, **kw)
            assert t.dtype == torch.int64 and ((t >= 0) & (t < V)).all()
            assert t[0] == 0 and t[1] == 0 and t[3] == 20 and t[4] == 11
            assert t[2] != 7 and t[5] not in (5, 6)


def test_draw_depends_on_the_row_alone():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(4, 300, generator=g)
    b = a.clone()
    b[[0, 1, 3]] = torch.randn(3, 300, generator=g)
    kw = dict(seed=9, step=4, do_sample=True, top_k=20, top_p=0.9)
    assert ops.sample_tokens(a, **kw)[2] == ops.sample_tokens(b, **kw)[2]


# ---------------------------------------------------------------------- sample_step
def test_sample_step_reproduces_the_generate_loop():
    B, V, T, eos, pad = 3, 17, 6, 4, 9
    g = torch.Generator().manual_seed(0)
    script = torch.randn(T, B, V, generator=g)
    script[:, :, eos] = -50.0  # EOS only where planted
    script[2, 1, eos] = 50.0  # row 1 emits EOS at step 2
    script[4, 1, eos] = 50.0  # ... and again when it is done already: stays pad, length stays
    script[5, 0, eos] = 50.0  # row 0 at the last step
    # the loop body of generate(), greedy
    out = torch.full((B, T), pad, dtype=torch.long)
    lengths = torch.full((B,), T, dtype=torch.long)
    done = torch.zeros(B, dtype=torch.bool)
    st = ops.SamplerState(B, T, "cpu", eos_token_id=eos, pad_token_id=pad)
    assert st.tok.dtype == st.out.dtype == st.lengths.dtype == torch.int64 and st.step.dtype == torch.int32
    for step in range(T):
        nxt = script[step].argmax(-1)
        nxt = torch.where(done, torch.full_like(nxt, pad), nxt)
        out[:, step] = nxt
        hit = (nxt == eos) & ~done
        lengths = torch.where(hit, torch.full_like(lengths, step + 1), lengths)
        done = done | hit
        tok = ops.sample_step(script[step], st)
        assert tok is st.tok and torch.equal(st.tok, nxt)
        assert int(st.step) == step + 1
        assert torch.equal(st.out, out) and torch.equal(st.lengths, lengths) and torch.equal(st.done, done)
    assert lengths.tolist() == [6, 3, 6] and out[1].tolist()[2:] == [eos, pad, pad, pad]
    # without an EOS nothing is ever done
    st = ops.SamplerState(B, T, "cpu")
    for step in range(T):
        ops.sample_step(script[step], st, seed=1, do_sample=True, top_k=5)
    assert not st.done.any() and st.lengths.tolist() == [T] * B
    assert torch.equal(st.out[:, 3], ops.sample_tokens(script[3], seed=1, step=3, do_sample=True, top_k=5))
