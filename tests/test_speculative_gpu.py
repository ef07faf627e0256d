"""The speculative-decoding kernels (csrc/kernels/spec_verify.hip) against the float64
reference of ops/speculative.py, ``rewind_each`` on the device, and ``generate(draft=...)`` in
bf16.

Judge.  The logits are the rows of ``test_sampling_gpu.make_logits`` (planted ties included);
position (b, j) takes row ``(b * (G + 1) + j) % ROWS`` as the target's logits and the same row
plus seeded noise as the draft's, so the reference distributions are computed once per row.
Candidates come half from the draft's distribution and half uniform.  ``TOL`` is
``test_sampling_gpu``'s (derived there): an accept decision must equal the oracle's wherever
``|u q(d) - p(d)| > TOL`` (and where ``p(d) = q(d) = 0``: the survivor sets are exact, so that
is a rejection on the device too); a drawn token must lie in the target's survivor set and inside the
oracle's running-sum interval, widened by ``2 * TOL / sum(r)`` for a residual draw (two
distributions' errors, in units of the residual's mass) and by ``TOL`` for a draw from P.  The
inputs are chosen, and asserted on the CPU side, so that every top-p margin exceeds 1e-4,
every residual of V >= 7 has ``sum(r) >= 0.05`` and at most 1 % of the decisions and draws lie
within the tolerance of flipping; those are still checked, with the widened rule.

Models.  ``extend`` and ``decode_step`` use different arithmetic, so speculative and plain bf16
tokens may part where two logits are close.  ``e`` is the largest logit error of GPU
``extend(all_logits=True)`` against the fp32 CPU copy over prompt + plain tokens; a row is
compared with the plain tokens up to its first difference, where the CPU copy's logits of the
two tokens may differ by at most ``4 e`` (both are argmaxes of logits within ``2 e`` each)."""
import copy
import itertools

import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import sampling as S
from paddle_amd.ops import speculative as SP

import test_sampling_gpu as TS
import test_speculative_cpu as TC
from test_generation_cpu import make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
TOL = TS.TOL
CONFIGS = TS.CONFIGS
SEED = 0x77C0FFEE1234
ROUND = 5
NOISE = 1.0
MIN_SUM_R = 0.05
PAD = 3
SENTINEL = -12345


# ---------------------------------------------------------------------- inputs and oracle
_rows = {}


def logit_rows(V, dtype):
    """(target rows [ROWS, V], draft rows [ROWS, V], per configuration and row (P, Q)) for the
    vocabulary in use, values exact in ``dtype``.  A draft row is drawn again while its top-p
    decision is within 2 * MARGIN of flipping or (V >= 7) some configuration's residual
    ``sum(max(p - q, 0))`` is below MIN_SUM_R."""
    key = (V, dtype)
    if key not in _rows:
        _rows.clear()
        x = TS.make_logits(V, dtype)
        g = torch.Generator().manual_seed(2000 + V)
        drafts, dists = [], [[] for _ in CONFIGS]
        for i in range(TS.ROWS):
            P = [S.reference_distribution(x[i], **cfg) for cfg in CONFIGS]
            for _ in range(200):
                r = (x[i] + torch.randn(V, generator=g) * NOISE).to(dtype).float()
                if not TS._margin_ok(r):
                    continue
                Q = [S.reference_distribution(r, **cfg) for cfg in CONFIGS]
                assert all(d is not None for d in P + Q)
                if V < 7 or min(float((SP._probs(x[i], p, cfg["temperature"]) - SP._probs(r, q, cfg["temperature"]))
                                      .clamp(min=0).sum()) for p, q, cfg in zip(P, Q, CONFIGS)) >= 2 * MIN_SUM_R:
                    break
            else:
                raise AssertionError(f"V={V} row {i}: no draft row with a residual of {2 * MIN_SUM_R}: "
                                     "choose another seed")
            drafts.append(r)
            for ci in range(len(CONFIGS)):
                dists[ci].append((P[ci], Q[ci]))
        y = torch.stack(drafts)
        for cfg in CONFIGS:
            if cfg["top_p"] < 1.0:
                worst = min(S.reference_top_p_margin(r, **cfg) for r in list(x) + list(y))
                assert worst > TS.MARGIN, f"V={V} {cfg}: top-p margin {worst:.2e}: choose another seed"
        _rows[key] = (x, y, dists)
    return _rows[key]


def row_of(b, j, G):
    return (b * (G + 1) + j) % TS.ROWS


def candidates(V, dtype, B, G, ci):
    """[B, G] int64: position n = b * G + j draws from the draft's distribution (n even) or
    uniformly (n odd), in both cases among the tokens whose accept test is more than 10 * TOL
    from flipping or has ``p = q = 0``: at a large V nearly every token has two tiny
    probabilities, and a test between those is within TOL whatever its outcome."""
    x, y, dists = logit_rows(V, dtype)
    T = CONFIGS[ci]["temperature"]
    g = torch.Generator().manual_seed(3000 + V + 17 * G + ci)
    cand = torch.empty(B, G, dtype=torch.long)
    for b in range(B):
        for j in range(G):
            i = row_of(b, j, G)
            p, q = SP._probs(x[i], dists[ci][i][0], T), SP._probs(y[i], dists[ci][i][1], T)
            ua = SP.philox3_u(SEED, ROUND, b, 2 * j + 1)
            clear = ((ua * q - p).abs() > 10 * TOL) | ((p == 0) & (q == 0))
            assert clear.any()
            u = float(torch.rand((), generator=g, dtype=torch.float64))
            if (b * G + j) % 2 == 0:
                w = torch.where(clear, q, torch.zeros_like(q))
                c = (w / w.sum()).cumsum(0)
                cand[b, j] = min(int(torch.searchsorted(c, torch.tensor(u, dtype=c.dtype), right=True)), V - 1)
            else:
                idx = clear.nonzero().flatten()
                cand[b, j] = idx[min(int(u * idx.numel()), idx.numel() - 1)]
    return cand


def oracle(V, dtype, B, G, ci, cand, do_sample=True):
    x, y, dists = logit_rows(V, dtype)
    recs = []
    for b in range(B):
        for j in range(G + 1):
            i = row_of(b, j, G)
            recs.append(SP.reference_judge_one(
                x[i], y[i], 0 if j == G else cand[b, j], SP.philox3_u(SEED, ROUND, b, 2 * j + 1),
                SP.philox3_u(SEED, ROUND, b, 2 * j + 2), do_sample, last=j == G, dists=dists[ci][i], **CONFIGS[ci]))
    return recs


def padded(rows, B, T, dtype):
    """rows [B, T, V] as device logits of ``dtype`` with a position stride of V + PAD and a row
    stride of T * (V + PAD) + 1, NaN in the padding: rows start at every misalignment."""
    V = rows.shape[-1]
    rs = T * (V + PAD) + 1
    buf = torch.full((B * rs + 8,), float("nan"), dtype=dtype, device=dev)
    view = buf[1:1 + B * rs].view(B, rs)[:, :T * (V + PAD)].view(B, T, V + PAD)[:, :, :V]
    view.copy_(rows.to(dev, dtype))
    return view


def device_inputs(V, dtype, B, G):
    x, y, _ = logit_rows(V, dtype)
    ti = torch.tensor([[row_of(b, j, G) for j in range(G + 1)] for b in range(B)])
    return padded(x[ti], B, G + 1, dtype), padded(y[ti[:, :G]], B, G, dtype)


def outputs(B, G):
    """(accept, alt) inside sentinel-filled allocations, and the check that those are intact."""
    abuf = torch.full((B * G + 128,), 7, dtype=torch.uint8, device=dev)
    lbuf = torch.full((B * (G + 1) + 128,), SENTINEL, dtype=torch.long, device=dev)
    accept = abuf[64:64 + B * G].view(torch.bool).view(B, G)
    alt = lbuf[64:64 + B * (G + 1)].view(B, G + 1)

    def intact():
        return bool((abuf[:64] == 7).all() and (abuf[64 + B * G:] == 7).all() and (lbuf[:64] == SENTINEL).all()
                    and (lbuf[64 + B * (G + 1):] == SENTINEL).all())

    return (accept, alt), intact


def check_sampled(recs, accept, alt, V, dtype, B, G, ci):
    """The sampled judge's outputs against the oracle's records; returns (near, total): the
    decisions and draws within the tolerance of flipping, and all of them."""
    near = total = 0
    what = f"V={V} {CONFIGS[ci]}"
    dists = logit_rows(V, dtype)[2][ci]
    for b in range(B):
        for j in range(G + 1):
            r = recs[b * (G + 1) + j]
            a = int(alt[b, j])
            assert 0 <= a < V, f"{what} ({b}, {j}): alt {a}"
            u2 = SP.philox3_u(SEED, ROUND, b, 2 * j + 2)
            if j < G:
                total += 1
                if V >= 7:
                    assert r["sum_r"] >= MIN_SUM_R, f"{what} ({b}, {j}): sum(r) = {r['sum_r']:.3f}: choose other inputs"
                if r["margin"] is not None and (r["margin"] > TOL or r["p_d"] == r["q_d"] == 0.0):
                    assert bool(accept[b, j]) == r["accept"], f"{what} ({b}, {j}): accept, margin {r['margin']:.2e}"
                else:
                    near += 1
            keep_p = dists[row_of(b, j, G)][0][0]
            assert keep_p[a], f"{what} ({b}, {j}): alt {a} is outside the target's survivor set"
            w = 2 * TOL / r["sum_r"] if r["kind"] == "residual" else TOL
            c = r["c"]
            lo, hi = (float(c[a - 1]) if a else 0.0), float(c[a])
            assert lo - w <= u2 < hi + w, f"{what} ({b}, {j}): alt {a} [{lo}, {hi}) for u' = {u2} ({r['kind']})"
            total += 1
            ends = torch.cat([torch.zeros(1, dtype=c.dtype), c])
            near += int(((ends - u2).abs() <= w).any())
    return near, total


CASES = [(V, dt, 3, G) for V, dt, G in itertools.product([1, 7, 1003, 50257], TS.DTYPES, [1, 4, 16])]
CASES += [(131072, dt, 1, 1) for dt in TS.DTYPES]


@pytest.mark.parametrize("V,dtype,B,G", CASES, ids=[f"V{V}-{str(dt)[6:]}-B{B}-G{G}" for V, dt, B, G in CASES])
def test_judge_against_the_reference(V, dtype, B, G):
    x, y, _ = logit_rows(V, dtype)
    tl, dl = device_inputs(V, dtype, B, G)
    assert tl.stride(1) == V + PAD and SP.spec_kernel_ok(tl, dl, True) and SP.spec_kernel_ok(tl)
    # greedy: exact, the planted ties included; the candidates are the greedy tokens and a few others
    cand = torch.tensor([[S.reference_greedy(x[row_of(b, j, G)]) if (b + j) % 2 == 0 else (b + j) % V
                          for j in range(G)] for b in range(B)])
    out, intact = outputs(B, G)
    accept, alt = ops.spec_judge(tl, cand.to(dev), None, out=out)
    assert accept.data_ptr() == out[0].data_ptr() and intact()
    want = oracle(V, dtype, B, G, 0, cand, do_sample=False)
    assert alt.cpu().flatten().tolist() == [r["alt"] for r in want]
    assert accept.cpu().flatten().tolist() == [r["accept"] for r in want if r["accept"] is not None]
    near = total = 0
    for ci, cfg in enumerate(CONFIGS):
        cand = candidates(V, dtype, B, G, ci)
        runs = []
        for _ in range(2):
            out, intact = outputs(B, G)
            accept, alt = ops.spec_judge(tl, cand.to(dev), dl, SEED, ROUND, True, out=out, **cfg)
            assert intact(), f"{cfg}: the judge wrote outside its outputs"
            runs.append((accept.cpu().clone(), alt.cpu().clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{cfg}: two runs differ"
        recs = oracle(V, dtype, B, G, ci, cand)
        n, t = check_sampled(recs, runs[0][0], runs[0][1], V, dtype, B, G, ci)
        near, total = near + n, total + t
        if V >= 7:
            rejected = sum(1 for r in recs if r["accept"] is False)
            assert 0 < rejected or G == 1, f"{cfg}: no candidate is rejected: choose other inputs"
    assert near <= 0.01 * total, f"{near} of {total} decisions and draws are within TOL of flipping"


def test_round_tensor_row_independence_and_bad_candidates():
    V, dtype, B, G = 1003, torch.bfloat16, 3, 4
    x, y, _ = logit_rows(V, dtype)
    tl, dl = device_inputs(V, dtype, B, G)
    cfg = CONFIGS[1]
    cand = candidates(V, dtype, B, G, 1)
    cand[0, 1], cand[1, 0], cand[2, 3] = -1, V, 2 ** 40
    a0, l0 = ops.spec_judge(tl, cand.to(dev), dl, SEED, ROUND, True, **cfg)
    assert not a0[0, 1] and not a0[1, 0] and not a0[2, 3]
    assert ((l0 >= 0) & (l0 < V)).all()
    g0, _ = ops.spec_judge(tl, cand.to(dev), None)
    assert not g0[0, 1] and not g0[1, 0] and not g0[2, 3]
    rnd = torch.tensor([ROUND], dtype=torch.int32, device=dev)
    a1, l1 = ops.spec_judge(tl, cand.to(dev), dl, SEED, rnd, True, **cfg)
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    a2, l2 = ops.spec_judge(tl, cand.to(dev), dl, SEED, ROUND + 1, True, **cfg)
    assert not torch.equal(l0, l2)
    # row 1 keeps its logits and candidates, rows 0 and 2 change theirs (same layout: same summation order)
    tc, dc, c2 = tl.float().cpu(), dl.float().cpu(), cand.clone()
    tc[0], tc[2] = tc[2].clone(), tc[0].flip(-1)
    dc[0], dc[2] = dc[2].flip(-1), dc[0].clone()
    c2[0], c2[2] = cand[2].clamp(0, V - 1), cand[0].clamp(0, V - 1)
    t2, d2 = padded(tc, B, G + 1, dtype), padded(dc, B, G, dtype)
    assert t2.stride() == tl.stride() and t2.data_ptr() % 16 == tl.data_ptr() % 16
    a3, l3 = ops.spec_judge(t2, c2.to(dev), d2, SEED, ROUND, True, **cfg)
    assert torch.equal(a3[1], a0[1]) and torch.equal(l3[1], l0[1])
    assert not torch.equal(l3[0], l0[0]) or not torch.equal(l3[2], l0[2])


@pytest.mark.parametrize("dtype", TS.DTYPES)
def test_degenerate_rows_follow_the_greedy_rule(dtype):
    V, G = 1003, 3
    ninf, nan, inf = float("-inf"), float("nan"), float("inf")
    rows = torch.randn(4, G + 1, V, generator=torch.Generator().manual_seed(9)) * 3
    rows[0].fill_(ninf)
    rows[1].fill_(nan)
    rows[2, :, 11] = inf
    rows[3, :, ::2] = nan
    rows[3, :, 777] = 5.0e3
    draft = torch.randn(4, G, V, generator=torch.Generator().manual_seed(10)) * 3
    draft[3, 0].fill_(nan)      # a draft with nothing to draw from: q is one-hot at token 0
    draft[3, 1].fill_(ninf)
    tl, dl = padded(rows, 4, G + 1, dtype), padded(draft, 4, G, dtype)
    cand = torch.tensor([[0, 1, 5], [0, 0, 7], [11, 3, 11], [777, 0, 778]], device=dev)
    for kw in (dict(temperature=1.0), dict(top_k=4, top_p=0.5, temperature=1e-9), dict(top_p=0.0),
               dict(temperature=1e9)):
        accept, alt = ops.spec_judge(tl, cand, dl, 3, 1, True, **kw)
        assert ((alt >= 0) & (alt < V)).all(), (kw, alt.tolist())
        assert alt[:3].tolist() == [[0] * (G + 1), [0] * (G + 1), [11] * (G + 1)], (kw, alt.tolist())
        assert accept[:3].tolist() == [[True, False, False], [True, True, False], [True, False, True]], kw
        assert (alt[3] % 2 == 1).all(), (kw, alt.tolist())  # the NaN columns are never drawn
        if kw.get("temperature", 1.0) <= 1.0:  # all the mass is on 777: accepted whatever the draft says, 778 has none
            assert alt[3].tolist() == [777] * (G + 1) and accept[3].tolist() == [True, False, False], kw
    accept, alt = ops.spec_judge(tl, cand, None)
    assert alt.tolist() == [[0] * (G + 1), [0] * (G + 1), [11] * (G + 1), [777] * (G + 1)]
    assert accept.tolist() == [[True, False, False], [True, True, False], [True, False, True], [True, False, False]]


def test_entry_points_refuse_what_they_do_not_cover():
    from paddle_amd.ops import _native as N

    t = torch.zeros(2, 3, 16, device=dev)
    d = torch.zeros(2, 2, 16, device=dev)
    cand = torch.zeros(2, 2, dtype=torch.long, device=dev)
    acc = torch.zeros(2, 2, dtype=torch.bool, device=dev)
    alt = torch.zeros(2, 3, dtype=torch.long, device=dev)

    def judge(**kw):
        a = dict(dtype=0, tl=N.ptr(t), dl=N.ptr(d), cand=N.ptr(cand), B=2, G=2, V=16, do_sample=1, acc=N.ptr(acc),
                 alt=N.ptr(alt))
        a.update(kw)
        return N.lib().pa_spec_judge(a["dtype"], a["tl"], 48, 16, a["dl"], 32, 16, a["cand"], a["B"], a["G"], a["V"], 1,
                                     None, 0, a["do_sample"], 1.0, 0, 1.0, a["acc"], a["alt"], N.stream())

    assert judge() == 0
    for kw in (dict(dtype=2), dict(G=0), dict(G=17), dict(V=0), dict(V=131073), dict(B=0), dict(tl=None),
               dict(dl=None), dict(cand=None), dict(acc=None), dict(alt=None)):
        assert judge(**kw) != 0, kw
    assert judge(dl=None, do_sample=0) == 0
    torch.cuda.synchronize()
    assert not SP.spec_kernel_ok(t.double()) and not SP.spec_kernel_ok(t.cpu()) and not SP.spec_kernel_ok(t, None, True)
    with pytest.raises(ValueError):
        ops.spec_judge(t, cand, None, do_sample=True)
    with pytest.raises(ValueError):
        ops.spec_judge(torch.zeros(2, 18, 16, device=dev), torch.zeros(2, 17, dtype=torch.long, device=dev))


# ---------------------------------------------------------------------- commit
def test_commit_equals_the_cpu():
    cpu, *args = TC.commit_case("cpu")
    ops.spec_commit(*args, cpu)
    st, accept, alt, cand = TC.commit_case(dev)
    B = st.batch
    buf = torch.full((B * TC.MAX_NEW + 64,), SENTINEL, dtype=torch.long, device=dev)
    st.out = buf[:B * TC.MAX_NEW].view(B, TC.MAX_NEW).fill_(TC.PAD)
    assert ops.spec_commit(accept, alt, cand, st) is st.kept
    TC.check_commit(st)
    for name in ("tok", "out", "lengths", "done", "pos", "kept", "accepted"):
        assert torch.equal(getattr(st, name).cpu(), getattr(cpu, name)), name
    assert (buf[B * TC.MAX_NEW:] == SENTINEL).all()


def test_verify_with_a_device_round_equals_a_host_round():
    V, dtype, B, G = 1003, torch.bfloat16, 3, 4
    tl, dl = device_inputs(V, dtype, B, G)
    cand = candidates(V, dtype, B, G, 1).to(dev)
    states = []
    for rnd in (ROUND, torch.tensor([ROUND], dtype=torch.int32, device=dev)):
        st = ops.SpecState(B, 8, G, dev, eos_token_id=None)
        ops.sample_step(tl[:, 0], st, SEED, True, **CONFIGS[1])
        assert st.pos.tolist() == [1] * B
        accept, alt = ops.spec_verify(tl, cand, dl, st, SEED, rnd, True, **CONFIGS[1])
        first = [next((j for j in range(G) if not accept[b, j]), G) for b in range(B)]
        assert st.kept.tolist() == [a + 1 for a in first] and st.pos.tolist() == [a + 2 for a in first]
        assert st.tok.tolist() == [int(alt[b, a]) for b, a in enumerate(first)]
        states.append(st)
    for name in ("tok", "out", "lengths", "done", "pos", "kept", "accepted"):
        assert torch.equal(getattr(states[0], name), getattr(states[1], name)), name


# ---------------------------------------------------------------------- rewind_each
def test_rewind_each_on_the_device():
    for where in ("cpu", dev):
        c = ops.KVCache(1, 3, 16, 1, 64, torch.bfloat16, where)
        c.set_lens([5, 3, 4])
        c.rewind_each([1, 0, 0])
        c.rewind_each([1, 0, 2], bound=3)
        assert c.lens.cpu().tolist() == [3, 3, 2] and c.bound == 3
        p = ops.PagedKVCache(1, 3, 64, 1, 64, torch.bfloat16, where, block_size=16, num_blocks=8)
        p.reserve([20, 3, 33])
        p.set_lens([20, 3, 33])
        table = p.block_table.clone()
        p.rewind_each([5, 0, 2])
        p.rewind_each([3], rows=[2])
        with pytest.raises(ValueError):
            p.rewind_each([0, 4, 0])
        assert p.lens.cpu().tolist() == p.host_lens == [15, 3, 28] and torch.equal(p.block_table, table)


# ---------------------------------------------------------------------- models
NEW = TC.NEW
PROMPT_LENS = TC.PROMPT_LENS
_gpu_models = {}


def perturbed(model, sigma, seed=5):
    """A copy of the device model with seeded N(0, sigma^2) noise on every parameter."""
    d = copy.deepcopy(model)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in d.parameters():
            p.add_((torch.randn(p.shape, generator=g) * sigma).to(p.device, p.dtype))
    return d


def gpu_setup(kind):
    """(bf16 GPU model, its fp32 CPU copy, prompt, plain tokens, e, CPU teacher-forced logits)."""
    if kind not in _gpu_models:
        m = make_model(kind, dev, "bfloat16")
        cpu = make_model(kind)
        cpu.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
        g = torch.Generator().manual_seed(1)
        ids = torch.zeros(len(PROMPT_LENS), max(PROMPT_LENS), dtype=torch.long)
        for b, n in enumerate(PROMPT_LENS):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        ids = ids.to(dev)
        plain, _ = m.generate(ids, NEW, prompt_lens=PROMPT_LENS)
        # e: extend(all_logits) on the GPU against the fp32 copy, over prompt + plain tokens
        cache = m.init_cache(len(PROMPT_LENS), max(PROMPT_LENS) + NEW)
        m.prefill(ids, cache, PROMPT_LENS)
        got = m.extend(plain[:, :NEW - 1], cache, all_logits=True).float().cpu()  # predict tokens 1 .. NEW-1
        teacher = []
        with torch.no_grad():
            for b, n in enumerate(PROMPT_LENS):
                seq = torch.cat([ids[b, :n], plain[b, :NEW - 1]]).cpu()[None]
                teacher.append(cpu(seq)[0, n - 1:].float())  # [NEW, V]: the logits that predict token 0 .. NEW-1
        teacher = torch.stack(teacher)
        e = float((got - teacher[:, 1:]).abs().max())
        _gpu_models[kind] = (m, cpu, ids, plain.cpu(), e, teacher)
    return _gpu_models[kind]


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
@pytest.mark.parametrize("kind", ["llama", "gpt"])
def test_models_greedy_bf16(kind, cache):
    m, _, ids, plain, e, teacher = gpu_setup(kind)
    noisy = perturbed(m, TC.SIGMA[kind])
    kw = dict(prompt_lens=PROMPT_LENS, cache=cache, num_draft=4)
    a, a_len = m.generate(ids, NEW, draft=noisy, **kw)
    s = m.last_speculation
    assert s.emitted == int(a_len.sum()) == NEW * len(PROMPT_LENS) and s.accepted == int(s.state.accepted.sum())
    assert 0 <= s.accepted <= s.proposed <= s.rounds * 4 * len(PROMPT_LENS) and s.rounds >= 5
    b, _ = m.generate(ids, NEW, draft=noisy, **kw)
    assert torch.equal(a, b)
    a = a.cpu()
    compared = 0
    for r in range(len(PROMPT_LENS)):
        diff = (a[r] != plain[r]).nonzero()
        k = int(diff[0, 0]) if diff.numel() else NEW
        compared += k
        if k < NEW:
            gap = abs(float(teacher[r, k, plain[r, k]] - teacher[r, k, a[r, k]]))
            assert gap <= 4 * e, f"row {r} parts from the plain tokens at {k}: the two logits differ by {gap}, e = {e}"
    frac = compared / (NEW * len(PROMPT_LENS))
    print(f"{kind} {cache}: e = {e:.4f}, compared {frac:.2f} of the tokens, accepted {s.accepted} of {s.proposed}")
    assert frac >= 0.5, "choose another seed: the runs part too early to compare"
    exact, _ = m.generate(ids, NEW, draft=copy.deepcopy(m), **kw)
    s = m.last_speculation
    print(f"{kind} {cache}: a copy of the target as draft: accepted {s.accepted} of {s.proposed} in {s.rounds} rounds")
    assert ((exact >= 0) & (exact < m.cfg.vocab_size)).all()


def test_models_sampled_bf16():
    m, _, ids, _, _, _ = gpu_setup("llama")
    noisy = perturbed(m, TC.SIGMA["llama"])
    kw = dict(prompt_lens=PROMPT_LENS, do_sample=True, temperature=0.9, top_k=50, top_p=0.95, draft=noisy, num_draft=4)
    a, a_len = m.generate(ids, NEW, seed=123, cache="paged", **kw)
    s = m.last_speculation
    assert s.emitted == int(a_len.sum()) and s.accepted == int(s.state.accepted.sum()) <= s.proposed
    b, _ = m.generate(ids, NEW, seed=123, cache="paged", **kw)
    c, _ = m.generate(ids, NEW, seed=124, cache="paged", **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.min().item() >= 0 and a.max().item() < m.cfg.vocab_size
