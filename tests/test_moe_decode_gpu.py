"""``ops.moe_decode_route`` / ``ops.moe_decode_ffn`` on the gfx950 kernels against the float64
oracle of moe_decode_oracle.py, their invariance and edge contracts, and bf16 ERNIE-MoE
generation on the GPU."""
import pytest
import torch

import moe_decode_oracle as O
import test_kv_fp8_cpu as K
import test_moe_decode_cpu as MC
from paddle_amd import ops
from paddle_amd.ops import _native
from paddle_amd.ops import moe_decode as MD
from paddle_amd.utils import flags

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPES = [(256, 128, 8, 2), (264, 136, 64, 6)]  # (H, I, E, k)
ROWS = [1, 2, 3, 5, 8, 16]
_cases = {}


def case(shape, seed=0):
    """16 rows of inputs on the device with their oracle, computed once per shape and shared
    (row results do not depend on each other, so the first M rows are the M-row case)."""
    if (shape, seed) not in _cases:
        H, I, E, k = shape
        x, gate_w, gate_up, down = O.make_inputs(16, H, I, E, seed)
        idx, w, gap, need = O.route_oracle(x, gate_w, k)
        ref, bound = O.ffn_oracle(x, gate_up, down, idx, w)
        _cases[(shape, seed)] = dict(x=x.to(dev), gate_w=gate_w.to(dev), gate_up=gate_up.to(dev), down=down.to(dev),
                                     idx=idx, w=w, gap=gap, need=need, ref=ref, bound=bound, k=k)
    return _cases[(shape, seed)]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def check_route(gi, gw, idx, w, what):
    assert torch.equal(gi.cpu().long(), idx), what
    rel = ((gw.double().cpu() - w).abs() / w).max().item()
    print(f"{what}: worst relative weight error {rel * 2 ** 20:.3f} x 2^-20")
    assert rel <= 2.0 ** -20, what


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M", ROWS)
def test_within_the_oracle_bound(shape, M):
    c = case(shape)
    assert (c["gap"] > c["need"]).all(), f"router margin: smallest gap/need {(c['gap'] / c['need']).min():.2f}"
    x = c["x"][:M]
    assert ops.moe_decode_ok(x, c["gate_w"], c["gate_up"], c["down"], c["k"])
    gi, gw = ops.moe_decode_route(x, c["gate_w"], c["k"])
    assert gi.dtype == torch.int32 and gw.dtype == torch.float32 and gi.shape == gw.shape == (M, c["k"])
    check_route(gi, gw, c["idx"][:M], c["w"][:M], f"route {shape} M={M}")
    y = ops.moe_decode_ffn(x.view(M, 1, -1), c["gate_w"], c["gate_up"], c["down"], c["k"])
    assert y.shape == (M, 1, shape[0]) and y.dtype == torch.bfloat16
    O.check_bound(y.view(M, -1), c["ref"][:M], c["bound"][:M], f"moe_decode_ffn {shape} M={M}")


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_equal_the_one_row_call_and_runs_repeat(shape):
    c = case(shape)
    args = (c["gate_w"], c["gate_up"], c["down"], c["k"])
    gi, gw = ops.moe_decode_route(c["x"], c["gate_w"], c["k"])
    y = ops.moe_decode_ffn(c["x"], *args)
    y2 = ops.moe_decode_ffn(c["x"], *args)
    assert same_bits(y, y2)
    for M in (5, 8):  # other row counts, other accumulator-row instantiations
        assert same_bits(ops.moe_decode_ffn(c["x"][:M], *args), y[:M])
    for t in range(16):
        i1, w1 = ops.moe_decode_route(c["x"][t:t + 1], c["gate_w"], c["k"])
        assert torch.equal(i1[0], gi[t]) and same_bits(w1[0], gw[t]), t
        assert same_bits(ops.moe_decode_ffn(c["x"][t:t + 1], *args)[0], y[t]), t


@pytest.mark.parametrize("shape", SHAPES)
def test_one_expert_set_for_all_rows_and_disjoint_experts(shape):
    H, I, E, k = shape
    c = case(shape)
    args = (c["gate_w"], c["gate_up"], c["down"], k)
    # 16 identical rows: every selected expert gets all 16 (the 16-row instantiation)
    x = c["x"][3:4].expand(16, H).contiguous()
    y = ops.moe_decode_ffn(x, *args)
    one = ops.moe_decode_ffn(x[:1], *args)
    for t in range(16):
        assert same_bits(y[t], one[0]), t
    O.check_bound(y, c["ref"][3:4].expand(16, H), c["bound"][3:4].expand(16, H), f"identical rows {shape}")
    # 9 rows of one choice and 7 of another: a 16-row call where slots hold 9 and 7 rows
    x = torch.cat([c["x"][3:4].expand(9, H), c["x"][4:5].expand(7, H)]).contiguous()
    y = ops.moe_decode_ffn(x, *args)
    two = ops.moe_decode_ffn(c["x"][3:5], *args)
    assert all(same_bits(y[t], two[0]) for t in range(9)) and all(same_bits(y[t], two[1]) for t in range(9, 16))
    # pairwise disjoint experts: row t picks experts k t .. k t + k - 1 (as many rows as E allows)
    M = min(16, E // k)
    g = torch.Generator().manual_seed(11)
    xd = 0.05 * torch.randn(M, H, generator=g)
    gate_w = 0.05 * torch.randn(H, E, generator=g)
    for t in range(M):
        xd[t, t] = 4.0
        for j in range(k):
            gate_w[t, k * t + j] = 1.0 - 0.1 * j
    xd = xd.to(torch.bfloat16)
    idx, w, gap, need = O.route_oracle(xd, gate_w, k)
    assert (gap > need).all()
    assert idx.tolist() == [[k * t + j for j in range(k)] for t in range(M)]
    gi, gw = ops.moe_decode_route(xd.to(dev), gate_w.to(dev), k)
    check_route(gi, gw, idx, w, f"disjoint experts {shape}")
    ref, bound = O.ffn_oracle(xd, c["gate_up"], c["down"], idx, w)
    y = ops.moe_decode_ffn(xd.to(dev), gate_w.to(dev), c["gate_up"], c["down"], k)
    O.check_bound(y, ref, bound, f"disjoint experts {shape}")


@pytest.mark.parametrize("splits", [1, 2, 3, (5, 5), (2, 1)])
def test_forced_split_counts(splits):
    """(5, 5) at H 256, I 128: the gate|up slices are 56 K rows (the last one short), the down
    slices 32 rows, so its fifth slice lies past the end of K and stores zeros."""
    shape = SHAPES[0]
    c = case(shape)
    for M in (3, 16):
        y = ops.moe_decode_ffn(c["x"][:M], c["gate_w"], c["gate_up"], c["down"], c["k"], num_splits=splits)
        O.check_bound(y, c["ref"][:M], c["bound"][:M], f"num_splits {splits} M={M}")
    one = ops.moe_decode_ffn(c["x"][7:8], c["gate_w"], c["gate_up"], c["down"], c["k"], num_splits=splits)
    assert same_bits(one[0], y[7])


def test_default_splits_come_from_the_shape():
    for H, I in ((256, 128), (264, 136), (2560, 1536), (4096, 1024)):
        sg, sd = ops.moe_decode_default_splits(H, I)
        assert sg >= 1 and sd >= 1 and (sg == 1 or H // sg >= 256) and (sd == 1 or I // sd >= 256)
    assert ops.moe_decode_default_splits(2560, 1536) == (4, 4)


def test_exact_ties_pick_the_lower_index():
    H, I, E, k = SHAPES[1]
    c = case(SHAPES[1])
    gate_w = c["gate_w"].clone()
    gate_w[:, 40] = gate_w[:, 7]  # duplicated columns: equal logits, bit for bit
    gate_w[:, 63] = gate_w[:, 0]
    gate_w[:, 21] = gate_w[:, 20]
    gi, gw = ops.moe_decode_route(c["x"], gate_w, k)
    seen = 0
    for row in gi.cpu().tolist():
        assert len(set(row)) == k and all(0 <= e < E for e in row)
        for lo, hi in ((7, 40), (0, 63), (20, 21)):
            if hi in row:
                assert lo in row and row.index(lo) + 1 == row.index(hi), row
                seen += 1
            elif lo in row:
                assert row.index(lo) == k - 1, row  # the tie was cut at k: the lower index stayed
                seen += 1
    assert seen >= 3, "the duplicated columns were never selected: duplicate other columns"
    # all logits equal: experts 0 .. k-1 with equal weights
    gi, gw = ops.moe_decode_route(torch.zeros(2, H, device=dev, dtype=torch.bfloat16), gate_w, k)
    assert gi.cpu().tolist() == [list(range(k))] * 2 and torch.allclose(gw.cpu(), torch.full((2, k), 1.0 / k), rtol=1e-6)
    # the full-softmax weights (no renormalisation), against float64
    idx, w, gap, need = O.route_oracle(c["x"], c["gate_w"], k, renorm=False)
    gi, gw = ops.moe_decode_route(c["x"], c["gate_w"], k, renorm=False)
    check_route(gi, gw, idx, w, "full-softmax weights")


def test_non_finite_inputs_give_distinct_indices_in_range():
    H, I, E, k = SHAPES[1]
    c = case(SHAPES[1])
    x = c["x"].clone()
    x[0, 5] = float("nan")
    x[1, 6] = float("inf")
    x[2, 7] = float("-inf")
    x[3, :2] = torch.tensor([float("inf"), float("-inf")])
    x[4] = float("nan")
    x[5] = float("inf")
    gi, _ = ops.moe_decode_route(x, c["gate_w"], k)
    for row in gi.cpu().tolist():
        assert len(set(row)) == k and all(0 <= e < E for e in row), row
    assert gi[0].cpu().tolist() == list(range(k))  # NaN logits count as -inf: all tie
    y = ops.moe_decode_ffn(x, c["gate_w"], c["gate_up"], c["down"], k)
    torch.cuda.synchronize()
    assert same_bits(y[6:], ops.moe_decode_ffn(c["x"], c["gate_w"], c["gate_up"], c["down"], k)[6:])


def test_sentinels_and_strided_views():
    H, I, E, k = SHAPES[1]
    c = case(SHAPES[1])
    M = 5
    want = ops.moe_decode_ffn(c["x"][:M], c["gate_w"], c["gate_up"], c["down"], k)
    # x: a strided view of a larger buffer whose other rows and columns hold NaN
    big = torch.full((M + 3, H + 8), float("nan"), device=dev, dtype=torch.bfloat16)
    big[:M, :H] = c["x"][:M]
    xv = big[:M, :H]
    assert xv.stride(0) == H + 8 and ops.moe_decode_ok(xv, c["gate_w"], c["gate_up"], c["down"], k)
    assert same_bits(ops.moe_decode_ffn(xv, c["gate_w"], c["gate_up"], c["down"], k), want)
    # y: a view inside a NaN-filled buffer; nothing around it is written
    buf = torch.full((M + 2, H + 16), float("nan"), device=dev, dtype=torch.bfloat16)
    out = buf[1:M + 1, 8:8 + H]
    gi, gw = MD._launch_route(xv, c["gate_w"], k, True)
    MD._launch_ffn(xv, c["gate_up"], c["down"], gi, gw, ops.moe_decode_default_splits(H, I), out=out)
    assert same_bits(out, want)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:M + 1, 8:8 + H] = False
    assert torch.isnan(buf[mask]).all()


def test_what_the_kernels_refuse():
    H, I, E, k = SHAPES[0]
    c = case(SHAPES[0])
    x, gw, gu, dn = c["x"][:4], c["gate_w"], c["gate_up"], c["down"]
    calls = []
    orig = _native.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    _native.call = spy
    try:
        y = ops.moe_decode_ffn(x, gw, gu, dn, k)
        assert calls == ["pa_moe_decode_route", "pa_moe_decode_ffn"]  # 1 + 3 launches
        del calls[:]
        assert not ops.moe_decode_ok(x.float(), gw, gu, dn, k)  # fp32 rows
        assert not ops.moe_decode_ok(x.cpu(), gw.cpu(), gu.cpu(), dn.cpu(), k)
        assert not ops.moe_decode_ok(x[:, 1:], gw[1:], gu[:, 1:], dn, k)  # H = 255
        assert not ops.moe_decode_ok(x[:, ::2], gw[::2], gu[:, ::2], dn, k)  # column stride 2
        assert not ops.moe_decode_ok(x, gw, gu[:, :, :-2], dn[:, :-1], k)  # I = 127, not contiguous
        flags.set("moe_decode", False)
        try:
            assert not ops.moe_decode_ok(x, gw, gu, dn, k)
            yr = ops.moe_decode_ffn(x, gw, gu, dn, k)  # the plain-torch definition on the device
        finally:
            flags.set("moe_decode", True)
        assert not calls
    finally:
        _native.call = orig
    O.check_bound(yr, c["ref"][:4], c["bound"][:4], "FLAGS_moe_decode=0")
    assert y.shape == yr.shape
    with pytest.raises(ValueError):
        ops.moe_decode_ffn(x, gw, gu, dn, E + 1)
    with pytest.raises(ValueError):
        ops.moe_decode_ffn(torch.cat([c["x"], x]), gw, gu, dn, k)  # 20 rows
    # routing alone has its own limits: any H, 2-byte aligned rows
    xr, gr = c["x"][:4, 2:254], gw[2:254].contiguous()
    with_spy = []
    _native.call = lambda name, *a: with_spy.append(name) or orig(name, *a)
    try:
        ri, rw = ops.moe_decode_route(xr, gr, k)
    finally:
        _native.call = orig
    assert with_spy == ["pa_moe_decode_route"]
    ci, cw = MD._route_ref(xr.cpu(), gr.cpu(), k, True)
    assert all(len(set(r)) == k and all(0 <= e < E for e in r) for r in ri.cpu().tolist())
    assert torch.allclose(rw.cpu().sum(-1), torch.ones(4), atol=1e-6)
    same = ri.cpu() == ci  # where the choice agrees with the reference (no margin is asserted here) so do the weights
    assert torch.allclose(rw.cpu()[same], cw[same], rtol=1e-4)
    L = _native.lib()
    bad = 1  # hipErrorInvalidValue
    idx, w = ops.moe_decode_route(x, gw, k)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=dev)
    out = torch.empty(4, H, dtype=torch.bfloat16, device=dev)
    P = _native.ptr

    def ffn(M=4, H_=H, I_=I, E_=E, k_=k, ldx=H, sg=1, sd=1, xp=x):
        return L.pa_moe_decode_ffn(P(xp), ldx, P(gu), P(dn), P(idx), P(w), P(ws), P(out), H_, M, H_, I_, E_, k_, sg, sd,
                                   _native.stream())

    assert ffn(M=17) == bad and ffn(M=0) == bad and ffn(H_=252) == bad and ffn(I_=124) == bad
    assert ffn(E_=257) == bad and ffn(k_=17) == bad and ffn(k_=0) == bad and ffn(E_=1) == bad  # k > E
    assert ffn(ldx=H - 8) == bad and ffn(sg=0) == bad and ffn(sd=65) == bad
    assert ffn(xp=x.view(-1)[4:]) == bad  # 8-byte aligned rows
    assert L.pa_moe_decode_route(P(x), H, P(gw), P(idx), P(w), 17, H, E, k, 1, _native.stream()) == bad
    assert L.pa_moe_decode_route(P(x), H, P(gw), P(idx), P(w), 4, H, 300, k, 1, _native.stream()) == bad
    assert L.pa_moe_decode_route(P(x), H, P(gw), P(idx), P(w), 4, H, E, E + 1, 1, _native.stream()) == bad
    L.pa_clear_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- models
# Seeds at which every router decision over the prompts and the GPU model's own greedy tokens has a
# relative gap (k-th minus (k+1)-th logit over the largest |logit| of the row) above 2^-6 on the
# fp32 copy, which the test asserts first.
SEEDS = {"list-shared": 163, "grouped": 76}
PROMPT_LENS = MC.PROMPT_LENS
NEW = 5
_gpu = {}


def setup(kind):
    """(bf16 GPU model, its fp32 CPU copy, prompts on the device, plain greedy tokens)."""
    if kind not in _gpu:
        cpu = MC.make_ernie(kind, seed=SEEDS[kind])
        with torch.no_grad():
            for n, p in cpu.named_parameters():
                if "gate.weight" not in n:  # the router stays fp32 in the bf16 model
                    p.copy_(p.bfloat16().float())
        m = MC.make_ernie(kind, dev, "bfloat16")
        m.load_state_dict(cpu.state_dict())
        g = torch.Generator().manual_seed(3)
        ids = torch.zeros(len(PROMPT_LENS), max(PROMPT_LENS), dtype=torch.long)
        for b, n in enumerate(PROMPT_LENS):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        ids = ids.to(dev)
        plain, lengths = m.generate(ids, NEW, prompt_lens=PROMPT_LENS)
        _gpu[kind] = (m, cpu, ids, plain, lengths)
    return _gpu[kind]


def router_margin(cpu, seqs):
    """Smallest relative router gap of the fp32 model over the token sequences."""
    worst = [float("inf")]

    def hook(mod, inp, out):
        x = inp[0].reshape(-1, inp[0].shape[-1]).double()
        logits = x @ mod.weight.double()
        sl = logits.sort(-1, descending=True).values
        rel = (sl[:, mod.top_k - 1] - sl[:, mod.top_k]) / logits.abs().max(-1).values
        worst[0] = min(worst[0], float(rel.min()))

    hooks = [layer.moe.gate.register_forward_hook(hook) for layer in cpu.layers if layer.is_moe]
    try:
        with torch.no_grad():
            for s in seqs:
                cpu(s[None])
    finally:
        for h in hooks:
            h.remove()
    return worst[0]


@pytest.mark.parametrize("kind", list(SEEDS))
def test_models_decode_step_and_generate_paths(kind):
    m, cpu, ids, plain, lengths = setup(kind)
    seqs = [torch.cat([ids[b, :n], plain[b]]).cpu() for b, n in enumerate(PROMPT_LENS)]
    margin = router_margin(cpu, seqs)
    print(f"{kind} seed {SEEDS[kind]}: smallest relative router gap {margin:.4f} (2^-6 = {2 ** -6:.4f})")
    assert margin > 2.0 ** -6, "choose another seed: a router decision of the tested tokens is too close"
    # decode_step against the fp32 copy: e1 <= 2 e0, e0 the error of model(ids) at the same position
    cache = m.init_cache(len(PROMPT_LENS), max(PROMPT_LENS) + NEW)
    m.prefill(ids, cache, PROMPT_LENS)
    import test_kv_fp8_gpu as KG

    with KG.knobs() as calls:
        got = m.decode_step(plain[:, 0], cache).float().cpu()
    n_moe = sum(layer.is_moe for layer in m.layers)
    # the step runs the expert-streaming kernels, once per MoE layer, not the fallback
    assert n_moe == 2 and calls.count("pa_moe_decode_route") == calls.count("pa_moe_decode_ffn") == n_moe, calls
    assert not [n for n in calls if n in ("pa_moe_route", "pa_moe_gather", "pa_moe_reduce")], calls
    e0 = e1 = 0.0
    with torch.no_grad():
        for b, n in enumerate(PROMPT_LENS):
            seq = seqs[b][:n + 1]
            want = cpu(seq[None])[0, -1]
            e0 = max(e0, float((m(seq[None].to(dev))[0, -1].float().cpu() - want).abs().max()))
            e1 = max(e1, float((got[b] - want).abs().max()))
    print(f"{kind}: e0 {e0:.3e} e1 {e1:.3e} e1/e0 {e1 / e0:.2f}")
    assert e1 <= 2 * e0, (e0, e1)
    # the launch loop, the replayed graph, the paged cache, chunked prefill and the plain-torch MoE
    kw = dict(prompt_lens=PROMPT_LENS)
    for how in (dict(graph=True), dict(cache="paged", block_size=16), dict(graph=True, cache="paged"),
                dict(sampler="philox"), dict(prefill_chunk=3)):
        toks, lens = m.generate(ids, NEW, **kw, **how)
        assert torch.equal(toks, plain) and torch.equal(lens, lengths), how
    flags.set("moe_decode", False)
    try:
        toks, _ = m.generate(ids, NEW, **kw)
    finally:
        flags.set("moe_decode", True)
    assert torch.equal(toks, plain), "FLAGS_moe_decode=0"


def test_models_more_than_sixteen_rows_per_decode_step():
    """17 rows are beyond the decode kernels: the MoE FFN of the step runs ``MoELayer.forward``
    (launch loop only: above 16 rows the step's GEMMs are ``ops.linear``'s, which a capture does
    not take)."""
    g = torch.Generator().manual_seed(9)
    for kind in ("grouped", "list-shared"):
        m = setup(kind)[0]
        ids = torch.randint(1, m.cfg.vocab_size, (17, 4), generator=g).to(dev)
        toks, lengths = m.generate(ids, 3)
        assert toks.shape == (17, 3) and lengths.tolist() == [3] * 17
        assert ((toks >= 0) & (toks < m.cfg.vocab_size)).all()
        again, _ = m.generate(ids, 3, sampler="philox", cache="paged")
        assert torch.equal(again, toks)


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
def test_models_fp8_kv_cache_equals_the_twin(cache):
    import test_kv_fp8_gpu as KG

    m, _, ids, _, _ = setup("grouped")
    kw = dict(cache=cache, block_size=16) if cache == "paged" else dict(cache=cache)
    with KG.knobs() as calls:
        toks, lengths = K.check_against_twin(m, ids, cache)
    f8 = [n for n in calls if n.endswith("_f8")]
    tail = "_paged_f8" if cache == "paged" else "_f8"
    assert set(f8) == {"pa_kv_append" + tail, "pa_attn_decode" + tail}, set(calls)
    g_toks, g_len = m.generate(ids, 12, prompt_lens=K.PROMPT_LENS, kv_dtype="fp8_e4m3", graph=True, **kw)
    p_toks, p_len = m.generate(ids, 12, prompt_lens=K.PROMPT_LENS, kv_dtype="fp8_e4m3", sampler="philox", **kw)
    assert torch.equal(g_toks, p_toks) and torch.equal(g_len, p_len)
    assert torch.equal(g_toks, toks) and torch.equal(g_len, lengths)


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
def test_models_speculative_greedy(cache):
    """What test_speculative_gpu.py::test_models_greedy_bf16 asserts for the dense models."""
    kind, NEW_S, sigma = "list-shared", 24, 1e-3
    m, cpu, ids, _, _ = setup(kind)
    plain, _ = m.generate(ids, NEW_S, prompt_lens=PROMPT_LENS)
    c = m.init_cache(len(PROMPT_LENS), max(PROMPT_LENS) + NEW_S)
    m.prefill(ids, c, PROMPT_LENS)
    got = m.extend(plain[:, :NEW_S - 1], c, all_logits=True).float().cpu()
    teacher = []
    with torch.no_grad():
        for b, n in enumerate(PROMPT_LENS):
            seq = torch.cat([ids[b, :n], plain[b, :NEW_S - 1]]).cpu()[None]
            teacher.append(cpu(seq)[0, n - 1:].float())
    teacher = torch.stack(teacher)
    e = float((got - teacher[:, 1:]).abs().max())
    plain = plain.cpu()
    noisy = MC.perturbed(m, kind, sigma)
    kw = dict(prompt_lens=PROMPT_LENS, cache=cache, num_draft=4)
    a, a_len = m.generate(ids, NEW_S, draft=noisy, **kw)
    s = m.last_speculation
    assert s.emitted == int(a_len.sum()) == NEW_S * len(PROMPT_LENS) and s.accepted == int(s.state.accepted.sum())
    assert 0 <= s.accepted <= s.proposed <= s.rounds * 4 * len(PROMPT_LENS) and s.rounds >= 5
    b_, _ = m.generate(ids, NEW_S, draft=noisy, **kw)
    assert torch.equal(a, b_)
    a = a.cpu()
    compared = 0
    for r in range(len(PROMPT_LENS)):
        diff = (a[r] != plain[r]).nonzero()
        k = int(diff[0, 0]) if diff.numel() else NEW_S
        compared += k
        if k < NEW_S:
            gap = abs(float(teacher[r, k, plain[r, k]] - teacher[r, k, a[r, k]]))
            assert gap <= 4 * e, f"row {r} parts from the plain tokens at {k}: the two logits differ by {gap}, e = {e}"
    frac = compared / (NEW_S * len(PROMPT_LENS))
    print(f"ernie {cache}: e = {e:.4f}, compared {frac:.2f} of the tokens, accepted {s.accepted} of {s.proposed}")
    assert frac >= 0.5, "choose another seed: the runs part too early to compare"
    exact, _ = m.generate(ids, NEW_S, draft=MC.perturbed(m, kind, 0.0), **kw)
    s = m.last_speculation
    print(f"ernie {cache}: a copy of the target as draft: accepted {s.accepted} of {s.proposed} in {s.rounds} rounds")
    assert ((exact >= 0) & (exact < m.cfg.vocab_size)).all()
