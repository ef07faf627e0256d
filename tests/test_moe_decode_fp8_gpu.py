"""``ops.moe_decode_ffn`` over ``Fp8ExpertWeights`` on the gfx950 e4m3 kernels against the float64
oracle of moe_decode_oracle.py on the dequantised stacks (its bound as it is: the kernel's
arithmetic on exact products is the bf16 kernel's), and a quantised bf16 ERNIE-MoE on the GPU."""
import pytest
import torch

import moe_decode_oracle as O
import test_kv_fp8_gpu as KG
import test_moe_decode_cpu as MC
import test_moe_decode_gpu as TG
from paddle_amd import ops
from paddle_amd.utils import flags

pytestmark = pytest.mark.gpu
dev = "cuda"
# (H, I, E, k) -> seed.  The second shape: partial 256-column tiles (2I = 288, H = 272), K no
# multiple of the 128-row step; its router margin needs seed 1 (0.83 with seed 0).
SHAPES = {(256, 128, 8, 2): 0, (272, 144, 64, 6): 1}
# K = 1040 in one slice: more than the 1024 K values of A a workgroup stages at a time (router
# gap/need 3.97 with seed 1, 1.34 with seed 0)
LONG_K = (1040, 1040, 4, 2)
SEEDS = {**SHAPES, LONG_K: 1}
ROWS = [1, 2, 3, 5, 8, 16]
same_bits = TG.same_bits
_cases = {}


def case(shape):
    """16 rows on the device, the quantised stacks, and the oracle on their dequantised images."""
    if shape not in _cases:
        H, I, E, k = shape
        x, gate_w, gate_up, down = O.make_inputs(16, H, I, E, SEEDS[shape])
        g = torch.Generator().manual_seed(17)
        # a seeded power of two per (expert, column): no two scales of a tile need be equal
        gu8 = ops.quantize_experts_fp8(gate_up.float() * 2.0 ** torch.randint(-6, 7, (E, 1, 2 * I), generator=g))
        dn8 = ops.quantize_experts_fp8(down.float() * 2.0 ** torch.randint(-6, 7, (E, 1, H), generator=g))
        idx, w, gap, need = O.route_oracle(x, gate_w, k)
        assert (gap > need).all(), f"router margin: smallest gap/need {(gap / need).min():.2f}"
        ref, bound = O.ffn_oracle(x, gu8.dequant(), dn8.dequant(), idx, w)
        _cases[shape] = dict(x=x.to(dev), gate_w=gate_w.to(dev), gu=gu8.to(dev), dn=dn8.to(dev), idx=idx, ref=ref,
                             bound=bound, k=k)
    return _cases[shape]


def ffn(c, x, **kw):
    return ops.moe_decode_ffn(x, c["gate_w"], c["gu"], c["dn"], c["k"], **kw)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M", ROWS)
def test_within_the_oracle_bound(shape, M):
    c = case(shape)
    x = c["x"][:M]
    assert ops.moe_decode_ok(x, c["gate_w"], c["gu"], c["dn"], c["k"])
    with KG.knobs() as calls:
        y = ffn(c, x.view(M, 1, -1))
    assert calls == ["pa_moe_decode_route", "pa_moe_decode_ffn_f8"]
    assert y.shape == (M, 1, shape[0]) and y.dtype == torch.bfloat16
    O.check_bound(y.view(M, -1), c["ref"][:M], c["bound"][:M], f"fp8 moe_decode_ffn {shape} M={M}")


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_equal_the_one_row_call_and_runs_repeat(shape):
    c = case(shape)
    H = shape[0]
    y = ffn(c, c["x"])
    assert same_bits(y, ffn(c, c["x"]))
    for t in range(16):
        assert same_bits(ffn(c, c["x"][t:t + 1])[0], y[t]), t
    # 16 identical rows: every selected expert gets all 16 (the 16-row instantiation)
    y16 = ffn(c, c["x"][3:4].expand(16, H).contiguous())
    assert all(same_bits(y16[t], y[3]) for t in range(16))
    O.check_bound(y16, c["ref"][3:4].expand(16, H), c["bound"][3:4].expand(16, H), f"identical rows {shape}")
    # 9 rows on one expert set and 7 on another
    y97 = ffn(c, torch.cat([c["x"][3:4].expand(9, H), c["x"][4:5].expand(7, H)]).contiguous())
    assert all(same_bits(y97[t], y[3]) for t in range(9)) and all(same_bits(y97[t], y[4]) for t in range(9, 16))


@pytest.mark.parametrize("splits", [1, 3, (5, 5)])
def test_forced_split_counts(splits):
    """(5, 5) at H 256, I 128: down slices of 32 K rows, so the fifth lies past the end of K."""
    c = case((256, 128, 8, 2))
    for M in (3, 16):
        y = ffn(c, c["x"][:M], num_splits=splits)
        O.check_bound(y, c["ref"][:M], c["bound"][:M], f"fp8 num_splits {splits} M={M}")
    assert same_bits(ffn(c, c["x"][7:8], num_splits=splits)[0], y[7])


def test_a_slice_longer_than_a_chunk_of_a():
    """One slice of 1040 K rows: A is staged twice on the way (3 rows: 1 to 4 accumulator rows;
    16 rows on 4 experts: 8 or 16), and the second pass of a 16-row slot cannot reuse the first's A."""
    c = case(LONG_K)
    H = LONG_K[0]
    y = ffn(c, c["x"], num_splits=1)
    O.check_bound(y, c["ref"], c["bound"], "one slice of 1040 K rows, M=16")
    y3 = ffn(c, c["x"][:3], num_splits=1)
    y16 = ffn(c, c["x"][2:3].expand(16, H).contiguous(), num_splits=1)
    assert same_bits(y3, y[:3]) and all(same_bits(y16[t], y[2]) for t in range(16))


@pytest.mark.parametrize("shape", SHAPES)
def test_only_the_selected_experts_are_touched(shape):
    c = case(shape)
    M = 5 if shape[2] > 8 else 2  # leave some experts unselected
    want = ffn(c, c["x"][:M])
    unused = torch.ones(shape[2], dtype=torch.bool)
    unused[c["idx"][:M].reshape(-1)] = False
    assert unused.any()
    poisoned = []
    for w8 in (c["gu"], c["dn"]):
        q, s = w8.q.clone(), w8.scale.clone()
        q.view(torch.uint8)[unused.to(dev)] = 0x7F  # the e4m3 NaN code
        s[unused.to(dev)] = float("inf")
        poisoned.append(ops.Fp8ExpertWeights(q, s))
    assert same_bits(ops.moe_decode_ffn(c["x"][:M], c["gate_w"], *poisoned, c["k"]), want)


def test_what_takes_the_definition():
    shape = (256, 128, 8, 2)
    c = case(shape)
    x, gw, k = c["x"][:4], c["gate_w"], c["k"]
    # H = 264: not a multiple of 16 (gap/need of its router is 91 with seed 0)
    x264, gw264, gu264, dn264 = O.make_inputs(4, 264, 128, 8, 0)
    g8, d8 = ops.quantize_experts_fp8(gu264), ops.quantize_experts_fp8(dn264)
    idx, w, gap, need = O.route_oracle(x264, gw264, k)
    assert (gap > need).all()
    ref264, bound264 = O.ffn_oracle(x264, g8.dequant(), d8.dequant(), idx, w)
    with KG.knobs() as calls:
        assert not ops.moe_decode_ok(x264.to(dev), gw264.to(dev), g8.to(dev), d8.to(dev), k)
        y264 = ops.moe_decode_ffn(x264.to(dev), gw264.to(dev), g8, d8, k)
        assert not ops.moe_decode_ok(x.float(), gw, c["gu"], c["dn"], k)
        y32 = ffn(c, x.float())
        flags.set("moe_decode_fp8", False)
        try:
            assert not ops.moe_decode_ok(x, gw, c["gu"], c["dn"], k)
            yr = ffn(c, x)
            assert ops.moe_decode_ok(x, gw, c["gu"].dequant(), c["dn"].dequant(), k)  # the bf16 kernels stay on
        finally:
            flags.set("moe_decode_fp8", True)
    assert not [n for n in calls if n.startswith("pa_moe_decode")], calls
    O.check_bound(yr, c["ref"][:4], c["bound"][:4], "FLAGS_moe_decode_fp8=0")
    O.check_bound(y32, c["ref"][:4], c["bound"][:4], "fp32 rows")
    O.check_bound(y264, ref264, bound264, "H = 264")


def test_quantised_model_on_the_device():
    # seed 30: the smallest relative router gap over the prompts and 5 greedy tokens is 0.0167 on
    # the fp32 copy (searched on the CPU; asserted below against the 2^-6 of test_moe_decode_gpu.py)
    kind, seed = "grouped", 30
    cpu = MC.make_ernie(kind, seed=seed)  # fp32, holding the values the quantised model dequantises to
    with torch.no_grad():
        targets = {id(getattr(mod, n)) for mod, n in cpu._quant_targets()}
        for n, p in cpu.named_parameters():
            if id(p) in targets:
                p.copy_((ops.quantize_experts_fp8 if p.dim() == 3 else ops.quantize_weight_fp8)(p).dequant(torch.float32))
            elif "gate.weight" not in n:
                p.copy_(p.bfloat16().float())
    twin, m = MC.make_ernie(kind, dev, "bfloat16"), MC.make_ernie(kind, dev, "bfloat16")
    twin.load_state_dict(cpu.state_dict())
    m.load_state_dict(cpu.state_dict())
    m.quantize_weights()
    ids = torch.zeros(len(TG.PROMPT_LENS), max(TG.PROMPT_LENS), dtype=torch.long)
    g = torch.Generator().manual_seed(3)
    for b, n in enumerate(TG.PROMPT_LENS):
        ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
    ids = ids.to(dev)
    plain, lens = m.generate(ids, 5, prompt_lens=TG.PROMPT_LENS)
    graph, glens = m.generate(ids, 5, prompt_lens=TG.PROMPT_LENS, graph=True)
    assert torch.equal(graph, plain) and torch.equal(glens, lens)
    caches = [mod.init_cache(len(TG.PROMPT_LENS), max(TG.PROMPT_LENS) + 2) for mod in (m, twin)]
    tok = m.prefill(ids, caches[0], TG.PROMPT_LENS).argmax(-1)
    assert torch.equal(tok, plain[:, 0])
    twin.prefill(ids, caches[1], TG.PROMPT_LENS)
    seqs = [torch.cat([ids[b, :n], tok[b:b + 1]]).cpu() for b, n in enumerate(TG.PROMPT_LENS)]
    margin = TG.router_margin(cpu, [torch.cat([ids[b, :n], plain[b]]).cpu() for b, n in enumerate(TG.PROMPT_LENS)])
    print(f"smallest relative router gap {margin:.4f} (2^-6 = {2 ** -6:.4f})")
    assert margin > 2.0 ** -6, "choose another seed: a router decision of the tested tokens is too close"
    with KG.knobs() as calls:
        got = m.decode_step(tok, caches[0]).float().cpu()
    # the e4m3 expert kernels once per MoE layer, and no dequantised image of anything
    assert calls.count("pa_moe_decode_ffn_f8") == 2 and "pa_moe_decode_ffn" not in calls, calls
    assert not [n for n in calls if "dequant" in n], calls
    got_twin = twin.decode_step(tok, caches[1]).float().cpu()
    with torch.no_grad():
        want = torch.stack([cpu(s[None])[0, -1] for s in seqs])
    e0, e1 = float((got_twin - want).abs().max()), float((got - want).abs().max())
    print(f"e0 {e0:.3e} (bf16 twin) e1 {e1:.3e} (quantised) e1/e0 {e1 / e0:.2f}")
    assert e1 <= 2 * e0, (e0, e1)
