"""``ops.grouped_swiglu_mlp_fp8w`` on the gfx950 e4m3 ragged grouped kernels
(csrc/kernels/moe_rows_f8.hip) against the float64 oracle of moe_decode_oracle.py on the
dequantised stacks, and a quantised ERNIE-MoE above 16 rows."""
import pytest
import torch

import moe_decode_oracle as O
import test_grouped_fp8w_cpu as C
import test_kv_fp8_gpu as KG
import test_moe_decode_cpu as MC
import test_moe_decode_gpu as TG
from paddle_amd import ops
from paddle_amd.ops.grouped_fp8w import CHUNK_K, ROUTED_SORTED_ROWS, TM
from paddle_amd.utils import flags

pytestmark = pytest.mark.gpu
dev = "cuda"
KERNEL = "pa_moe_rows_f8"
# the second shape: partial column tiles (I = 144, H = 272), K no multiple of the 128-k step
SHAPES = [(256, 128, 8), (272, 144, 64)]
same_bits = TG.same_bits


def on_device(c):
    if "xd" not in c:  # fresh stacks: Module.to() would move the case's own
        c.update(xd=c["x"].to(dev), gud=ops.Fp8ExpertWeights(c["gu"].q.to(dev), c["gu"].scale.to(dev)),
                 dnd=ops.Fp8ExpertWeights(c["dn"].q.to(dev), c["dn"].scale.to(dev)))
    return c["xd"], c["gud"], c["dnd"]


def run(c, counts=None, x=None):
    xd, gu, dn = on_device(c)
    return ops.grouped_swiglu_mlp_fp8w(xd if x is None else x, gu, dn, c["counts"] if counts is None else counts)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pattern", C.PATTERNS)
@pytest.mark.parametrize("where", ["host", "device"])
def test_within_the_oracle_bound(shape, pattern, where):
    c = C.case(*shape, pattern)
    x, gu, dn = on_device(c)
    counts = c["counts"] if where == "host" else torch.tensor(c["counts"], device=dev)
    assert ops.grouped_fp8w_ok(x, gu, dn)
    with KG.knobs() as calls:
        y = run(c, counts)
    assert calls == [KERNEL], calls
    assert y.shape == x.shape and y.dtype == torch.bfloat16
    O.check_bound(y, c["ref"], c["bound"], f"grouped fp8w {shape} {pattern} counts on the {where}")


@pytest.mark.parametrize("shape", SHAPES)
def test_a_row_has_the_same_bits_wherever_it_stands(shape):
    H, I, E = shape
    c = C.case(*shape, "random_100")
    x, _, _ = on_device(c)
    y = run(c)
    assert same_bits(run(c), y)
    e = max(range(E), key=lambda i: c["counts"][i])  # an expert with rows in the 100-row case
    t = sum(c["counts"][:e + 1]) - 1                 # its last row
    one_hot = lambda n: [n if i == e else 0 for i in range(E)]
    alone = run(c, one_hot(1), x[t:t + 1])
    assert same_bits(alone[0], y[t])
    for pos in (0, TM - 1, TM):  # first row, last row of the first tile, alone in the second
        xs = x[:TM + 1].clone()
        xs[pos] = x[t]
        assert same_bits(run(c, one_hot(TM + 1), xs)[pos], alone[0]), pos


def test_k_longer_than_a_chunk_of_rows():
    """H = I = CHUNK_K + 16: both products stage their rows twice."""
    K = CHUNK_K + 16
    c = C.case(K, K, 4, (5, 0, TM + 1, 2))
    assert sum(c["counts"]) == 40
    O.check_bound(run(c), c["ref"], c["bound"], f"K = {K}, 40 rows on 4 experts")


def test_what_takes_the_definition():
    c = C.case(256, 128, 8, (2, 0, 1, 0, 3, 0, 0, 0))
    c264 = C.case(264, 128, 8, (2, 0, 1, 0, 3, 0, 0, 1))  # H no multiple of 16
    x, gu, dn = on_device(c)
    with KG.knobs() as calls:
        assert not ops.grouped_fp8w_ok(*on_device(c264))
        y264 = run(c264)
        assert not ops.grouped_fp8w_ok(x.float(), gu, dn)
        y32 = run(c, x=x.float())
        flags.set("moe_rows_fp8", False)
        try:
            assert not ops.grouped_fp8w_ok(x, gu, dn)
            yr = run(c)
        finally:
            flags.set("moe_rows_fp8", True)
        with pytest.raises(ValueError):
            ops.grouped_fp8w_kernel(*on_device(c264), c264["counts"])
    assert KERNEL not in calls, calls
    O.check_bound(y264, c264["ref"], c264["bound"], "H = 264")
    O.check_bound(y32, c["ref"], c["bound"], "fp32 rows")
    O.check_bound(yr, c["ref"], c["bound"], "FLAGS_moe_rows_fp8=0")
    assert same_bits(ops.grouped_fp8w_kernel(x, gu, dn, c["counts"]), run(c))  # the flag does not bind it


def test_quantised_model_above_16_rows():
    """decode_step at batch 20 (40 sorted rows) and a 40-token prefill (80) of the quantised tiny
    model: the kernels once per MoE layer and no dequantised expert image.  The attention and
    dense-MLP ``Fp8Weight``s still dequantise above 16 rows (``pa_fp8w_dequant``, not part of this
    kernel), so that one name is the only launch with "dequant" in it that may appear."""
    assert ROUTED_SORTED_ROWS is None or ROUTED_SORTED_ROWS >= 80
    cpu = MC.make_ernie("grouped", seed=30)  # fp32, holding the values the quantised model dequantises to
    with torch.no_grad():
        targets = {id(getattr(mod, n)) for mod, n in cpu._quant_targets()}
        for n, p in cpu.named_parameters():
            if id(p) in targets:
                p.copy_((ops.quantize_experts_fp8 if p.dim() == 3 else ops.quantize_weight_fp8)(p).dequant(torch.float32))
            elif "gate.weight" not in n:
                p.copy_(p.bfloat16().float())
    m = MC.make_ernie("grouped", dev, "bfloat16")
    m.load_state_dict(cpu.state_dict())
    m.quantize_weights()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, m.cfg.vocab_size, (20, 4), generator=g)
    long = torch.randint(1, m.cfg.vocab_size, (1, 40), generator=g)
    with torch.no_grad():
        want_d = torch.stack([cpu(s[None])[0, -1] for s in ids])
        want_p = cpu(long)[0, -1:]

    def both(on):
        flags.set("moe_rows_fp8", on)
        try:
            cache = m.init_cache(20, 8)
            m.prefill(ids[:, :3].to(dev), cache, [3] * 20)
            with KG.knobs() as cd:
                got_d = m.decode_step(ids[:, 3].to(dev), cache).float().cpu()
            with KG.knobs() as cp:
                got_p = m.prefill(long.to(dev), m.init_cache(1, 48), [40]).float().cpu()
        finally:
            flags.set("moe_rows_fp8", True)
        return cd, cp, float((got_d - want_d).abs().max()), float((got_p - want_p).abs().max())

    cd0, cp0, d0, p0 = both(False)
    cd1, cp1, d1, p1 = both(True)
    print(f"decode B 20: err {d1:.3e} (flag off {d0:.3e}); prefill 40: err {p1:.3e} (flag off {p0:.3e})")
    for calls, off in ((cd1, cd0), (cp1, cp0)):
        assert calls.count(KERNEL) == 2 and KERNEL not in off, calls
        assert not [n for n in calls if "dequant" in n and n != "pa_fp8w_dequant"], calls
        assert "pa_fp8w_dequant_experts" in off
    assert d1 <= 2 * d0 and p1 <= 2 * p0, (d0, d1, p0, p1)
