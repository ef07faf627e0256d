"""``ops.quantize_experts_fp8`` / ``Fp8ExpertWeights``, ``ops.moe_decode_ffn`` on a quantised pair
and ``ErnieMoEForCausalLM.quantize_weights()`` on the plain-torch (CPU) paths: everything is the
bf16 / fp32 computation on the dequantised weights, bit for bit."""
import pytest
import torch

import test_moe_decode_cpu as MC
from paddle_amd import ops


def stacks(seed=0, E=4, H=32, I=16):
    g = torch.Generator().manual_seed(seed)
    # a seeded power of two per (expert, column): the scales differ across experts and columns
    gu = 0.05 * torch.randn(E, H, 2 * I, generator=g) * 2.0 ** torch.randint(-6, 7, (E, 1, 2 * I), generator=g)
    dn = 0.05 * torch.randn(E, I, H, generator=g) * 2.0 ** torch.randint(-6, 7, (E, 1, H), generator=g)
    return gu, dn, g


def test_quantize_experts_is_quantize_weight_per_expert():
    w = stacks()[0]
    w[2, :, 5] = 0.0  # a zero column
    w8 = ops.quantize_experts_fp8(w)
    assert w8.q.dtype == torch.float8_e4m3fn and w8.q.shape == w.shape and w8.q.is_contiguous()
    assert w8.scale.dtype == torch.float32 and w8.scale.shape == (4, 32) and w8.scale[2, 5] == 1.0
    assert w8.nbytes == w.numel() + 4 * 4 * 32 and not w8.state_dict()
    for e in range(4):
        one = ops.quantize_weight_fp8(w[e])
        assert torch.equal(w8.q[e].view(torch.uint8), one.q.view(torch.uint8)) and torch.equal(w8.scale[e], one.scale)
    exact = w8.q.float() * w8.scale[:, None, :]
    assert w8.dequant().dtype == torch.bfloat16 and torch.equal(w8.dequant().float(), exact)
    sel = torch.tensor([3, 0, 3])
    assert torch.equal(w8.dequant(torch.float32, experts=sel), exact[sel])
    w[1, 3, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_experts_fp8(w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ffn_on_a_quantised_pair_is_the_ffn_on_the_dequantised_stacks(dtype):
    gu, dn, g = stacks()
    x = torch.randn(5, 32, generator=g).to(dtype)
    gate_w = 0.5 * torch.randn(32, 4, generator=g)
    gu8, dn8 = ops.quantize_experts_fp8(gu), ops.quantize_experts_fp8(dn)
    y = ops.moe_decode_ffn(x, gate_w, gu8, dn8, 2)
    assert y.dtype == dtype and torch.equal(y, ops.moe_decode_ffn(x, gate_w, gu8.dequant(), dn8.dequant(), 2))
    assert not ops.moe_decode_ok(x, gate_w, gu8, dn8, 2)  # CPU tensors
    for pair in ((gu8, dn), (gu, dn8)):
        with pytest.raises(ValueError, match="both"):
            ops.moe_decode_ffn(x, gate_w, *pair, 2)


def quantised_and_twin(kind):
    """(quantised model, a model from the same seed whose parameters hold the dequantised values)."""
    m, twin = MC.make_ernie(kind), MC.make_ernie(kind)
    with torch.no_grad():
        for mod, n in twin._quant_targets():
            p = getattr(mod, n)
            quant = ops.quantize_experts_fp8 if p.dim() == 3 else ops.quantize_weight_fp8
            p.copy_(quant(p).dequant(torch.float32))
    before = sum(p.numel() for p in m.parameters())
    assert m.quantize_weights() is m
    assert isinstance(m.layers[1].moe.stacked_experts()[0], ops.Fp8ExpertWeights)
    assert isinstance(m.layers[0].mlp.down, ops.Fp8Weight) and isinstance(m.layers[2].qkv_proj, ops.Fp8Weight)
    assert sum(p.numel() for p in m.parameters()) < before / 3  # the bf16 parameters are gone
    return m, twin


@pytest.mark.parametrize("kind", ["grouped", "grouped-shared"])
def test_quantised_model_equals_its_dequantised_twin(kind):
    m, twin = quantised_and_twin(kind)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, m.cfg.vocab_size, (3, 6), generator=g)
    with torch.no_grad():
        assert torch.equal(m(ids), twin(ids))
    ca, cb = m.init_cache(3, 16), twin.init_cache(3, 16)
    first = m.prefill(ids, ca)
    assert torch.equal(first, twin.prefill(ids, cb))
    tok = first.argmax(-1)
    assert torch.equal(m.decode_step(tok, ca), twin.decode_step(tok, cb))
    want, _ = twin.generate(ids, 8)
    for how in (dict(), dict(cache="paged"), dict(prefill_chunk=4)):
        got, _ = m.generate(ids, 8, **how)
        assert torch.equal(got, want), how
    with pytest.raises(RuntimeError, match="already"):
        m.quantize_weights()
    with pytest.raises(NotImplementedError, match="state_dict"):
        m.state_dict()
    with pytest.raises(RuntimeError, match="inference only"):
        m(ids)  # gradients on


def test_quantize_weights_refusals_change_nothing():
    m = MC.make_ernie("grouped", use_fp8_experts=True)
    with pytest.raises(NotImplementedError, match="use_fp8_experts"):
        m.quantize_weights()
    assert isinstance(m.layers[0].qkv_proj, torch.nn.Parameter)
    m = MC.make_ernie("list")
    with pytest.raises(NotImplementedError, match="grouped_experts=True"):
        m.quantize_weights()
    assert isinstance(m.layers[0].qkv_proj, torch.nn.Parameter)
