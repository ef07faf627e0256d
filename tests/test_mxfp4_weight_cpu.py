"""MXFP4 weight-only quantisation on the CPU (ops/skinny_mxfp4.py, quantize_weights("mxfp4")): the
quantiser's contract, the packed image, and quantised models against a twin that holds the
dequantised values -- bit for bit, because power-of-two group scales make ``code * scale`` exact
in bf16 and fp32."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.autograd import tape
from paddle_amd.models.ernie_moe import ERNIE_MOE_CONFIGS, ErnieMoEConfig, ErnieMoEForCausalLM
from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM
from test_generation_cpu import make_model

E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


def _scales(w4):
    return torch.ldexp(torch.ones(()), w4.scale_e8m0.int() - 127)


def test_every_code_decodes_to_the_e2m1_table():
    """Column n of a [32, 16] weight holds the 16 table values times 2^(n - 8), twice: amax is
    6 * 2^(n - 8), so the scale is 2^(n - 8) and row k gets code k % 16 (-0 becomes code 0)."""
    w = E2M1.repeat(2)[:, None] * torch.exp2(torch.arange(16.) - 8)
    w4 = ops.quantize_weight_mxfp4(w)
    want = (torch.arange(32) % 16).to(torch.uint8)
    want[want == 8] = 0
    assert torch.equal(w4.codes(), want[:, None].expand(32, 16))
    assert torch.equal(w4.scale_e8m0, (torch.arange(16) - 8 + 127).to(torch.uint8)[None])
    assert torch.equal(w4.dequant(torch.float32), w)


@pytest.mark.parametrize("amax,exp", [(6 * 2.0 ** -3, -3), (6 * 2.0 ** -3 * (1 + 2.0 ** -23), -2), (0.0, 0),
                                      (2.0 ** 120, 100), (2.0 ** -120, -100), (6.0, 0), (3.0, -1), (3.01, 0)])
def test_scale_rule(amax, exp):
    w = torch.zeros(64, 16)
    w[40, 3] = -amax  # the second group of column 3; every other group is all zero
    w4 = ops.quantize_weight_mxfp4(w)
    want = torch.full((2, 16), 127, dtype=torch.uint8)
    want[1, 3] = exp + 127
    assert torch.equal(w4.scale_e8m0, want)


@pytest.mark.parametrize("K,Nn", [(32, 16), (160, 48), (96, 40)])
def test_contract_and_packed_image(K, Nn):
    """(96, 40): N is padded in the image (to 48) with zero codes; K never is."""
    g = torch.Generator().manual_seed(K + Nn)
    w = (torch.randn(K, Nn, generator=g) * torch.exp2(torch.randint(-20, 20, (K // 32, 1, Nn), generator=g).float())
         .expand(-1, 32, -1).reshape(K, Nn)).bfloat16()
    w4 = ops.quantize_weight_mxfp4(w)
    assert w4.shape == w.shape and w4.packed.dtype == w4.scale_e8m0.dtype == torch.uint8
    assert w4.packed.numel() == K * 8 * -(-Nn // 16) and w4.nbytes == w4.packed.numel() + K // 32 * Nn
    assert not hasattr(w4, "q")  # the canonical code tensor is not kept
    codes = w4.codes()
    assert codes.shape == (K, Nn) and codes.dtype == torch.uint8 and codes.max() < 16
    # the documented order: strip, group, column, byte, low nibble first
    for k, n in [(0, 0), (K - 1, Nn - 1), (K // 2 + 1, Nn // 2)]:
        byte = w4.packed[((n // 16 * (K // 32) + k // 32) * 16 + n % 16) * 16 + k % 32 // 2]
        assert (byte >> 4 * (k % 2)) & 15 == codes[k, n]
    deq, scale = w4.dequant(), _scales(w4).repeat_interleave(32, 0)
    assert deq.dtype == torch.bfloat16 and deq.data_ptr() != w4.dequant().data_ptr()
    assert torch.equal(deq.float(), w4.dequant(torch.float32))
    assert torch.equal(deq.float(), E2M1[codes.long()] * scale), "code * scale is exact in bf16"
    err, bound = (deq.double() - w.double()).abs(), torch.maximum(w.double().abs(), scale.double()) / 4
    assert (err <= bound).all()


def test_out_of_scope_raises():
    with pytest.raises(ValueError, match="32"):
        ops.quantize_weight_mxfp4(torch.ones(48, 16))
    for bad in (float("nan"), float("inf")):
        w = torch.ones(32, 16)
        w[3, 5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ops.quantize_weight_mxfp4(w)
    quant = _pair("llama")[0]
    ids = torch.randint(1, 512, (1, 4))
    with pytest.raises(RuntimeError, match="already quantised"):
        quant.quantize_weights("mxfp4")
    with pytest.raises(ValueError, match="fmt.*mxfp4"):
        make_model("gpt").quantize_weights(fmt="int4")
    with pytest.raises(RuntimeError, match="inference only"):
        quant(ids)  # gradients enabled
    with torch.no_grad(), tape.recording(), pytest.raises(RuntimeError, match="inference only"):
        quant(ids)
    with pytest.raises(NotImplementedError, match="state_dict"):
        quant.state_dict()
    moe = ErnieMoEForCausalLM(ErnieMoEConfig(**ERNIE_MOE_CONFIGS["ernie-moe-tiny"], grouped_experts=True,
                                             dtype="float32"), device="cpu")
    with pytest.raises(NotImplementedError, match="mxfp4"):
        moe.quantize_weights(fmt="mxfp4")
    assert getattr(moe, "_pa_quantized", None) is None and isinstance(moe.layers[0].qkv_proj, torch.nn.Parameter)
    bad = make_model("llama")  # down_proj has K = 688, no multiple of 32
    with pytest.raises(ValueError, match="multiple of 32"):
        bad.quantize_weights("mxfp4")
    assert isinstance(bad.layers[0].qkv_proj, torch.nn.Parameter)  # nothing was converted


def tiny(kind, device="cpu", dtype="float32"):
    """test_generation_cpu's tiny models; the llama with an intermediate size of 704 instead of 688,
    which is no multiple of the group of 32."""
    if kind == "gpt":
        return make_model(kind, device, dtype)
    torch.manual_seed(0)
    cfg = LlamaConfig(**dict(LLAMA_CONFIGS["llama-tiny"], intermediate_size=704), dtype=dtype)
    return LlamaForCausalLM(cfg, device=device).eval()


def _pair(kind, head=False, dtype="float32"):
    """(quantised model, twin holding the dequantised values) from one seed."""
    quant, twin = tiny(kind, "cpu", dtype), tiny(kind, "cpu", dtype)
    names = twin._quant_weights + (("lm_head",) if head else ())
    sd = twin.state_dict()  # canonical layout: columns permuted only, and a group lies inside one column
    for k in list(sd):
        if k.split(".")[-1] in names and (head or k.startswith("layers.")):
            sd[k] = ops.quantize_weight_mxfp4(sd[k]).dequant(sd[k].dtype)
    twin.load_state_dict(sd)
    assert quant.quantize_weights("mxfp4", include_head=head) is quant
    return quant, twin


@pytest.mark.parametrize("kind,head,dtype", [("llama", False, "float32"), ("llama", True, "bfloat16"),
                                             ("gpt", False, "float32")])
def test_quantised_model_equals_its_dequantised_twin(kind, head, dtype):
    quant, twin = _pair(kind, head, dtype)
    conv = [(layer, n) for layer in quant.layers for n in quant._quant_weights] + [(quant, "lm_head")] * head
    assert all(isinstance(getattr(m, n), ops.Mxfp4Weight) and n not in dict(m.named_parameters()) for m, n in conv)
    ids = torch.randint(1, quant.cfg.vocab_size, (2, 12), generator=torch.Generator().manual_seed(2))
    toks, _ = quant.generate(ids[:, :5], 12)
    assert torch.equal(toks, twin.generate(ids[:, :5], 12)[0])
    assert torch.equal(toks, quant.generate(ids[:, :5], 12, cache="paged", block_size=16)[0])
    for paged in (False, True):
        logits = []
        for model in (quant, twin):
            cache = model.init_cache(2, 12, paged=paged)
            logits.append(torch.stack([model.prefill(ids[:, :4], cache)] +
                                      [model.decode_step(ids[:, t], cache) for t in range(4, 12)], 1))
        assert torch.equal(*logits)
    with torch.no_grad():
        assert torch.equal(quant(ids), twin(ids))


@pytest.mark.parametrize("kind", ["llama", "gpt"])
def test_layer_bytes(kind):
    model = tiny(kind, "cpu", "bfloat16")
    nbytes = lambda: sum(t.numel() * t.element_size() for t in [*model.layers.parameters(), *model.layers.buffers()])  # noqa: E731
    before = nbytes()
    small = sum(p.numel() * p.element_size() for p in model.layers.parameters() if p.dim() == 1)
    model.quantize_weights("mxfp4")
    assert nbytes() <= (0.5 + 1 / 32) / 2 * (before - small) + small
