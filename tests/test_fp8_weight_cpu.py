"""FP8 weight-only quantisation on the CPU (ops/skinny_fp8.py, GenerationMixin.quantize_weights):
the quantiser's contract, the op's dequant path, and quantised models against a twin that holds
the dequantised values -- bit for bit, because power-of-two column scales make ``q * scale``
exact in bf16 and fp32."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.autograd import tape
from test_generation_cpu import MODELS, make_model


# ------------------------------------------------------------------ quantiser
def _weight():
    """[688, 256] bf16: column c scaled by 2^(c % 41 - 20), column 7 all zero, column 9 one huge
    outlier over small values."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(688, 256, generator=g) * torch.exp2((torch.arange(256) % 41 - 20).float())
    w[:, 7] = 0
    w[:, 9] = torch.randn(688, generator=g) * 1e-3
    w[100, 9] = 2.0 ** 15
    return w.bfloat16()


def test_quantiser_contract():
    w = _weight()
    w8 = ops.quantize_weight_fp8(w)
    q, s = w8.q, w8.scale
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape == w8.shape
    assert s.dtype == torch.float32 and s.shape == (256,) and w8.nbytes == 688 * 256 + 4 * 256
    m, _ = torch.frexp(s)
    assert (m == 0.5).all(), "every scale is a power of two"
    amax = w.float().abs().amax(0)
    nz = amax > 0
    ratio = amax[nz] / s[nz]
    assert (ratio > 224).all() and (ratio <= 448).all()
    assert ((q.view(torch.uint8) & 0x7F) != 0x7F).all(), "a NaN code"
    deq = w8.dequant()
    assert deq.dtype == torch.bfloat16 and deq.data_ptr() != w8.dequant().data_ptr()
    assert torch.equal(deq.float(), q.float() * s), "q * scale is exact in bf16"
    # half an ulp of a 3-bit mantissa plus half the subnormal step
    err = (deq.double() - w.double()).abs()
    bound = 2.0 ** -4 * w.double().abs() + 2.0 ** -10 * s.double()
    print(f"quantiser: max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()
    assert s[7] == 1 and (q[:, 7].float() == 0).all()
    assert q[100, 9].float() * s[9] == w[100, 9].float()  # the outlier sets the scale and survives


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_quantiser_refuses_non_finite(bad):
    w = _weight()
    w[3, 5] = bad
    with pytest.raises(ValueError):
        ops.quantize_weight_fp8(w)


# ------------------------------------------------------------------ the op on the CPU
def test_op_equals_the_dequant_path_on_cpu():
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(688, 256, generator=g) * 688 ** -0.5).bfloat16()
    w8 = ops.quantize_weight_fp8(w)
    wd = w8.dequant().float()
    x = torch.randn(5, 688, generator=g)
    b = torch.randn(256, generator=g)
    assert not ops.skinny_fp8_ok(x, w8)
    for bias, act in [(None, None), (b, None), (b, "gelu_tanh"), (None, "swiglu_interleaved")]:
        got = ops.skinny_linear(x, w8, bias, act)
        want = ops.skinny_linear(x, wd, bias, act)
        assert got.shape == (5, 128 if act == "swiglu_interleaved" else 256)
        assert torch.equal(got, want), f"bias={bias is not None} act={act}"
    with pytest.raises(ValueError):
        ops.skinny_linear(x, w8, act="relu")


# ------------------------------------------------------------------ models
_models = {}


def trio(kind):
    """(unquantised model, quantised model, twin holding the dequantised values), fp32 on the
    CPU, all from one seed; shared, unchanged."""
    if kind not in _models:
        base, twin = make_model(kind), make_model(kind)
        sd = twin.state_dict()  # canonical layout; the quantiser is per column, so it commutes
        names = twin._quant_weights
        for k in list(sd):
            if k.startswith("layers.") and k.split(".")[-1] in names:
                sd[k] = ops.quantize_weight_fp8(sd[k]).dequant(torch.float32)
        twin.load_state_dict(sd)
        quant = make_model(kind)
        assert quant.quantize_weights() is quant
        _models[kind] = (base, quant, twin)
    return _models[kind]


def _teacher_forced(model, ids, P, paged=False):
    B, S = ids.shape
    cache = model.init_cache(B, S, paged=paged)
    out = [model.prefill(ids[:, :P], cache)]
    for t in range(P, S):
        out.append(model.decode_step(ids[:, t], cache))
    return torch.stack(out, 1)


@pytest.mark.parametrize("kind", MODELS)
def test_quantised_model_equals_its_dequantised_twin(kind):
    base, quant, twin = trio(kind)
    for layer in quant.layers:
        for n in quant._quant_weights:
            assert isinstance(getattr(layer, n), ops.Fp8Weight) and n not in dict(layer.named_parameters())
    ids = torch.randint(1, base.cfg.vocab_size, (2, 12), generator=torch.Generator().manual_seed(2))
    toks, _ = quant.generate(ids[:, :5], 12)
    assert torch.equal(toks, twin.generate(ids[:, :5], 12)[0])
    assert torch.equal(toks, quant.generate(ids[:, :5], 12, cache="paged", block_size=16)[0])
    got = _teacher_forced(quant, ids, 4)
    assert torch.equal(got, _teacher_forced(twin, ids, 4))
    assert torch.equal(got, _teacher_forced(quant, ids, 4, paged=True))
    with torch.no_grad():
        assert torch.equal(quant(ids), twin(ids))  # the plain inference forward
        ref = base(ids)[:, 3:]
    print(f"{kind}: logits of the quantised model against the unquantised one, norm ratio "
          f"{((got - ref).norm() / ref.norm()).item():.3e}")


def test_quantisation_changes_some_tokens():
    differ = []
    for kind in MODELS:
        base, quant, _ = trio(kind)
        ids = torch.randint(1, base.cfg.vocab_size, (4, 6), generator=torch.Generator().manual_seed(3))
        differ.append(not torch.equal(base.generate(ids, 24)[0], quant.generate(ids, 24)[0]))
    print("tokens differ from the unquantised model:", dict(zip(MODELS, differ)))
    assert any(differ)


def test_include_head():
    quant, twin = make_model("llama"), make_model("llama")
    sd = twin.state_dict()
    for k in list(sd):
        if k.split(".")[-1] in twin._quant_weights + ("lm_head",):
            sd[k] = ops.quantize_weight_fp8(sd[k]).dequant(torch.float32)
    twin.load_state_dict(sd)
    quant.quantize_weights(include_head=True)
    assert isinstance(quant.lm_head, ops.Fp8Weight)
    ids = torch.randint(1, 512, (2, 5), generator=torch.Generator().manual_seed(4))
    assert torch.equal(quant.generate(ids, 6)[0], twin.generate(ids, 6)[0])
    with pytest.raises(ValueError):
        make_model("gpt").quantize_weights(include_head=True)  # a tied head stays bf16


@pytest.mark.parametrize("kind", MODELS)
def test_layer_bytes_halve(kind):
    model = make_model(kind, "cpu", "bfloat16")

    def layer_bytes():
        ts = list(model.layers.parameters()) + list(model.layers.buffers())
        return sum(t.numel() * t.element_size() for t in ts)

    before = layer_bytes()
    small = sum(p.numel() * p.element_size() for p in model.layers.parameters() if p.dim() == 1)
    cols = sum(getattr(layer, n).shape[1] for layer in model.layers for n in model._quant_weights)
    model.quantize_weights()
    after = layer_bytes()
    print(f"{kind}: decoder layers {before} -> {after} bytes")
    assert after <= 0.5 * before + 4 * cols + small
    assert after < 0.52 * before


def test_out_of_scope_raises():
    quant = trio("llama")[1]
    ids = torch.randint(1, 512, (1, 4))
    with pytest.raises(RuntimeError, match="already quantised"):
        quant.quantize_weights()
    with pytest.raises(ValueError, match="fmt"):
        make_model("gpt").quantize_weights(fmt="int4")
    tp_model = make_model("gpt")
    tp_model.tp = object()
    with pytest.raises(NotImplementedError, match="tensor parallel"):
        tp_model.quantize_weights()
    with pytest.raises(RuntimeError, match="inference only"):
        quant(ids)  # gradients enabled
    with torch.no_grad(), tape.recording(), pytest.raises(RuntimeError, match="inference only"):
        quant(ids)
    with pytest.raises(NotImplementedError, match="state_dict"):
        quant.state_dict()
    with pytest.raises(NotImplementedError, match="state_dict"):
        quant.load_state_dict({})
    bad = make_model("gpt")
    with torch.no_grad():
        bad.layers[1].fc1_w[0, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        bad.quantize_weights()
    assert isinstance(bad.layers[0].qkv_w, torch.nn.Parameter)  # nothing was converted
