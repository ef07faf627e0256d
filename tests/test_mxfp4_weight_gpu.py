"""The MXFP4 weight-only decode GEMM (csrc/kernels/gemm_skinny_mxfp4.hip, ops/skinny_mxfp4.py)
and quantised models on the GPU.

References are fp64 on the CPU from the bf16 ``x`` and the dequantised weight.  Plain product /
bias bound, per element, that of test_fp8_weight_gpu.py:

    |got - ref| <= 2^-8 |ref| + K * 2^-22 * (|x| @ |dq|)

one bf16 rounding with a factor 2 plus the first-order bound of an fp32 sum of K terms in any
order with a factor 2; the e2m1 -> bf16 conversion with its scale is exact.  Activations: the same
rounding term plus that sum bound ``d`` pushed through the activation, |f'| <= 1.13 for GELU and
<= 1.1 for SiLU: ``1.13 d`` and ``1.1 |u| dg + |silu g| du + 1.1 dg du``."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import _native as N
from paddle_amd.ops import skinny_mxfp4
from paddle_amd.utils import flags
from test_mxfp4_weight_cpu import tiny

pytestmark = pytest.mark.gpu

dev = "cuda"
lin = skinny_mxfp4.skinny_kernel  # the kernel itself, whatever the routing and the flag say
_data = {}


def on_gpu(w4):
    return ops.Mxfp4Weight(w4.packed.to(dev), w4.scale_e8m0.to(dev))


def problem(K, Nn):
    """16 rows of x, a quantised weight and a bias for (K, N), with the fp64 products of x and
    the dequantised weight; shared, unchanged."""
    if (K, Nn) not in _data:
        g = torch.Generator().manual_seed(1000 * K + Nn)
        x = torch.randn(16, K, generator=g).bfloat16()
        b = torch.randn(Nn, generator=g).bfloat16()
        w4 = ops.quantize_weight_mxfp4((torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16())
        xd, wd = x.double(), w4.dequant().double()
        ref = xd @ wd
        _data[K, Nn] = dict(x=x.to(dev), w4=on_gpu(w4), wd=w4.dequant(), b=b.to(dev), ref=ref, refb=ref + b.double(),
                            d=K * 2.0 ** -22 * (xd.abs() @ wd.abs()), K=K, N=Nn)
    return _data[K, Nn]


def check(got, ref, slack, what):
    got = got.double().cpu()
    err, bound = (got - ref).abs(), 2.0 ** -8 * ref.abs() + slack
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err/bound {worst:.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{what}: err/bound {worst:.3f}"


class count_launches:
    def __enter__(self):
        self.n, self._orig, skinny_mxfp4._launch = 0, skinny_mxfp4._launch, self._counted
        return self

    def _counted(self, *a, **k):
        self.n += 1
        return self._orig(*a, **k)

    def __exit__(self, *exc):
        skinny_mxfp4._launch = self._orig


# one group; a K tail inside the last 128-k step; one workgroup tile; a ragged last workgroup; many chunks + split-K
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("K,Nn", [(32, 16), (160, 48), (128, 64), (416, 272), (4128, 80)])
def test_plain_and_bias(K, Nn, M):
    d = problem(K, Nn)
    x = d["x"][:M]
    assert torch.equal(d["w4"].dequant().cpu(), d["wd"]), "pa_mxfp4w_dequant against the torch unpack"
    assert ops.skinny_mxfp4_ok(x, d["w4"]) and ops.skinny_mxfp4_ok(x, d["w4"], bias=d["b"])
    with count_launches() as c:
        got = ops.skinny_linear(x, d["w4"])
        gotb = ops.skinny_linear(x.view(1, M, K), d["w4"], d["b"].float())
    assert c.n == 2 and got.shape == (M, Nn) and gotb.shape == (1, M, Nn) and got.dtype == torch.bfloat16
    check(got, d["ref"][:M], d["d"][:M], f"mxfp4 {K}x{Nn} M={M}")
    check(gotb[0], d["refb"][:M], d["d"][:M], f"mxfp4+bias {K}x{Nn} M={M}")


@pytest.mark.parametrize("M", range(1, 17))
def test_activations(M):
    d = problem(416, 288)
    x, dd = d["x"][:M], d["d"][:M]
    got = lin(x, d["w4"], bias=d["b"], act="gelu_tanh")
    check(got, torch.nn.functional.gelu(d["refb"][:M], approximate="tanh"), 1.13 * dd, f"gelu M={M}")
    got = lin(x, d["w4"], act="swiglu_interleaved")
    assert got.shape == (M, 144)
    (g, u), (dg, du) = ops.deinterleave_gate_up(d["ref"][:M]), ops.deinterleave_gate_up(dd)
    silu = g * torch.sigmoid(g)
    check(got, silu * u, 1.1 * u.abs() * dg + silu.abs() * du + 1.1 * dg * du, f"swiglu M={M}")


@pytest.mark.parametrize("splits", [1, 2, 7])  # 7: K has four 128-k steps, slices 4..6 are empty
def test_forced_num_splits(splits):
    d = problem(416, 272)
    x = d["x"][:5]
    with count_launches() as c:
        got = lin(x, d["w4"], bias=d["b"], num_splits=splits)
    assert c.n == 1
    check(got, d["refb"][:5], d["d"][:5], f"splits={splits}")
    assert torch.equal(lin(x, d["w4"], bias=d["b"], num_splits=splits), got), "two runs differ"


@pytest.mark.parametrize("K,Nn,kw", [(4128, 80, {}), (416, 272, dict(num_splits=2)), (416, 272, dict(bias="b")),
                                     (416, 288, dict(act="swiglu_interleaved"))])
def test_row_invariance_and_run_to_run_bits(K, Nn, kw):
    d = problem(K, Nn)
    assert ops.skinny_mxfp4_default_splits(80, 4128) > 1
    kw = {k: d[v] if k == "bias" else v for k, v in kw.items()}
    full = lin(d["x"], d["w4"], **kw)
    for i in range(16):
        assert torch.equal(lin(d["x"][i:i + 1], d["w4"], **kw), full[i:i + 1]), f"row {i}"
    assert torch.equal(lin(d["x"], d["w4"], **kw), full), "two runs differ"


def test_every_code_at_every_scale():
    """[96, 16]: every group holds the 16 codes twice, with scales 2^-100, 1 and 2^100; one-hot rows
    of x pick one weight row each, so the fp64 product rounded to bf16 is the exact value."""
    codes = ((torch.arange(96)[:, None] + torch.arange(16)[None]) % 16).to(torch.uint8)
    w4 = ops.Mxfp4Weight(skinny_mxfp4._pack(codes), torch.tensor([27, 127, 227], dtype=torch.uint8)[:, None].repeat(1, 16))
    dq = w4.dequant(torch.float32)
    assert dq.abs().max() == 6 * 2.0 ** 100 and dq[dq != 0].abs().min() == 2.0 ** -101
    w4g = on_gpu(w4)
    assert torch.equal(w4g.dequant().cpu().float(), dq)
    eye = torch.eye(96, dtype=torch.bfloat16)
    for r in range(0, 96, 16):
        want = (eye[r:r + 16].double() @ dq.double()).bfloat16()
        assert torch.equal(lin(eye[r:r + 16].to(dev), w4g).cpu(), want), f"rows {r}..{r + 15}"


@pytest.mark.parametrize("M", [1, 5])
def test_nothing_outside_the_operands_is_touched(M):
    K, Nn = 416, 272
    d = problem(K, Nn)
    xb = torch.full((16, K), float("nan"), dtype=torch.bfloat16, device=dev)
    xb[:M] = d["x"][:M]
    for splits in (1, 2):
        ob = torch.full((M + 2, Nn + 16), float("nan"), dtype=torch.bfloat16, device=dev)
        out = ob[1:1 + M, 8:8 + Nn]
        ws = torch.empty(splits * M * Nn, dtype=torch.float32, device=dev)
        skinny_mxfp4._launch(xb[:M], d["w4"].packed, d["w4"].scale_e8m0, out, d["b"], ws, M, Nn, K, 1, splits)
        check(out, d["refb"][:M], d["d"][:M], f"poisoned M={M} splits={splits}")
        inside = torch.zeros_like(ob, dtype=torch.bool)
        inside[1:1 + M, 8:8 + Nn] = True
        assert torch.isnan(ob[~inside]).all(), "a store landed outside the output view"


def test_refusals_take_the_dequant_path():
    ok, (A, B, C, S) = N.lib().pa_gemm_skinny_mxfp4_ok, (0x10000, 0x20000, 0x30000, 0x40000)
    assert ok(16, 64, 64, 64, 64, 0, 1, A, B, C, None, S)
    for M, Nn, K in [(17, 64, 64), (0, 64, 64), (4, 40, 64), (4, 64, 48), (4, 1 << 20, 1 << 13)]:  # the last: 4 GiB of codes
        assert not ok(M, Nn, K, K, Nn, 0, 1, A, B, C, None, S), (M, Nn, K)
    d = problem(416, 272)
    x17 = torch.randn(17, 416, device=dev).bfloat16()
    g = torch.Generator().manual_seed(9)
    w40 = on_gpu(ops.quantize_weight_mxfp4(torch.randn(96, 40, generator=g).bfloat16()))  # N % 16 != 0
    x40 = torch.randn(4, 96, generator=g).bfloat16().to(dev)
    with count_launches() as c:
        for x, w4 in [(x17, d["w4"]), (d["x"][:4].float(), d["w4"]), (x40, w40)]:
            assert not ops.skinny_mxfp4_ok(x, w4)
            got = ops.skinny_linear(x, w4)
            assert got.dtype == x.dtype and torch.equal(got, ops.skinny_linear(x, w4.dequant(x.dtype)))
        prev = flags.get("skinny_mxfp4")
        flags.set("skinny_mxfp4", False)
        try:
            assert not ops.skinny_mxfp4_ok(d["x"][:4], d["w4"])
            got = ops.skinny_linear(d["x"][:4], d["w4"], d["b"])
        finally:
            flags.set("skinny_mxfp4", prev)
        assert torch.equal(got, ops.skinny_linear(d["x"][:4], d["wd"].to(dev), d["b"]))
    assert c.n == 0 and ops.skinny_mxfp4_ok(d["x"][:4], d["w4"])
    with pytest.raises(ValueError):
        lin(x40, w40)


def _logits(model, ids, P):
    cache = model.init_cache(ids.shape[0], ids.shape[1])
    out = [model.prefill(ids[:, :P], cache)] + [model.decode_step(ids[:, t], cache) for t in range(P, ids.shape[1] - 1)]
    return torch.stack(out, 1).double().cpu()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["llama", "gpt"])
def test_quantised_models(kind, B):
    """The existing model test's tolerance: against an fp32 model holding the dequantised weights,
    the error of the decode steps on the mxfp4 kernel is at most twice that of the same steps with
    FLAGS_skinny_mxfp4=0 (dequant + the bf16 path)."""
    quant, ref = tiny(kind, dev, "bfloat16"), tiny(kind, dev, "float32")
    ref.load_state_dict({k: v.float() for k, v in quant.state_dict().items()})
    quant.quantize_weights("mxfp4")
    for lq, lr in zip(quant.layers, ref.layers):
        for n in quant._quant_weights:
            getattr(lr, n).data.copy_(getattr(lq, n).dequant(torch.float32))
    torch.manual_seed(3)
    ids = torch.randint(1, quant.cfg.vocab_size, (B, 16), device=dev)
    want = _logits(ref, ids, 8)
    with count_launches() as c:
        on = _logits(quant, ids, 8)
    assert c.n == 7 * 4 * quant.cfg.num_hidden_layers  # four products per layer and decode step
    with count_launches() as c:
        toks, _ = quant.generate(ids[:, :6], 8)
    assert c.n > 0
    flags.set("skinny_mxfp4", False)
    try:
        with count_launches() as c:
            off = _logits(quant, ids, 8)
    finally:
        flags.set("skinny_mxfp4", True)
    assert c.n == 0
    e_on, e_off = ((on - want).norm() / want.norm()).item(), ((off - want).norm() / want.norm()).item()
    print(f"{kind} B={B}: E_on {e_on:.3e}  E_off {e_off:.3e}")
    assert torch.isfinite(on).all() and e_on <= 2 * e_off
    assert torch.equal(quant.generate(ids[:, :6], 8, graph=True)[0], toks)
