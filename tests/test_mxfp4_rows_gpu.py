"""The MXFP4 weight GEMM for 17..256 rows (csrc/kernels/gemm_rows_mxfp4.hip, ops/rows_mxfp4.py)
and quantised models above 16 rows on the GPU.

References are fp64 on the CPU from the bf16 ``x`` and the dequantised weight; the bounds are
those of test_mxfp4_weight_gpu.py (derived there):

    |got - ref| <= 2^-8 |ref| + K * 2^-22 * (|x| @ |dq|)

and that sum bound ``d`` pushed through the activations, ``1.13 d`` for GELU and
``1.1 |u| dg + |silu g| du + 1.1 dg du`` for SwiGLU."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import _native as N
from paddle_amd.ops import rows_mxfp4, skinny_mxfp4
from paddle_amd.utils import flags
from test_mxfp4_weight_cpu import tiny

pytestmark = pytest.mark.gpu

dev = "cuda"
rows = rows_mxfp4.rows_kernel  # the kernel itself, whatever the routing and the flag say
_data = {}


def on_gpu(w4):
    return ops.Mxfp4Weight(w4.packed.to(dev), w4.scale_e8m0.to(dev))


def problem(K, Nn):
    """256 rows of x, a quantised weight and a bias for (K, N), with the fp64 products of x and
    the dequantised weight; shared, unchanged."""
    if (K, Nn) not in _data:
        g = torch.Generator().manual_seed(1000 * K + Nn)
        x = torch.randn(256, K, generator=g).bfloat16()
        b = torch.randn(Nn, generator=g).bfloat16()
        w4 = ops.quantize_weight_mxfp4((torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16())
        xd, wd = x.double(), w4.dequant().double()
        ref = xd @ wd
        _data[K, Nn] = dict(x=x.to(dev), w4=on_gpu(w4), b=b.to(dev), ref=ref, refb=ref + b.double(),
                            d=K * 2.0 ** -22 * (xd.abs() @ wd.abs()))
    return _data[K, Nn]


def check(got, ref, slack, what):
    got = got.double().cpu()
    err, bound = (got - ref).abs(), 2.0 ** -8 * ref.abs() + slack
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err/bound {worst:.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{what}: err/bound {worst:.3f}"


def check_swiglu(got, ref, d, what):
    (g, u), (dg, du) = ops.deinterleave_gate_up(ref), ops.deinterleave_gate_up(d)
    silu = g * torch.sigmoid(g)
    check(got, silu * u, 1.1 * u.abs() * dg + silu.abs() * du + 1.1 * dg * du, what)


class count_launches:
    def __init__(self, mod=rows_mxfp4):
        self.mod = mod

    def __enter__(self):
        self.n, self._orig, self.mod._launch = 0, self.mod._launch, self._counted
        return self

    def _counted(self, *a, **k):
        self.n += 1
        return self._orig(*a, **k)

    def __exit__(self, *exc):
        self.mod._launch = self._orig


# M: first row of a second 16-row tile, a partial tile, one 64-row tile, one row past it, ragged, the maximum
# (K, N): one group; a K tail inside a step; a ragged last workgroup; many A chunks + default split-K
@pytest.mark.parametrize("M", [17, 33, 64, 65, 100, 256])
@pytest.mark.parametrize("K,Nn", [(32, 16), (160, 48), (416, 272), (4128, 80)])
def test_plain_and_bias(K, Nn, M):
    d = problem(K, Nn)
    x = d["x"][:M]
    assert ops.rows_mxfp4_default_splits(80, 4128) > 1
    routed = M <= rows_mxfp4.ROUTED_ROWS  # beyond the measured routing bound: the kernel entry
    assert ops.mxfp4_linear_ok(x, d["w4"]) == ops.mxfp4_linear_ok(x, d["w4"], bias=d["b"]) == routed
    lin = ops.mxfp4_linear if routed else (lambda x, w, b=None: rows(x, w, bias=b))
    with count_launches() as c:
        got = lin(x, d["w4"])
        gotb = lin(x.view(1, M, K), d["w4"], d["b"].float())[0]
    assert c.n == 2 and got.shape == gotb.shape == (M, Nn) and got.dtype == torch.bfloat16
    check(got, d["ref"][:M], d["d"][:M], f"rows {K}x{Nn} M={M}")
    check(gotb, d["refb"][:M], d["d"][:M], f"rows+bias {K}x{Nn} M={M}")


@pytest.mark.parametrize("M", [17, 40, 65])
def test_activations(M):
    d = problem(416, 288)
    x, dd = d["x"][:M], d["d"][:M]
    got = rows(x, d["w4"], bias=d["b"], act="gelu_tanh")
    check(got, torch.nn.functional.gelu(d["refb"][:M], approximate="tanh"), 1.13 * dd, f"gelu M={M}")
    got = rows(x, d["w4"], act="swiglu_interleaved")
    assert got.shape == (M, 144)
    check_swiglu(got, d["ref"][:M], dd, f"swiglu M={M}")


@pytest.mark.parametrize("splits", [1, 2, 7])  # 7: K has four 128-k steps, slices 4..6 are empty
def test_forced_num_splits(splits):
    d = problem(416, 272)
    x = d["x"][:37]
    with count_launches() as c:
        got = rows(x, d["w4"], bias=d["b"], num_splits=splits)
    assert c.n == 1
    check(got, d["refb"][:37], d["d"][:37], f"splits={splits}")
    assert torch.equal(rows(x, d["w4"], bias=d["b"], num_splits=splits), got), "two runs differ"


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("K,Nn,kw", [(4128, 80, {}), (416, 272, {}), (416, 272, dict(bias="b")),
                                     (416, 288, dict(act="swiglu_interleaved"))])
def test_row_invariance_and_the_siblings_bits(K, Nn, kw, splits):
    d = problem(K, Nn)
    kw = dict({k: d[v] if k == "bias" else v for k, v in kw.items()}, num_splits=splits)
    x = d["x"][:100]
    full = rows(x, d["w4"], **kw)
    for r in range(0, 100, 16):
        assert torch.equal(skinny_mxfp4.skinny_kernel(x[r:r + 16], d["w4"], **kw), full[r:r + 16]), f"rows {r}.."
    assert torch.equal(rows(x[99:], d["w4"], **kw), full[99:]), "row 99 alone"


def test_every_code_at_every_scale():
    """test_mxfp4_weight_gpu's [96, 16] weight: every group holds the 16 codes twice, with scales
    2^-100, 1 and 2^100; the one-hot rows of x pick one weight row each."""
    codes = ((torch.arange(96)[:, None] + torch.arange(16)[None]) % 16).to(torch.uint8)
    w4 = ops.Mxfp4Weight(skinny_mxfp4._pack(codes), torch.tensor([27, 127, 227], dtype=torch.uint8)[:, None].repeat(1, 16))
    eye = torch.eye(96, dtype=torch.bfloat16)
    want = (eye.double() @ w4.dequant(torch.float32).double()).bfloat16()
    assert torch.equal(rows(eye.to(dev), on_gpu(w4)).cpu(), want)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("M", [17, 65])
def test_nothing_outside_the_operands_is_touched(M, splits):
    K, Nn = 416, 272
    d = problem(K, Nn)
    xb = torch.full((M + 15, K), float("nan"), dtype=torch.bfloat16, device=dev)
    xb[:M] = d["x"][:M]
    ob = torch.full((M + 2, Nn + 16), float("nan"), dtype=torch.bfloat16, device=dev)
    out = ob[1:1 + M, 8:8 + Nn]
    ws = torch.empty(splits * M * Nn, dtype=torch.float32, device=dev)
    rows_mxfp4._launch(xb[:M], d["w4"].packed, d["w4"].scale_e8m0, out, d["b"], ws, M, Nn, K, 1, splits)
    check(out, d["refb"][:M], d["d"][:M], f"poisoned M={M} splits={splits}")
    inside = torch.zeros_like(ob, dtype=torch.bool)
    inside[1:1 + M, 8:8 + Nn] = True
    assert torch.isnan(ob[~inside]).all(), "a store landed outside the output view"


def test_refusals():
    lib, (A, B, C, S) = N.lib(), (0x10000, 0x20000, 0x30000, 0x40000)
    assert lib.pa_gemm_rows_mxfp4_ok(256, 64, 64, 64, 64, 0, 1, A, B, C, None, S)
    # M 0 and 257, N 40, K 48, a misaligned x, a slab of 2^34 floats
    for M, Nn, K, a, splits in [(0, 64, 64, A, 1), (257, 64, 64, A, 1), (20, 40, 64, A, 1), (20, 64, 48, A, 1),
                                (20, 64, 64, A + 8, 1), (256, 1 << 16, 32, A, 1024)]:
        assert not lib.pa_gemm_rows_mxfp4_ok(M, Nn, K, K, Nn, 0, splits, a, B, C, None, S), (M, Nn, K)
        assert lib.pa_gemm_rows_mxfp4(a, B, S, C, None, 0, A, M, Nn, K, K, Nn, 0, splits, None) != 0  # launches nothing
    d = problem(416, 272)
    x300 = torch.cat([d["x"], d["x"][:44]])
    prev_routed, rows_mxfp4.ROUTED_ROWS = rows_mxfp4.ROUTED_ROWS, 256  # 300 rows are refused whatever was measured
    try:
        with count_launches() as c, count_launches(skinny_mxfp4) as cs:
            for x, b in ((x300, d["b"]), (d["x"][:20].float(), None)):
                assert not ops.mxfp4_linear_ok(x, d["w4"], b)
                assert torch.equal(ops.mxfp4_linear(x, d["w4"], b), ops.skinny_linear(x, d["w4"], b))
            flags.set("mxfp4_rows", False)
            try:
                assert not ops.mxfp4_linear_ok(d["x"][:20], d["w4"])
                got = ops.mxfp4_linear(d["x"][:20], d["w4"], d["b"])
            finally:
                flags.set("mxfp4_rows", True)
            assert torch.equal(got, ops.skinny_linear(d["x"][:20], d["w4"], d["b"]))
            assert c.n == 0 and cs.n == 0
            assert not ops.mxfp4_linear_ok(d["x"][:16], d["w4"])
            ops.mxfp4_linear(d["x"][:16], d["w4"])
            assert c.n == 0 and cs.n == 1
    finally:
        rows_mxfp4.ROUTED_ROWS = prev_routed
    with pytest.raises(ValueError):
        rows(x300, d["w4"])


def _logits(model, ids):
    """Prefill of 8 tokens and three decode steps at B = 20; then, on a second cache, the first 6
    prompts and one extend of 6 rows x 4 tokens."""
    cache = model.init_cache(20, 12)
    out = [model.prefill(ids[:, :8], cache)] + [model.decode_step(ids[:, t], cache) for t in range(8, 11)]
    cache = model.init_cache(6, 12)
    model.prefill(ids[:6, :8], cache)
    out.append(model.extend(ids[:6, 8:12], cache, all_logits=True).reshape(24, -1)[:20])
    return torch.stack(out, 1).double().cpu()


@pytest.mark.parametrize("kind", ["llama", "gpt"])
def test_quantised_models(kind):
    """test_mxfp4_weight_gpu's rule: against an fp32 model holding the dequantised weights, the
    error with the kernel is at most twice that with FLAGS_mxfp4_rows=0 (dequant + the bf16 path).
    Greedy tokens at B = 20 are not asserted equal between the two settings: measured
    (profiles/mxfp4_rows_bench.md), they first differ at step 1 (llama, row 2) and step 2 (GPT, row
    15), where the two candidates' logits are one bf16 ulp (2^-8) apart or tied."""
    quant, ref = tiny(kind, dev, "bfloat16"), tiny(kind, dev, "float32")
    ref.load_state_dict({k: v.float() for k, v in quant.state_dict().items()})
    quant.quantize_weights("mxfp4")
    for lq, lr in zip(quant.layers, ref.layers):
        for n in quant._quant_weights:
            getattr(lr, n).data.copy_(getattr(lq, n).dequant(torch.float32))
    torch.manual_seed(3)
    ids = torch.randint(1, quant.cfg.vocab_size, (20, 12), device=dev)
    want = _logits(ref, ids)
    with count_launches() as c:
        on = _logits(quant, ids)
    assert c.n == (3 + 1) * 4 * quant.cfg.num_hidden_layers  # four products per layer, decode step and extend
    flags.set("mxfp4_rows", False)
    try:
        with count_launches() as c:
            off = _logits(quant, ids)
    finally:
        flags.set("mxfp4_rows", True)
    assert c.n == 0
    e_on, e_off = ((on - want).norm() / want.norm()).item(), ((off - want).norm() / want.norm()).item()
    print(f"{kind}: E_on {e_on:.3e}  E_off {e_off:.3e}")
    assert torch.isfinite(on).all() and e_on <= 2 * e_off
