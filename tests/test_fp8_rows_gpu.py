"""The weight-only e4m3 GEMM for 17..256 rows (csrc/kernels/gemm_rows_f8.hip, ops/rows_fp8.py)
and quantised models above 16 rows.  References are fp64 on the CPU from the bf16 ``x`` and
``w8.dequant()``; the bound is test_fp8_weight_gpu.py's, |got - ref| <= 2^-8 |ref| + K * 2^-22 *
(|x| @ |dq|), pushed through the activations by test_mxfp4_rows_gpu.py's ``check`` helpers."""
import pytest
import torch

import test_moe_decode_cpu as MC
from paddle_amd import ops
from paddle_amd.ops import _native as N
from paddle_amd.ops import rows_fp8, skinny_fp8
from paddle_amd.utils import flags
from test_generation_cpu import make_model
from test_kv_fp8_gpu import knobs
from test_mxfp4_rows_gpu import _logits, check, check_swiglu, count_launches

pytestmark = pytest.mark.gpu

dev, _data = "cuda", {}
rows = rows_fp8.rows_kernel  # the kernel itself, whatever the routing and the flag say


def on_gpu(w8):
    return ops.Fp8Weight(w8.q.to(dev), w8.scale.to(dev))


def problem(K, Nn):
    """256 rows of x, a quantised weight, a bias and their fp64 products; shared, unchanged."""
    if (K, Nn) not in _data:
        g = torch.Generator().manual_seed(1000 * K + Nn)
        x = torch.randn(256, K, generator=g).bfloat16()
        b = torch.randn(Nn, generator=g).bfloat16()
        w8 = ops.quantize_weight_fp8((torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16())
        xd, wd = x.double(), w8.dequant().double()
        ref = xd @ wd
        _data[K, Nn] = dict(x=x.to(dev), w8=on_gpu(w8), b=b.to(dev), ref=ref, refb=ref + b.double(),
                            d=K * 2.0 ** -22 * (xd.abs() @ wd.abs()))
    return _data[K, Nn]


# M: first row of a second 16-row tile, a partial tile, one 64-row tile, one row past it, ragged, the maximum
# (K, N): half an MFMA step; a K tail inside a step; a ragged last workgroup; many A chunks + default split-K
@pytest.mark.parametrize("M", [17, 33, 64, 65, 100, 256])
@pytest.mark.parametrize("K,Nn", [(16, 16), (144, 48), (400, 272), (4112, 80)])
def test_plain_and_bias(K, Nn, M):
    d = problem(K, Nn)
    x = d["x"][:M]
    assert ops.rows_fp8_default_splits(80, 4112) == 8
    routed = M <= rows_fp8.ROUTED_ROWS  # beyond the measured routing bound: the kernel entry
    assert ops.fp8_linear_ok(x, d["w8"]) == ops.fp8_linear_ok(x, d["w8"], bias=d["b"]) == routed
    lin = ops.fp8_linear if routed else (lambda x, w, b=None: rows(x, w, bias=b))
    with count_launches(rows_fp8) as c:
        got = lin(x, d["w8"])
        gotb = lin(x.view(1, M, K), d["w8"], d["b"].float())[0]
    assert c.n == 2 and got.shape == gotb.shape == (M, Nn) and got.dtype == torch.bfloat16
    check(got, d["ref"][:M], d["d"][:M], f"rows {K}x{Nn} M={M}")
    check(gotb, d["refb"][:M], d["d"][:M], f"rows+bias {K}x{Nn} M={M}")


@pytest.mark.parametrize("M", [17, 40, 65])
def test_activations(M):
    d = problem(400, 288)
    x, dd = d["x"][:M], d["d"][:M]
    got = rows(x, d["w8"], bias=d["b"], act="gelu_tanh")
    check(got, torch.nn.functional.gelu(d["refb"][:M], approximate="tanh"), 1.13 * dd, f"gelu M={M}")
    got = rows(x, d["w8"], act="swiglu_interleaved")
    assert got.shape == (M, 144)
    check_swiglu(got, d["ref"][:M], dd, f"swiglu M={M}")


@pytest.mark.parametrize("splits", [1, 2, 7])  # 7: K has four 128-k steps, slices 4..6 are empty
def test_forced_num_splits(splits):
    d = problem(400, 272)
    x = d["x"][:37]
    with count_launches(rows_fp8) as c:
        got = rows(x, d["w8"], bias=d["b"], num_splits=splits)
    assert c.n == 1
    check(got, d["refb"][:37], d["d"][:37], f"splits={splits}")
    assert torch.equal(rows(x, d["w8"], bias=d["b"], num_splits=splits), got), "two runs differ"


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("Nn,kw", [(272, {}), (272, dict(bias="b")), (288, dict(act="swiglu_interleaved"))])
def test_row_invariance(Nn, kw, splits):
    d = problem(400, Nn)
    kw = dict({k: d[v] if k == "bias" else v for k, v in kw.items()}, num_splits=splits)
    x = d["x"][:100]
    full = rows(x, d["w8"], **kw)
    for r in range(0, 100, 16):
        assert torch.equal(rows(x[r:r + 16], d["w8"], **kw), full[r:r + 16]), f"rows {r}.."
    assert torch.equal(rows(x[99:], d["w8"], **kw), full[99:]), "row 99 alone"


def test_every_code_at_the_scale_extremes():
    # row k holds code byte k (the NaN codes replaced by 0); the one-hot rows of x pick one row each
    codes = torch.arange(256, dtype=torch.uint8)
    codes[[0x7F, 0xFF]] = 0
    q = codes[:, None].repeat(1, 48).view(torch.float8_e4m3fn)
    w8 = ops.Fp8Weight(q, torch.tensor([2.0 ** -100, 1.0, 2.0 ** 100]).repeat(16))
    want = w8.dequant(torch.float32).bfloat16()
    assert torch.equal(rows(torch.eye(256, dtype=torch.bfloat16, device=dev), on_gpu(w8)).cpu(), want)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("M", [17, 65])
def test_nothing_outside_the_operands_is_touched(M, splits):
    K, Nn = 400, 272
    d = problem(K, Nn)
    xb = torch.full((M + 15, K), float("nan"), dtype=torch.bfloat16, device=dev)
    xb[:M] = d["x"][:M]
    ob = torch.full((M + 2, Nn + 16), float("nan"), dtype=torch.bfloat16, device=dev)
    out = ob[1:1 + M, 8:8 + Nn]
    ws = torch.empty(splits * M * Nn, dtype=torch.float32, device=dev)
    rows_fp8._launch(xb[:M], d["w8"].q, d["w8"].scale, out, d["b"], ws, M, Nn, K, 1, splits)
    check(out, d["refb"][:M], d["d"][:M], f"poisoned M={M} splits={splits}")
    inside = torch.zeros_like(ob, dtype=torch.bool)
    inside[1:1 + M, 8:8 + Nn] = True
    assert torch.isnan(ob[~inside]).all(), "a store landed outside the output view"


def test_refusals():
    lib, (A, B, C, S) = N.lib(), (0x10000, 0x20000, 0x30000, 0x40000)
    assert lib.pa_gemm_rows_f8_ok(256, 64, 64, 64, 64, 64, 0, 1, A, B, C, None, S)
    # M 0 and 257, N 40, K 24, a misaligned x, a slab of 2^34 floats
    for M, Nn, K, a, splits in [(0, 64, 64, A, 1), (257, 64, 64, A, 1), (20, 40, 64, A, 1), (20, 64, 24, A, 1),
                                (20, 64, 64, A + 8, 1), (256, 1 << 16, 16, A, 1024)]:
        assert not lib.pa_gemm_rows_f8_ok(M, Nn, K, K, Nn, Nn, 0, splits, a, B, C, None, S), (M, Nn, K)
        assert lib.pa_gemm_rows_f8(a, B, Nn, S, C, None, 0, A, M, Nn, K, K, Nn, 0, splits, None) != 0  # launches nothing
    d = problem(400, 272)
    x300 = torch.cat([d["x"], d["x"][:44]])
    prev_routed, rows_fp8.ROUTED_ROWS = rows_fp8.ROUTED_ROWS, 256  # 300 rows are refused whatever was measured
    try:
        with count_launches(rows_fp8) as c, count_launches(skinny_fp8) as cs:
            for x, b in ((x300, d["b"]), (d["x"][:20].float(), None)):
                assert not ops.fp8_linear_ok(x, d["w8"], b)
                assert torch.equal(ops.fp8_linear(x, d["w8"], b), ops.skinny_linear(x, d["w8"], b))
            flags.set("fp8_rows", False)
            try:
                assert not ops.fp8_linear_ok(d["x"][:20], d["w8"])
                got = ops.fp8_linear(d["x"][:20], d["w8"], d["b"])
            finally:
                flags.set("fp8_rows", True)
            assert torch.equal(got, ops.skinny_linear(d["x"][:20], d["w8"], d["b"]))
            assert c.n == 0 and cs.n == 0
            assert not ops.fp8_linear_ok(d["x"][:16], d["w8"])
            ops.fp8_linear(d["x"][:16], d["w8"])
            assert c.n == 0 and cs.n == 1
    finally:
        rows_fp8.ROUTED_ROWS = prev_routed
    with pytest.raises(ValueError):
        rows(x300, d["w8"])


@pytest.mark.parametrize("kind", ["llama", "gpt", "ernie"])
def test_quantised_models(kind):
    """test_mxfp4_rows_gpu's rule: against an fp32 model holding the dequantised weights (ERNIE-MoE:
    on the CPU), the error with the kernel is at most twice that with FLAGS_fp8_rows=0; greedy tokens
    are not compared.  A dense model's decode step at B 20 launches no dequantised weight image."""
    make = (lambda d, t: MC.make_ernie("grouped_shared", d, t)) if kind == "ernie" else (lambda d, t: make_model(kind, d, t))
    rdev = "cpu" if kind == "ernie" else dev
    quant, ref = make(dev, "bfloat16"), make(rdev, "float32")
    ref.load_state_dict({k: v.float().to(rdev) for k, v in quant.state_dict().items()})
    quant.quantize_weights()
    for (mq, n), (mr, _) in zip(quant._quant_targets(), ref._quant_targets()):
        getattr(mr, n).data.copy_(getattr(mq, n).dequant(torch.float32))
    per_pass = sum(isinstance(m, ops.Fp8Weight) for m in quant.modules())
    assert per_pass == (12 if kind == "ernie" else 4 * quant.cfg.num_hidden_layers)
    torch.manual_seed(3)
    ids = torch.randint(1, quant.cfg.vocab_size, (20, 12), device=dev)
    want = _logits(ref, ids.to(rdev))
    with count_launches(rows_fp8) as c:
        on = _logits(quant, ids)
    assert c.n == (3 + 1) * per_pass  # every Fp8Weight once per decode step and extend
    flags.set("fp8_rows", False)
    try:
        with count_launches(rows_fp8) as c:
            off = _logits(quant, ids)
    finally:
        flags.set("fp8_rows", True)
    assert c.n == 0
    e_on, e_off = ((on - want).norm() / want.norm()).item(), ((off - want).norm() / want.norm()).item()
    print(f"{kind}: E_on {e_on:.3e}  E_off {e_off:.3e}")
    assert torch.isfinite(on).all() and e_on <= 2 * e_off
    if kind != "ernie":
        cache = quant.init_cache(20, 12)
        quant.prefill(ids[:, :8], cache)
        with knobs() as calls:
            quant.decode_step(ids[:, 8], cache)
        assert not [n for n in calls if "dequant" in n], calls
