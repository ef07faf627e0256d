"""The FP8 weight-only decode GEMM (csrc/kernels/gemm_skinny_f8.hip, ops/skinny_fp8.py) and
quantised models on the GPU.

References are fp64 on the CPU from the bf16 ``x`` and the dequantised weight.  Plain product /
bias bound, per element, that of test_skinny_gemm_gpu.py:

    |got - ref| <= 2^-8 |ref| + K * 2^-22 * (|x| @ |w_deq|)

one bf16 rounding with a factor 2 plus the first-order bound of an fp32 sum of K terms in any
order with a factor 2.  It carries over unchanged because the e4m3 -> fp32 conversion is exact
and so is the scaling of the sum by a power of two (a hand-made scale adds one fp32 rounding,
2^-24 relative, inside the first term's slack).

GELU / SwiGLU epilogues and whole models: the norm-ratio error must be at most twice that of
the path they replace on the dequantised weight."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import _native as N
from paddle_amd.ops import skinny, skinny_fp8
from paddle_amd.utils import flags
from test_generation_cpu import MODELS, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
ALL_M = list(range(1, 17))
F8 = torch.float8_e4m3fn


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


_data = {}


def problem(K, Nn):
    """16 rows of x, a quantised weight and a bias for (K, N), with the fp64 products of x and
    the dequantised weight; shared, unchanged."""
    key = (K, Nn)
    if key not in _data:
        g = torch.Generator().manual_seed(1000 * K + Nn)
        x = torch.randn(16, K, generator=g).bfloat16()
        w = (torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16()
        b = torch.randn(Nn, generator=g).bfloat16()
        w8 = ops.quantize_weight_fp8(w)
        xd, wd = x.double(), w8.dequant().double()
        ref = xd @ wd
        _data[key] = dict(x=x.to(dev), w8=w8.to(dev), wd=w8.dequant().to(dev), b=b.to(dev), ref=ref,
                          refb=ref + b.double(), mag=xd.abs() @ wd.abs(), K=K, N=Nn)
    return _data[key]


def check_bound(got, ref, mag, K, what):
    got = got.double().cpu()
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * mag
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err/bound {worst:.3f}")
    assert torch.isfinite(got).all(), what
    assert (err <= bound).all(), f"{what}: err/bound {worst:.3f}"


def swiglu_ref(ref):
    g, u = ops.deinterleave_gate_up(ref)
    return g * torch.sigmoid(g) * u


def swiglu_parent(x, w):
    gu = ops.linear(x, w)
    g, u = ops.deinterleave_gate_up(gu)
    return (torch.nn.functional.silu(g.float()) * u.float()).to(x.dtype)


def gelu_ref(z):
    return torch.nn.functional.gelu(z, approximate="tanh")


def lin(x, w8, bias=None, act=None, num_splits=None):
    """The fp8 kernel itself, whatever the routing and the flag say."""
    return skinny_fp8.skinny_kernel(x, w8, bias=bias, act=act, num_splits=num_splits)


def routed(M):
    """Every row count the kernel covers is routed to it: at 16 rows it still beats dequant +
    ops.linear, the only alternative (profiles/skinny_fp8_bench.md)."""
    return M <= 16


class count_launches:
    """Counts the launches that go through ``mod._launch`` (skinny_fp8: the e4m3 kernel,
    skinny: the bf16 one)."""

    def __init__(self, mod=skinny_fp8):
        self.mod = mod

    def __enter__(self):
        self.n = 0
        self._orig = self.mod._launch

        def wrapped(*a, **k):
            self.n += 1
            return self._orig(*a, **k)

        self.mod._launch = wrapped
        return self

    def __exit__(self, *exc):
        self.mod._launch = self._orig


# ------------------------------------------------------------------ accuracy, every M
@pytest.mark.parametrize("K,Nn", [(8, 16), (256, 768), (688, 256), (264, 528), (256, 1376)])
def test_plain_and_bias(K, Nn):
    d = problem(K, Nn)
    with count_launches() as c:
        for M in ALL_M:
            x = d["x"][:M]
            assert ops.skinny_fp8_ok(x, d["w8"]) == routed(M) == ops.skinny_fp8_ok(x, d["w8"], bias=d["b"])
            got = lin(x, d["w8"])
            if routed(M):  # the public op runs the same kernel
                assert torch.equal(ops.skinny_linear(x, d["w8"]), got)
            assert got.shape == (M, Nn) and got.dtype == torch.bfloat16
            check_bound(got, d["ref"][:M], d["mag"][:M], K, f"f8 {K}x{Nn} M={M}")
            got = lin(x, d["w8"], d["b"])
            if routed(M):
                assert torch.equal(ops.skinny_linear(x, d["w8"], d["b"]), got)
            check_bound(got, d["refb"][:M], d["mag"][:M], K, f"f8+bias {K}x{Nn} M={M}")
    assert c.n == 4 * len(ALL_M)
    # fp32 bias, and x with leading dimensions
    got = lin(d["x"][:6].view(3, 2, K), d["w8"], d["b"].float())
    assert got.shape == (3, 2, Nn)
    check_bound(got.view(6, Nn), d["refb"][:6], d["mag"][:6], K, f"f8+fp32 bias {K}x{Nn}")


def test_scale_that_is_no_power_of_two():
    K, Nn = 264, 528
    d = problem(K, Nn)
    g = torch.Generator().manual_seed(7)
    scale = (d["w8"].scale.cpu() * (0.6 + 0.8 * torch.rand(Nn, generator=g))).contiguous()
    w8 = ops.Fp8Weight(d["w8"].q, scale.to(dev))
    xd = d["x"].double().cpu()
    wd = d["w8"].q.cpu().double() * scale.double()
    ref, mag = xd @ wd, xd.abs() @ wd.abs()
    for M in (1, 5, 8, 16):
        check_bound(lin(d["x"][:M], w8), ref[:M], mag[:M], K, f"hand-made scale M={M}")
    # the dequantiser rounds the fp32 product once
    assert torch.equal(w8.dequant().cpu(), (d["w8"].q.cpu().float() * scale).bfloat16())


# ------------------------------------------------------------------ every code
def test_every_code_decodes_exactly():
    """Row k of the [256, 16] weight holds code k (0x7F / 0xFF, the NaNs, replaced by their
    neighbours 0x7E / 0xFE: two rows repeat); one-hot rows of x pick one code at a time, so each
    output is bf16(code * scale) exactly -- subnormals, +-0 and +-448 included."""
    codes = torch.arange(256, dtype=torch.int32)
    codes[0x7F], codes[0xFF] = 0x7E, 0xFE
    q = codes.to(torch.uint8)[:, None].expand(256, 16).contiguous().view(F8)
    assert torch.isfinite(q.float()).all() and q.float().abs().max() == 448
    scale = torch.exp2((torch.arange(16) % 8 - 3).float())
    want = (q.float() * scale).bfloat16()
    assert torch.equal(want.float(), q.float() * scale)
    w8 = ops.Fp8Weight(q.to(dev), scale.to(dev))
    eye = torch.eye(256, dtype=torch.bfloat16, device=dev)
    for r in range(0, 256, 16):
        got = lin(eye[r:r + 16], w8)
        assert torch.equal(got.cpu().float(), want[r:r + 16].float()), f"codes {r}..{r + 15}"
    assert torch.equal(w8.dequant().cpu().float(), want.float())


# ------------------------------------------------------------------ activations
def test_swiglu_every_m():
    K, Nn = 256, 1376  # llama-tiny gate|up: N is no multiple of the column tile
    d = problem(K, Nn)
    want = swiglu_ref(d["ref"])
    for M in ALL_M:
        x = d["x"][:M]
        with count_launches() as c:
            got = lin(x, d["w8"], act="swiglu_interleaved")
        assert c.n == 1 and got.shape == (M, Nn // 2)
        if routed(M):
            assert torch.equal(ops.skinny_linear(x, d["w8"], act="swiglu_interleaved"), got)
        e_new, e_old = _rel(got, want[:M]), _rel(swiglu_parent(x, d["wd"]), want[:M])
        print(f"swiglu M={M}: f8 {e_new:.3e}  parent {e_old:.3e}")
        assert torch.isfinite(got).all() and e_new <= 2 * e_old


def test_bias_gelu_every_m():
    K, Nn = 256, 768
    d = problem(K, Nn)
    want = gelu_ref(d["refb"])
    for M in ALL_M:
        x = d["x"][:M]
        with count_launches() as c:
            got = lin(x, d["w8"], d["b"], act="gelu_tanh")
        assert c.n == 1 and got.shape == (M, Nn)
        e_new, e_old = _rel(got, want[:M]), _rel(ops.linear_gelu(x, d["wd"], d["b"]), want[:M])
        print(f"gelu M={M}: f8 {e_new:.3e}  parent {e_old:.3e}")
        assert torch.isfinite(got).all() and e_new <= 2 * e_old


# ------------------------------------------------------------------ forced split counts
@pytest.mark.parametrize("K,Nn,M", [(688, 256, 5), (264, 528, 16)])
def test_forced_num_splits(K, Nn, M):
    d = problem(K, Nn)
    x = d["x"][:M]
    for s in (1, 2, 3, 8, K // 8 + 3):  # the last one has slices past the end of K
        with count_launches() as c:
            got = lin(x, d["w8"], d["b"], num_splits=s)
        assert c.n == 1
        check_bound(got, d["refb"][:M], d["mag"][:M], K, f"splits={s} {K}x{Nn} M={M}")
        assert torch.equal(lin(x, d["w8"], d["b"], num_splits=s), got), f"splits={s}: two runs differ"


def test_forced_num_splits_activations():
    d = problem(256, 1376)
    x = d["x"][:5]
    want = swiglu_ref(d["ref"])[:5]
    e_old = _rel(swiglu_parent(x, d["wd"]), want)
    for s in (1, 2, 3, 8, 256 // 8 + 3):
        e_new = _rel(lin(x, d["w8"], act="swiglu_interleaved", num_splits=s), want)
        print(f"swiglu splits={s}: f8 {e_new:.3e}  parent {e_old:.3e}")
        assert e_new <= 2 * e_old
    d = problem(256, 768)
    x = d["x"][:5]
    want = gelu_ref(d["refb"])[:5]
    e_old = _rel(ops.linear_gelu(x, d["wd"], d["b"]), want)
    for s in (1, 2, 3, 8, 256 // 8 + 3):
        e_new = _rel(lin(x, d["w8"], d["b"], act="gelu_tanh", num_splits=s), want)
        print(f"gelu splits={s}: f8 {e_new:.3e}  parent {e_old:.3e}")
        assert e_new <= 2 * e_old


def test_default_splits_come_from_n_and_k_alone():
    for K, Nn in [(688, 256), (264, 528), (256, 1376)]:
        d = problem(K, Nn)
        want = int(N.lib().pa_gemm_skinny_f8_splits(Nn, K))
        assert ops.skinny_fp8_default_splits(Nn, K) == want >= 1
        for M in (1, 3, 8, 16):
            x = d["x"][:M]
            assert skinny_fp8._problem(x, d["w8"], None, None, policy=False)[-1] == want
            assert torch.equal(lin(x, d["w8"]), lin(x, d["w8"], num_splits=want))
    # llama-7b's products: computed on the host, no launch
    for Nn, K in [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)]:
        assert 1 <= ops.skinny_fp8_default_splits(Nn, K) <= 64


# ------------------------------------------------------------------ batch invariance
def _raw(x, q, scale, bias, epi, splits, out=None):
    """One kernel call through skinny_fp8._launch."""
    M, K = x.shape
    Nn = q.shape[1]
    nout = Nn // 2 if epi == 3 else Nn
    if out is None:
        out = torch.empty(M, nout, dtype=torch.bfloat16, device=dev)
    nws = int(N.lib().pa_gemm_skinny_f8_ws_floats(M, Nn, splits))
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dev)
    return skinny_fp8._launch(x, q, scale, out, bias, ws, M, Nn, K, epi, splits)


def test_batch_invariance_and_run_to_run_bits():
    cases = []
    for K, Nn in [(688, 256), (264, 528)]:
        d = problem(K, Nn)
        for s in (1, 3):
            cases += [(d, None, 0, s), (d, d["b"], 2, s)]
    d = problem(256, 1376)
    cases += [(d, None, 3, 1), (d, None, 3, 2)]
    for d, bias, epi, s in cases:
        q, sc = d["w8"].q, d["w8"].scale
        rows = [_raw(d["x"][i:i + 1], q, sc, bias, epi, s) for i in range(16)]
        for M in range(2, 17):
            full = _raw(d["x"][:M], q, sc, bias, epi, s)
            assert torch.equal(full, torch.cat(rows[:M])), f"M={M} {d['K']}x{d['N']} epi={epi} splits={s}"
        assert torch.equal(_raw(d["x"], q, sc, bias, epi, s), full), "two runs differ"
    # and through the op at its default split count
    d = problem(688, 256)
    full = lin(d["x"][:8], d["w8"])
    for i in range(8):
        assert torch.equal(full[i:i + 1], ops.skinny_linear(d["x"][i:i + 1], d["w8"]))


# ------------------------------------------------------------------ poisoned surroundings
@pytest.mark.parametrize("M", [1, 5, 16])
def test_poisoned_surroundings(M):
    """Every operand is a view into a larger buffer of NaNs (codes: 0x7F) with a row stride
    larger than its extent; the output is a view into a buffer of sentinels.  A stray read
    shows as a non-finite result, a stray write as a changed sentinel."""
    K, Nn = 264, 528
    d = problem(K, Nn)
    nan = float("nan")
    xb = torch.full((M + 2, K + 8), nan, dtype=torch.bfloat16, device=dev)
    xb[1:1 + M, :K] = d["x"][:M]
    x = xb[1:1 + M, :K]
    qb = torch.full((K + 3, Nn + 48), 0x7F, dtype=torch.uint8, device=dev)
    qb[:K, 16:16 + Nn] = d["w8"].q.view(torch.uint8)
    q = qb.view(F8)[:K, 16:16 + Nn]
    sb = torch.full((Nn + 8,), nan, dtype=torch.float32, device=dev)
    sb[4:4 + Nn] = d["w8"].scale
    bb = torch.full((Nn + 16,), nan, dtype=torch.bfloat16, device=dev)
    bb[8:8 + Nn] = d["b"]
    scale, bias = sb[4:4 + Nn], bb[8:8 + Nn]
    for s in (1, 2, K // 8 + 3):
        ob = torch.full((M + 2, Nn + 24), -7.0, dtype=torch.bfloat16, device=dev)
        out = ob[1:1 + M, 8:8 + Nn]
        _raw(x, q, scale, bias, 1, s, out=out)
        check_bound(out, d["refb"][:M], d["mag"][:M], K, f"poisoned M={M} splits={s}")
        keep = torch.ones_like(ob, dtype=torch.bool)
        keep[1:1 + M, 8:8 + Nn] = False
        assert (ob[keep] == -7.0).all(), "a store landed outside the output view"
    w8 = ops.Fp8Weight(q, scale)  # the op itself takes strided views
    assert ops.skinny_fp8_ok(x, w8, bias=bias) == routed(M)
    check_bound(lin(x, w8, bias), d["refb"][:M], d["mag"][:M], K, f"poisoned op M={M}")
    assert torch.equal(w8.dequant(), d["wd"])


# ------------------------------------------------------------------ byte offsets past 2^31
def test_offsets_past_2_31_bytes():
    """A 2.5 GiB buffer seen as codes [40, 2^26] of which only [:, :256] is written and read:
    the rows from K = 32 on lie beyond byte offset 2^31."""
    K, Nn = 40, 256
    g = torch.Generator().manual_seed(5)
    w8c = ops.quantize_weight_fp8((torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16())
    x = torch.randn(3, K, generator=g).bfloat16()
    xd, wd = x.double(), w8c.dequant().double()
    big = torch.empty(40 * 2 ** 26, dtype=torch.uint8, device=dev)
    view = w8 = None
    try:
        view = big.view(40, 2 ** 26)
        view[:, :Nn] = w8c.q.view(torch.uint8).to(dev)
        w8 = ops.Fp8Weight(view.view(F8)[:, :Nn], w8c.scale.to(dev))
        assert ops.skinny_fp8_ok(x.to(dev), w8)
        for s in (None, 2):
            got = lin(x.to(dev), w8, num_splits=s)
            check_bound(got, xd @ wd, xd.abs() @ wd.abs(), K, f"2.5 GiB splits={s}")
    finally:
        del big, view, w8
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ refusals
class fp8_flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = flags.get("skinny_fp8")
        flags.set("skinny_fp8", self.on)

    def __exit__(self, *exc):
        flags.set("skinny_fp8", self.prev)


def _small(K, Nn, M, seed):
    g = torch.Generator().manual_seed(seed)
    w8 = ops.quantize_weight_fp8((torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16())
    x = torch.randn(M, K, generator=g).bfloat16()
    xd, wd = x.double(), w8.dequant().double()
    return x.to(dev), w8.to(dev), xd @ wd, xd.abs() @ wd.abs()


def test_refusals_take_the_dequant_path():
    ok = N.lib().pa_gemm_skinny_f8_ok
    A, B, C, S = 0x10000, 0x20000, 0x30000, 0x40000
    assert ok(16, 256, 64, 64, 256, 256, 0, 1, A, B, C, None, S)
    assert not ok(17, 256, 64, 64, 256, 256, 0, 1, A, B, C, None, S)
    assert not ok(4, 264, 64, 64, 264, 264, 0, 1, A, B, C, None, S)  # N % 16
    assert not ok(4, 256, 60, 64, 256, 256, 0, 1, A, B, C, None, S)  # K % 8
    assert not ok(4, 256, 64, 64, 264, 256, 0, 1, A, B, C, None, S)  # ldb % 16
    assert not ok(4, 256, 64, 64, 256, 256, 0, 1, A, B + 8, C, None, S)  # unaligned codes
    assert not ok(4, 48, 64, 64, 48, 24, 3, 1, A, B, C, None, S)  # SwiGLU N % 32
    assert not ok(4, 256, 64, 64, 256, 256, 1, 1, A, B, C, None, S)  # bias epilogue without a bias
    assert not ok(4, 256, 1 << 25, 1 << 25, 256, 256, 0, 1, A, B, C, None, S)  # >= 4 GiB of codes
    # a refused launch returns an error code and does not launch
    d = problem(264, 528)
    out = torch.full((17, 528), -7.0, dtype=torch.bfloat16, device=dev)
    x17 = torch.zeros(17, 264, dtype=torch.bfloat16, device=dev)
    rc = N.lib().pa_gemm_skinny_f8(N.ptr(x17), N.ptr(d["w8"].q), N.ptr(d["w8"].scale), N.ptr(out), None, 0, None, 17,
                                   528, 264, 264, 528, 528, 0, 1, N.stream())
    assert rc != 0
    N.lib().pa_clear_error()
    assert (out == -7.0).all()

    with count_launches() as c:
        x, w8, ref, mag = _small(64, 24, 4, 11)  # N % 16 != 0
        assert not ops.skinny_fp8_ok(x, w8)
        check_bound(ops.skinny_linear(x, w8), ref, mag, 64, "N % 16")
        x, w8, ref, mag = _small(12, 32, 4, 12)  # K % 8 != 0
        assert not ops.skinny_fp8_ok(x, w8)
        check_bound(ops.skinny_linear(x, w8), ref, mag, 12, "K % 8")
        x, w8, ref, mag = _small(264, 528, 17, 13)
        xu = torch.empty(4 * 264 + 1, dtype=torch.bfloat16, device=dev)[1:].view(4, 264)  # 2-byte aligned only
        xu.copy_(x[:4])
        assert not ops.skinny_fp8_ok(xu, w8) and not ops.skinny_fp8_ok(x, w8)
        check_bound(ops.skinny_linear(xu, w8), ref[:4], mag[:4], 264, "unaligned x")
        check_bound(ops.skinny_linear(x, w8), ref, mag, 264, "17 rows")
        assert not ops.skinny_fp8_ok(x[:4].float(), w8)
        got = ops.skinny_linear(x[:4].float(), w8)
        assert got.dtype == torch.float32
        check_bound(got, ref[:4], mag[:4], 264, "fp32 x")
        # SwiGLU over N % 32 != 0: the 16-column interleave does not exist for such an N, so the
        # dequant path refuses it exactly as it refuses the bf16 weight
        x, w8, _, _ = _small(64, 48, 4, 14)
        assert not ops.skinny_fp8_ok(x, w8, act="swiglu_interleaved")
        with pytest.raises(RuntimeError):
            ops.skinny_linear(x, w8.dequant(), act="swiglu_interleaved")
        with pytest.raises(RuntimeError):
            ops.skinny_linear(x, w8, act="swiglu_interleaved")
        with pytest.raises(ValueError):
            lin(x, w8, act="swiglu_interleaved")
        # the flag
        d = problem(264, 528)
        x = d["x"][:4]
        with fp8_flag(False):
            assert not ops.skinny_fp8_ok(x, d["w8"])
            got = ops.skinny_linear(x, d["w8"], d["b"])
        assert torch.equal(got, ops.skinny_linear(x, d["wd"], d["b"]))
        check_bound(got, d["refb"][:4], d["mag"][:4], 264, "FLAGS_skinny_fp8=0")
    assert c.n == 0
    assert ops.skinny_fp8_ok(x, d["w8"])


# ------------------------------------------------------------------ models
_sets = {}


def model_set(kind, head=False):
    """(quantised bf16 model, bf16 twin and fp32 twin holding the dequantised weights), on the
    GPU, from one seed; shared, unchanged."""
    key = (kind, head)
    if key not in _sets:
        twin = make_model(kind, dev, "bfloat16")
        names = twin._quant_weights + (("lm_head",) if head else ())
        sd = twin.state_dict()
        for k in list(sd):
            if k.split(".")[-1] in names:
                sd[k] = ops.quantize_weight_fp8(sd[k]).dequant()
        twin.load_state_dict(sd)
        ref = make_model(kind, dev, "float32")
        ref.load_state_dict({k: v.float() for k, v in sd.items()})
        quant = make_model(kind, dev, "bfloat16").quantize_weights(include_head=head)
        _sets[key] = (quant, twin, ref)
    return _sets[key]


def _teacher_forced(model, ids, P, paged=False):
    """Prefill P tokens, then feed the rest one at a time: the logits of positions P-1 .. S-2 and
    the (fp8, bf16 skinny) launches of the prefill and of each decode step."""
    B, S = ids.shape
    cache = model.init_cache(B, S, paged=paged)
    with count_launches() as c8, count_launches(skinny) as c16:
        got = [model.prefill(ids[:, :P], cache)]
    n_prefill, n_steps = (c8.n, c16.n), []
    for t in range(P, S):
        with count_launches() as c8, count_launches(skinny) as c16:
            got.append(model.decode_step(ids[:, t], cache))
        n_steps.append((c8.n, c16.n))
    return torch.stack(got[:-1], 1).float(), n_prefill, n_steps


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("kind,head", [(k, False) for k in MODELS] + [("llama", True)])
def test_quantised_models(kind, head, B):
    """E_decode <= 2 * E_full against an fp32 model holding the dequantised weights, where
    E_full is a bf16 model holding them on the unquantised path; per decode step 4 fp8 launches
    per layer (+ the head with include_head) and no bf16 skinny launch but the unquantised
    head's; no fp8 launch in the prefill's layers; run-to-run bits; paged == contiguous."""
    quant, twin, ref = model_set(kind, head)
    torch.manual_seed(3)
    S, P = 24, 8
    ids = torch.randint(1, quant.cfg.vocab_size, (B, S), device=dev)
    with torch.no_grad():
        want = ref(ids)[:, P - 1:S - 1].float()
        full = twin(ids)[:, P - 1:S - 1].float()
        assert torch.equal(quant(ids), twin(ids)), "the inference forward runs on the exact dequantised image"
    dec, n_prefill, n_steps = _teacher_forced(quant, ids, P)
    e_full, e_dec = _rel(full, want), _rel(dec, want)
    print(f"quantised {kind} head={head} B={B}: E_full {e_full:.3e}  E_decode {e_dec:.3e}  launches (fp8, bf16) "
          f"prefill {n_prefill} step {n_steps[0]}")
    assert torch.isfinite(dec).all()
    assert e_dec <= 2 * e_full
    layers = quant.cfg.num_hidden_layers
    assert n_prefill == ((1, 0) if head else (0, 1))  # the last-row logits only
    assert n_steps == [(4 * layers + 1, 0) if head else (4 * layers, 1)] * (S - P)
    # run-to-run bits, generate twice, paged against contiguous
    assert torch.equal(_teacher_forced(quant, ids, P)[0], dec)
    a, _ = quant.generate(ids[:, :6], 8)
    assert torch.equal(a, quant.generate(ids[:, :6], 8)[0])
    assert torch.equal(a, quant.generate(ids[:, :6], 8, cache="paged")[0])
