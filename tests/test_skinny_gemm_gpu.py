"""The skinny-M GEMM kernels (csrc/kernels/gemm_skinny.hip) against an fp64 CPU reference
computed from the same bf16 inputs.

Plain product / bias bound, per element:

    |got - ref| <= 2^-8 |ref| + K * 2^-22 * (|x| @ |w|)

one bf16 rounding (2^-9 relative) with a factor 2, plus the first-order bound of an fp32
sum of K terms in any order (K * 2^-24 * sum |terms|) with a factor 2 and the product
roundings.  Partials kept in bf16 would break it from K ~ 700 on.

GELU / SwiGLU epilogues: the norm-ratio error must be at most twice that of the path they
replace on the same inputs (which rounds to bf16 before the activation)."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import _native as N
from paddle_amd.ops import skinny

pytestmark = pytest.mark.gpu

dev = "cuda"
ALL_M = list(range(1, 17))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


_data = {}


def problem(K, Nn, kmaj=False):
    """16 rows of x, a weight and a bias for (K, N), with the fp64 products; shared, unchanged."""
    key = (K, Nn, kmaj)
    if key not in _data:
        g = torch.Generator().manual_seed(1000 * K + Nn + int(kmaj))
        x = torch.randn(16, K, generator=g).bfloat16()
        w = (torch.randn(K, Nn, generator=g) * K ** -0.5).bfloat16()
        b = torch.randn(Nn, generator=g).bfloat16()
        xd, wd = x.double(), w.double()
        ref = xd @ wd
        mag = xd.abs() @ wd.abs()
        wg = (w.t().contiguous() if kmaj else w).to(dev)
        _data[key] = dict(x=x.to(dev), w=wg, b=b.to(dev), ref=ref, refb=ref + b.double(), mag=mag, K=K, N=Nn)
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
    """fp64 silu(gate) * up over the interleaved layout."""
    g, u = ops.deinterleave_gate_up(ref)
    return g * torch.sigmoid(g) * u


def swiglu_parent(x, w):
    gu = ops.linear(x, w)
    g, u = ops.deinterleave_gate_up(gu)
    return (torch.nn.functional.silu(g.float()) * u.float()).to(x.dtype)


def gelu_ref(z):
    return torch.nn.functional.gelu(z, approximate="tanh")


def lin(x, w, bias=None, act=None, num_splits=None):
    """The MN-major kernel for every M it covers (the ops route only part of them to it)."""
    return skinny.skinny_kernel(x, w, bias=bias, act=act, num_splits=num_splits)


def lin_t(x, w, num_splits=None):
    return skinny.skinny_kernel(x, w, b_kmaj=True, num_splits=num_splits)


def routed(M, Nn, act=None):
    return M <= 8 and (M == 1 or Nn < 8192 or act == "swiglu_interleaved")


class count_launches:
    def __enter__(self):
        self.n = 0
        self._orig = skinny._launch

        def wrapped(*a, **k):
            self.n += 1
            return self._orig(*a, **k)

        skinny._launch = wrapped
        return self

    def __exit__(self, *exc):
        skinny._launch = self._orig


# ------------------------------------------------------------------ accuracy, every M
@pytest.mark.parametrize("K,Nn", [(8, 8), (256, 768), (688, 256), (264, 520)])
def test_mn_major_plain_and_bias(K, Nn):
    d = problem(K, Nn)
    with count_launches() as c:
        for M in ALL_M:
            x = d["x"][:M]
            assert ops.skinny_ok(x, d["w"]) == routed(M, Nn) == ops.skinny_ok(x, d["w"], bias=d["b"])
            got = lin(x, d["w"])
            if routed(M, Nn):  # the public op runs the same kernel
                assert torch.equal(ops.skinny_linear(x, d["w"]), got)
            assert got.shape == (M, Nn) and got.dtype == torch.bfloat16
            check_bound(got, d["ref"][:M], d["mag"][:M], K, f"mn {K}x{Nn} M={M}")
            got = lin(x, d["w"], d["b"])
            check_bound(got, d["refb"][:M], d["mag"][:M], K, f"mn+bias {K}x{Nn} M={M}")
    assert c.n == 2 * len(ALL_M) + 8
    # fp32 bias, and x with leading dimensions
    got = lin(d["x"][:6].view(3, 2, K), d["w"], d["b"].float())
    assert got.shape == (3, 2, Nn)
    check_bound(got.view(6, Nn), d["refb"][:6], d["mag"][:6], K, f"mn+fp32 bias {K}x{Nn}")


def test_mn_major_swiglu_every_m():
    K, Nn = 256, 1376  # llama-tiny gate|up: N is no multiple of the 128-column tile
    d = problem(K, Nn)
    want = swiglu_ref(d["ref"])
    for M in ALL_M:
        x = d["x"][:M]
        with count_launches() as c:
            got = lin(x, d["w"], act="swiglu_interleaved")
        assert c.n == 1 and got.shape == (M, Nn // 2)
        e_new, e_old = _rel(got, want[:M]), _rel(swiglu_parent(x, d["w"]), want[:M])
        print(f"swiglu M={M}: skinny {e_new:.3e}  parent {e_old:.3e}")
        assert torch.isfinite(got).all() and e_new <= 2 * e_old


def test_mn_major_bias_gelu_every_m():
    K, Nn = 256, 1024
    d = problem(K, Nn)
    want = gelu_ref(d["refb"])
    for M in ALL_M:
        x = d["x"][:M]
        with count_launches() as c:
            got = lin(x, d["w"], d["b"], act="gelu_tanh")
        assert c.n == 1 and got.shape == (M, Nn)
        e_new, e_old = _rel(got, want[:M]), _rel(ops.linear_gelu(x, d["w"], d["b"]), want[:M])
        print(f"gelu M={M}: skinny {e_new:.3e}  parent {e_old:.3e}")
        assert torch.isfinite(got).all() and e_new <= 2 * e_old


@pytest.mark.parametrize("K,Nn", [(8, 1), (256, 512), (264, 1001)])
def test_k_major(K, Nn):
    d = problem(K, Nn, kmaj=True)
    for M in (1, 3, 8, 16):
        x = d["x"][:M]
        assert ops.skinny_ok(x, d["w"], b_kmaj=True) == routed(M, Nn)
        with count_launches() as c:
            got = lin_t(x, d["w"])
        if routed(M, Nn):
            assert torch.equal(ops.skinny_linear_t(x, d["w"]), got)
        assert c.n == 1 and got.shape == (M, Nn)
        check_bound(got, d["ref"][:M], d["mag"][:M], K, f"kmaj {K}x{Nn} M={M}")


# ------------------------------------------------------------------ forced split counts
@pytest.mark.parametrize("kmaj,K,Nn,M", [(False, 688, 256, 5), (False, 264, 520, 16), (True, 264, 1001, 3),
                                          (True, 256, 512, 16)])
def test_forced_num_splits(kmaj, K, Nn, M):
    d = problem(K, Nn, kmaj)
    x = d["x"][:M]
    f = (lambda s: lin_t(x, d["w"], num_splits=s)) if kmaj else \
        (lambda s: lin(x, d["w"], d["b"], num_splits=s))
    ref = d["ref"] if kmaj else d["refb"]
    for s in (1, 2, 5, K // 8 + 3):  # the last one has empty slices
        with count_launches() as c:
            got = f(s)
        assert c.n == 1
        check_bound(got, ref[:M], d["mag"][:M], K, f"splits={s} kmaj={kmaj} {K}x{Nn} M={M}")
        assert torch.equal(f(s), got), f"splits={s}: two runs differ"


def test_forced_num_splits_activations():
    d = problem(256, 1376)
    x = d["x"][:5]
    want = swiglu_ref(d["ref"])[:5]
    e_old = _rel(swiglu_parent(x, d["w"]), want)
    for s in (1, 2, 5, 256 // 8 + 3):
        got = lin(x, d["w"], act="swiglu_interleaved", num_splits=s)
        e_new = _rel(got, want)
        print(f"swiglu splits={s}: skinny {e_new:.3e}  parent {e_old:.3e}")
        assert e_new <= 2 * e_old
        assert torch.equal(lin(x, d["w"], act="swiglu_interleaved", num_splits=s), got)
    d = problem(256, 1024)
    x = d["x"][:5]
    want = gelu_ref(d["refb"])[:5]
    e_old = _rel(ops.linear_gelu(x, d["w"], d["b"]), want)
    for s in (1, 2, 5, 256 // 8 + 3):
        got = lin(x, d["w"], d["b"], act="gelu_tanh", num_splits=s)
        e_new = _rel(got, want)
        print(f"gelu splits={s}: skinny {e_new:.3e}  parent {e_old:.3e}")
        assert e_new <= 2 * e_old
        assert torch.equal(lin(x, d["w"], d["b"], act="gelu_tanh", num_splits=s), got)


# ------------------------------------------------------------------ batch invariance
def _raw(kmaj, x, w, bias, epi, splits, out=None):
    """One kernel call through skinny._launch (epilogues the public K-major op does not expose)."""
    M, K = x.shape
    Nn = w.shape[0] if kmaj else w.shape[1]
    nout = Nn // 2 if epi == 3 else Nn
    if out is None:
        out = torch.empty(M, nout, dtype=torch.bfloat16, device=dev)
    nws = int(N.lib().pa_gemm_skinny_ws_floats(M, Nn, splits))
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dev)
    return skinny._launch(kmaj, x, w, out, bias, ws, M, Nn, K, epi, splits)


@pytest.mark.parametrize("M", [3, 8, 16])
def test_batch_invariance(M):
    cases = []
    for K, Nn in [(688, 256), (264, 520)]:
        d = problem(K, Nn)
        for s in (1, 2, 5):
            cases += [(False, d, None, 0, s), (False, d, d["b"], 2, s)]
    d = problem(256, 1376)
    cases += [(False, d, None, 3, 1), (False, d, None, 3, 3)]
    d = problem(264, 1001, kmaj=True)
    cases += [(True, d, None, 0, 1), (True, d, None, 0, 3), (True, d, d["b"], 1, 1), (True, d, d["b"], 2, 3)]
    for kmaj, d, bias, epi, s in cases:
        x = d["x"][:M]
        full = _raw(kmaj, x, d["w"], bias, epi, s)
        for i in range(M):
            one = _raw(kmaj, x[i:i + 1], d["w"], bias, epi, s)
            assert torch.equal(full[i:i + 1], one), f"row {i} of M={M} kmaj={kmaj} epi={epi} splits={s}"
    # and through the public ops at their default split counts
    d = problem(688, 256)
    full = lin(d["x"][:M], d["w"])
    for i in range(M):
        assert torch.equal(full[i:i + 1], lin(d["x"][i:i + 1], d["w"]))
    d = problem(264, 1001, kmaj=True)
    full = lin_t(d["x"][:M], d["w"])
    for i in range(M):
        assert torch.equal(full[i:i + 1], lin_t(d["x"][i:i + 1], d["w"]))


# ------------------------------------------------------------------ poisoned surroundings
@pytest.mark.parametrize("kmaj", [False, True])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_poisoned_surroundings(kmaj, M):
    """Views into larger buffers whose every other element is inf; the output is a view into
    a buffer of sentinels.  A stray read shows as a non-finite result, a stray write as a
    changed sentinel."""
    K, Nn = (264, 1001) if kmaj else (264, 520)
    d = problem(K, Nn, kmaj)
    inf = float("inf")
    xb = torch.full((M + 2, K + 8), inf, dtype=torch.bfloat16, device=dev)
    xb[1:1 + M, :K] = d["x"][:M]
    x = xb[1:1 + M, :K]
    rows, cols = d["w"].shape
    wb = torch.full((rows + 3, cols + 24), inf, dtype=torch.bfloat16, device=dev)
    wb[:rows, :cols] = d["w"]
    w = wb[:rows, :cols]
    pad = 16 if not kmaj else 7
    for s in (1, 2, K // 8 + 3):
        ob = torch.full((M + 2, Nn + pad + 8), -7.0, dtype=torch.bfloat16, device=dev)
        out = ob[1:1 + M, 8:8 + Nn]
        _raw(kmaj, x, w, None, 0, s, out=out)
        check_bound(out, d["ref"][:M], d["mag"][:M], K, f"poisoned kmaj={kmaj} M={M} splits={s}")
        keep = torch.ones_like(ob, dtype=torch.bool)
        keep[1:1 + M, 8:8 + Nn] = False
        assert (ob[keep] == -7.0).all(), "a store landed outside the output view"
    if not kmaj:  # the op itself takes strided views of x and w
        assert ops.skinny_ok(x, w) == routed(M, Nn)
        check_bound(lin(x, w), d["ref"][:M], d["mag"][:M], K, f"poisoned op M={M}")


# ------------------------------------------------------------------ byte offsets past 2^31
def test_offsets_past_2_31_bytes():
    """One 2.15 GB buffer seen as an MN-major weight [8200, 131080] and as a K-major one
    [131080, 8200]: the last 64 outputs read bytes beyond offset 2^31."""
    big = torch.empty(8200 * 131080, dtype=torch.bfloat16, device=dev)
    big.normal_(generator=torch.Generator(device=dev).manual_seed(5))
    big.mul_(8200 ** -0.5)
    x = torch.randn(2, 8200, generator=torch.Generator().manual_seed(6)).bfloat16().to(dev)
    xd = x.double().cpu()
    try:
        w = big.view(8200, 131080)
        assert not ops.skinny_ok(x, w) and ops.skinny_ok(x[:1], w)  # wide N: routed at one row
        ws = w[:, -64:].double().cpu()
        for s in (None, 2):
            got = lin(x, w, num_splits=s)
            assert got.shape == (2, 131080)
            check_bound(got[:, -64:], xd @ ws, xd.abs() @ ws.abs(), 8200, f"mn-major 2.15 GB splits={s}")
        wt = big.view(131080, 8200)
        assert not ops.skinny_ok(x, wt, b_kmaj=True) and ops.skinny_ok(x[:1], wt, b_kmaj=True)
        ws = wt[-64:].double().cpu().t()
        for s in (None, 2):
            got = lin_t(x, wt, num_splits=s)
            assert got.shape == (2, 131080)
            check_bound(got[:, -64:], xd @ ws, xd.abs() @ ws.abs(), 8200, f"k-major 2.15 GB splits={s}")
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ refusals
def test_refusals_fall_back_to_the_parent_path():
    ok = N.lib().pa_gemm_skinny_ok
    A, B, C = 0x10000, 0x20000, 0x30000
    assert ok(0, 16, 256, 64, 64, 256, 256, 0, 1, A, B, C, None)
    assert not ok(0, 17, 256, 64, 64, 256, 256, 0, 1, A, B, C, None)
    assert not ok(0, 4, 256, 64, 64, 256, 256, 0, 1, A + 2, B, C, None)  # unaligned base
    assert not ok(0, 4, 131080, 16384, 16384, 131080, 131080, 0, 1, A, B, C, None)  # >= 4 GiB
    assert not ok(1, 4, 262144, 8192, 8192, 8192, 262144, 0, 1, A, B, C, None)
    # a refused launch returns an error code and does not launch
    d = problem(264, 520)
    out = torch.full((17, 520), -7.0, dtype=torch.bfloat16, device=dev)
    rc = N.lib().pa_gemm_skinny(0, N.ptr(d["x"]), N.ptr(d["w"]), N.ptr(out), None, 0, None, 17, 520, 264, 264, 520,
                                520, 0, 1, N.stream())
    assert rc != 0
    N.lib().pa_clear_error()
    assert (out == -7.0).all()
    # the ops fall back and still return the right answer
    g = torch.Generator().manual_seed(9)
    x17 = torch.randn(17, 264, generator=g).bfloat16()
    ref = x17.double() @ d["w"].double().cpu()
    mag = x17.double().abs() @ d["w"].double().cpu().abs()
    xu = torch.empty(4 * 264 + 1, dtype=torch.bfloat16, device=dev)[1:].view(4, 264)  # 2-byte aligned only
    xu.copy_(x17[:4])
    with count_launches() as c:
        assert not ops.skinny_ok(x17.to(dev), d["w"]) and not ops.skinny_ok(xu, d["w"])
        check_bound(ops.skinny_linear(x17.to(dev), d["w"]), ref, mag, 264, "17 rows")
        check_bound(ops.skinny_linear(xu, d["w"]), ref[:4], mag[:4], 264, "unaligned x")
        x12 = x17[:12].to(dev)  # covered by the kernel, not routed to it
        check_bound(ops.skinny_linear(x12, d["w"]), ref[:12], mag[:12], 264, "12 rows")
        assert not ops.skinny_ok(d["x"][:4].float(), d["w"].float())
    assert c.n == 0
