"""The row kernels (norm.hip, softmax_ce.hip, the rotary / SwiGLU / embedding kernels of
elementwise.hip) against the per-row float64 oracle (tests/row_oracle.py), through the
public ops, in bf16 and fp32, at the smallest shapes that reach every dispatch edge.

Every device input is a view into a NaN-filled parent, and every tensor the op allocates
while it runs (outputs, saved statistics, workspaces) is a view into a sentinel-filled
parent (``sentinels``): a stray read shows as a non-finite result, a stray store as a
changed sentinel, an element never written as the sentinel itself.  Each case runs twice
and everything but dw / db (LDS float atomics) must come out with the same bits.  The
module prints the worst statistic per kernel and dtype when it finishes (the table kept in
row_oracle's docstring; run with -s to see it)."""
import contextlib
import math

import pytest
import torch

import row_oracle as R
from paddle_amd.ops import _native
from paddle_amd.ops import fused as F

pytestmark = pytest.mark.gpu

dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
PAD = 1024       # border elements on each side (a multiple of 16 bytes for every dtype)
SENT = -7777.0
WORST = {}


def _dn(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nworst statistic per kernel and dtype")
    for k in sorted(WORST):
        print("    %-28s %-5s " % k + "  ".join(f"{n} {s:.2e}" for n, s in sorted(WORST[k].items())))


def _record(kernel, dtype, stats, bounds, what, fails):
    w = WORST.setdefault((kernel, _dn(dtype)), {})
    for n, s in stats.items():
        w[n] = max(w.get(n, 0.0), s)
        if not s <= bounds[n]:
            fails.append((kernel, _dn(dtype), what, n, s, bounds[n]))


def _finish(fails):
    assert not fails, (len(fails), fails[:6])


# ------------------------------------------------------------------ poisoned surroundings
def bordered(t, fill=float("nan")):
    """CPU tensor -> contiguous device view with PAD elements of ``fill`` before and after it."""
    if t is None:
        return None
    n = t.numel()
    parent = torch.full((n + 2 * PAD,), fill, dtype=t.dtype, device=dev)
    v = parent[PAD:PAD + n].view(t.shape)
    v.copy_(t)
    return v


class _Alloc:
    """Hands out views into sentinel-filled parents and checks the borders afterwards."""

    def __init__(self):
        self.blocks, self.views, self.native = [], [], []

    def view_at(self, pointer):
        """The view handed out at this device address (a ctypes pointer of a native call)."""
        (v,) = [v for v in self.views if v.data_ptr() == pointer.value]
        return v

    def alloc(self, shape, dtype, device):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape)
        parent = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=device)
        v = parent[PAD:PAD + n].view(shape)
        self.blocks.append((parent, n))
        self.views.append(v)
        return v

    def intact(self):
        for parent, n in self.blocks:
            s = torch.full((), SENT, dtype=parent.dtype, device=parent.device)
            if not ((parent[:PAD] == s).all() and (parent[PAD + n:] == s).all()):
                return False
        return True


class _TorchProxy:
    """``torch`` as paddle_amd.ops.fused sees it while a case runs: device allocations come
    from an _Alloc, everything else is torch's."""

    def __init__(self, a):
        self._a = a

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _shape(size):
        return tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size

    def empty(self, *size, dtype=None, device=None, **kw):
        if device is None or torch.device(device).type != "cuda":
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._a.alloc(self._shape(size), dtype or torch.float32, device)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if device is None or torch.device(device).type != "cuda":
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._a.alloc(self._shape(size), dtype or torch.float32, device).zero_()

    def empty_like(self, t, dtype=None, **kw):
        if not t.is_cuda:
            return torch.empty_like(t, dtype=dtype, **kw)
        return self._a.alloc(t.shape, dtype or t.dtype, t.device)


@contextlib.contextmanager
def sentinels():
    """Inside: every device tensor fused.py allocates is sentinel-bordered, and the native
    calls are recorded.  Yields (allocator, calls)."""
    a, calls, orig = _Alloc(), [], _native.call

    def spy(name, *args):
        calls.append(name)
        a.native.append((name, args))
        return orig(name, *args)

    F.torch = _TorchProxy(a)
    _native.call = spy
    try:
        yield a, calls
        torch.cuda.synchronize()
    finally:
        F.torch = torch
        _native.call = orig


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _det(t):
    return None if t is None else t.detach()


# ====================================================================== norm
def run_norm(inp, rms, use_dh, expect_kernel=True):
    t = {k: bordered(v) for k, v in inp.items()}
    x, w = t["x"].requires_grad_(), t["w"].requires_grad_()
    res = t["res"].requires_grad_() if t["res"] is not None else None
    b = t["b"].requires_grad_() if t["b"] is not None else None
    with sentinels() as (a, calls):
        if rms:
            out = F.rms_norm(x, w, R.norm_eps(rms), residual=res)
        else:
            out = F.layer_norm(x, w, b, R.norm_eps(rms), residual=res)
        y, h = out if res is not None else (out, None)
        if use_dh:
            torch.autograd.backward([y, h], [t["dy"], t["dh"]])
        else:
            y.backward(t["dy"])
    assert a.intact(), "stray store"
    ran = [c for c in calls if c.startswith("pa_norm")]
    assert ran == (["pa_norm_fwd", "pa_norm_bwd"] if expect_kernel else []), calls
    return dict(y=_det(y), h=_det(h), dx=x.grad, dres=None if res is None else res.grad, dw=w.grad,
                db=None if b is None else b.grad)


def _norm_case(kernel, dtype, inp, rms, use_dh, what, fails, expect_kernel=True, bound_dtype=None):
    N = inp["x"].shape[0]
    ref, mag = R.norm_case_reference(inp, rms, use_dh)
    got = run_norm(inp, rms, use_dh, expect_kernel)
    again = run_norm(inp, rms, use_dh, expect_kernel)
    for n in ("y", "h", "dx", "dres"):
        assert _same_bits(got[n], again[n]), (what, n, "differs between two runs")
    _record(kernel, dtype, R.norm_stats(got, ref, mag), R.norm_bounds(bound_dtype or dtype, N), what, fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("H", R.NORM_H)
def test_norm(H, dtype):
    """Every MAXV dispatch edge (H / 512 vectors per lane: 1, 2, 4, 8, 16), both two-waves-
    per-row backward variants (2048 < H <= 4096 and H > 4096) and a partly populated lane
    (H % 512 == 8), with 1, 5 and 67 rows (67: five blocks, partial last iterations)."""
    fails = []
    for N, prof, rms, with_res, use_dh, with_bias in R.norm_cases(H):
        inp = R.norm_inputs(prof, N, H, dtype, with_res, with_bias)
        _norm_case("rms_norm" if rms else "layer_norm", dtype, inp, rms, use_dh,
                   (H, N, prof, with_res, use_dh, with_bias), fails)
    _finish(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("N,H", R.NORM_BIG)
def test_norm_many_rows(N, H, dtype):
    """N = 8193: the backward's block cap binds (482 blocks of 17 rows, the fifth iteration
    of a block holds one row)."""
    fails = []
    for rms in (True, False):
        inp = R.norm_inputs("flat", N, H, dtype, True, not rms)
        _norm_case("rms_norm" if rms else "layer_norm", dtype, inp, rms, True, (H, N, rms), fails)
    _finish(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_layer_norm_stats(dtype):
    """layer_norm_stats / layer_norm_stats_grad (the fluid layer_norm op's path): y, the saved
    mean and rstd, and the backward from them."""
    fails, N, H = [], 67, 1032
    for prof in R.NORM_PROFILES:
        inp = R.norm_inputs(prof, N, H, dtype, False, True)
        ref, mag = R.norm_case_reference(inp, False, False)
        t = {k: bordered(v) for k, v in inp.items()}
        runs = []
        for _ in range(2):
            with sentinels() as (a, calls):
                y, mean, rstd = F.layer_norm_stats(t["x"], t["w"], t["b"], 1e-5)
                dx, dw, db = F.layer_norm_stats_grad(t["dy"], t["x"], t["w"], mean, rstd, True)
            assert a.intact() and calls == ["pa_norm_fwd", "pa_norm_bwd"], calls
            runs.append(dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db))
        for n in ("y", "mean", "rstd", "dx"):
            assert _same_bits(runs[0][n], runs[1][n]), (prof, n)
        _record("layer_norm_stats", dtype, R.norm_stats(runs[0], ref, mag), R.norm_bounds(dtype, N), prof, fails)
    _finish(fails)


@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
@pytest.mark.parametrize("case", ["H1004", "H8200", "fp32_weight"])
def test_norm_routing(case, rms):
    """What the kernel cannot take runs the reference path: no norm kernel is launched, the
    answer is the oracle's within the same bounds."""
    fails = []
    for dtype in DTYPES:
        H = {"H1004": 1004, "H8200": 8200, "fp32_weight": 1024}[case]
        if case == "fp32_weight" and dtype == torch.float32:
            continue
        inp = R.norm_inputs("flat", 5, H, dtype, True, not rms)
        if case == "fp32_weight":
            inp["w"] = inp["w"].float()
            if inp["b"] is not None:
                inp["b"] = inp["b"].float()
        _norm_case("norm, reference path", dtype, inp, rms, True, (case, rms), fails, expect_kernel=False)
    _finish(fails)


def test_norm_launchers_refuse_partial_vectors():
    """pa_norm_fwd / pa_norm_bwd return an error for H % 8 != 0 before any launch."""
    N, H = 2, 1004
    buf = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
    x, y, w, st, ws = buf(N * 1008), buf(N * 1008), buf(1008), buf(N), buf(2 * 1008)
    with pytest.raises(_native.EnforceError):
        _native.call("pa_norm_fwd", 0, 1, _native.ptr(x), None, _native.ptr(w), None, _native.ptr(y), None, None,
                     _native.ptr(st), N, H, 1e-6, _native.stream())
    with pytest.raises(_native.EnforceError):
        _native.call("pa_norm_bwd", 0, 1, _native.ptr(x), _native.ptr(x), _native.ptr(w), None, _native.ptr(st), None,
                     _native.ptr(y), _native.ptr(w), None, _native.ptr(ws), N, H, _native.stream())
    torch.cuda.synchronize()
    assert not y.any()


# ====================================================================== softmax cross-entropy
def run_ce(x_cpu, lab, up, reduction, inplace):
    x = bordered(x_cpu).requires_grad_()
    labd = lab.to(dev)
    with sentinels() as (a, calls):
        out = F.softmax_cross_entropy(x, labd, -100, reduction, inplace_grad=inplace)
        # the lse the forward kernel was given: argument 5 of pa_softmax_ce_fwd(dtype, logits,
        # label, soft, loss, lse, ...)
        (fwd_args,) = [args for name, args in a.native if name == "pa_softmax_ce_fwd"]
        lse = a.view_at(fwd_args[5])
        assert lse.shape == (x.shape[0],) and lse.dtype == torch.float32
        assert lse.data_ptr() != a.view_at(fwd_args[4]).data_ptr()
        got = {("loss" if reduction == "none" else reduction): (out.sum() if reduction == "sum" else out).detach().clone()}
        if reduction == "none":
            out.backward(up.to(dev))
        elif reduction == "sum":
            out.backward(torch.tensor(float(up), device=dev))
        else:
            out.backward(torch.tensor(float(up), device=dev))
        torch.cuda.synchronize()
        got.update(lse=lse.clone(), dlogits=x.grad.clone())
    assert a.intact(), "stray store"
    assert [c for c in calls if "softmax_ce" in c] == ["pa_softmax_ce_fwd", "pa_softmax_ce_bwd"], calls
    return got


def _ce_case(dtype, x, lab, reduction, what, fails):
    N = x.shape[0]
    up = torch.linspace(-2, 2, N) if reduction == "none" else 1.7
    ref, mag = R.ce_reference(x, lab, up, -100, reduction)
    got = run_ce(x, lab, up, reduction, False)
    again = run_ce(x, lab, up, reduction, False)
    inpl = run_ce(x, lab, up, reduction, True)
    for n in got:
        assert _same_bits(got[n], again[n]), (what, n, "differs between two runs")
        assert _same_bits(got[n], inpl[n]), (what, n, "inplace_grad differs")
    dead = ~((lab != -100) & (lab >= 0) & (lab < x.shape[1]))
    assert not got["dlogits"][dead.to(dev)].any(), (what, "gradient on a row without a valid label")
    if reduction == "none":
        assert not got["loss"][dead.to(dev)].any(), (what, "loss on a row without a valid label")
    chk = R.ce_check(got, ref, mag, dtype)
    _record("softmax_cross_entropy", dtype, {n: s for n, (s, b) in chk.items()}, {n: b for n, (s, b) in chk.items()},
            what, fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("V", R.SOFTMAX_V)
def test_softmax_cross_entropy(V, dtype):
    """Scalar (V % 8 != 0) and vector path, one and two passes of the 256 x 8 stride, threads
    with no element; every logit profile (the masked ones are the -inf chunks that used to
    give NaN), every kind of label, the three reductions, inplace_grad."""
    fails = []
    for N in R.SOFTMAX_N:
        for prof in R.LOGIT_PROFILES:
            x, hot = R.logit_inputs(prof, N, V, dtype)
            lab = R.make_labels(x, hot)
            for red in ("mean", "none", "sum"):
                _ce_case(dtype, x, lab, red, (V, N, prof, red), fails)
    x, hot = R.logit_inputs("flat", 3, V, dtype)
    for red in ("mean", "none"):
        _ce_case(dtype, x, torch.full((3,), -100), red, (V, "all ignored", red), fails)
    _ce_case(dtype, x, R.make_labels(x, hot, kinds=("first", "last", "random")), "mean", (V, "all valid"), fails)
    _finish(fails)


# ====================================================================== softmax / log-softmax
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("V", R.SOFTMAX_V)
def test_softmax(V, dtype):
    fails = []
    for N in R.SOFTMAX_N:
        for prof in ("flat",) + R.MASKED_PROFILES:
            x_cpu, _ = R.logit_inputs(prof, N, V, dtype)
            dy_cpu = torch.randn(N, V, generator=torch.Generator().manual_seed(V + N)).to(dtype)
            for log in (False, True):
                ref, mag = R.softmax_reference(x_cpu, dy_cpu, log)
                runs = []
                for _ in range(2):
                    x, dy = bordered(x_cpu).requires_grad_(), bordered(dy_cpu)
                    with sentinels() as (a, calls):
                        y = F.softmax(x, -1, log=log)
                        y.backward(dy)
                    assert a.intact() and calls == ["pa_softmax_fwd", "pa_softmax_bwd"], calls
                    runs.append(dict(y=y.detach(), dx=x.grad))
                for n in ("y", "dx"):
                    assert _same_bits(runs[0][n], runs[1][n]), (V, N, prof, log, n)
                st = {n: R.masked_row_stat(runs[0][n], ref[n], mag[n]) for n in ("y", "dx")}
                _record("log_softmax" if log else "softmax", dtype, st, {n: R.exp_bound(dtype) for n in st},
                        (V, N, prof), fails)
    _finish(fails)


# ====================================================================== embedding
def _int_dout(n_tok, H, seed=0):
    return torch.randint(-8, 9, (n_tok, H), generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def _run_embedding(W_cpu, ids, dout_cpu, pad):
    W = bordered(W_cpu).requires_grad_()
    with sentinels() as (a, calls):
        out = F.embedding(ids.to(dev), W, None if pad < 0 else pad)
        out.backward(bordered(dout_cpu))
    assert a.intact(), "stray store"
    assert [c for c in calls if "embedding" in c] == ["pa_embedding_fwd", "pa_embedding_bwd"], calls
    return out.detach(), W.grad


def _run_embedding_main_grad(W_cpu, ids, dout_cpu, pad, prefill):
    """Backward straight into an fp32 main_grad: zeroed first (``prefill`` None: the first
    write after zero_grad, over stale contents) or accumulated onto ``prefill``."""
    W = bordered(W_cpu).requires_grad_()
    mg = bordered(torch.full(W_cpu.shape, 555.0) if prefill is None else prefill, fill=SENT)
    W._pa_main_grad, W._pa_grad_fresh = mg, prefill is None
    with sentinels() as (a, calls):
        out = F.embedding(ids.to(dev), W, None if pad < 0 else pad)
        out.backward(bordered(dout_cpu))
    assert a.intact() and W.grad is None
    parent = mg._base
    s = torch.full((), SENT, device=dev)
    assert (parent[:PAD] == s).all() and (parent[PAD + mg.numel():] == s).all(), "stray store round main_grad"
    return mg


@pytest.mark.parametrize("n_tok,H", R.EMB_CASES)
def test_embedding(n_tok, H):
    """Gather and the deterministic scatter backward: ranges of 8192 rows, 64-row id scans,
    groups of 16 rows in flight, two column passes at H = 4104.  With small-integer dout the
    fp32 accumulator must hold the exact integer sums: into the zeroed dW the backward
    allocates (fp32 table), into a zeroed main_grad and on top of a pre-filled one (bf16
    dout); with random dout the rounded dW meets the bound with the same bits twice."""
    fails = []
    vocab = n_tok + 8
    g = torch.Generator().manual_seed(n_tok + H)
    for dtype in DTYPES:
        W = torch.randn(vocab, H, generator=g).to(dtype)
        dout = torch.randn(n_tok, H, generator=g).to(dtype)
        for name, ids in R.id_patterns(n_tok, vocab).items():
            pad = 2 if name == "padding" else -1
            ref, mag = R.embedding_reference(ids, W, dout, pad)
            out, dW = _run_embedding(W, ids, dout, pad)
            out2, dW2 = _run_embedding(W, ids, dout, pad)
            assert torch.equal(out.cpu().double(), ref["out"]), (n_tok, H, name, "gather")
            assert _same_bits(out, out2) and _same_bits(dW, dW2), (n_tok, H, name, "differs between two runs")
            nmax = int(torch.bincount(ids).max())
            _record("embedding", dtype, {"dW": R.row_stat(dW, ref["dW"], mag["dW"])}, {"dW": R.acc_bound(dtype, nmax)},
                    (n_tok, H, name), fails)
            if dtype == torch.float32:
                # the ordinary path (a zeroed fp32 dW allocated by the backward, no cast): exact
                di = _int_dout(n_tok, H).float()
                want = R.embedding_reference(ids, W, di, pad)[0]["dW"]
                assert torch.equal(_run_embedding(W, ids, di, pad)[1].cpu().double(), want), (name, "zeroed dW")
            if dtype == torch.bfloat16:
                di = _int_dout(n_tok, H)
                base = torch.randint(-1000, 1001, (vocab, H), generator=g).float()
                want0 = R.embedding_reference(ids, W, di, pad)[0]["dW"]
                want1 = R.embedding_reference(ids, W, di, pad, base=base)[0]["dW"]
                assert want1.abs().max() < 2 ** 24
                assert torch.equal(_run_embedding_main_grad(W, ids, di, pad, None).cpu().double(), want0), (name, "zeroed")
                assert torch.equal(_run_embedding_main_grad(W, ids, di, pad, base).cpu().double(), want1), (name, "accumulated")
    _finish(fails)


# ====================================================================== rotary
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("S", R.ROPE_S)
@pytest.mark.parametrize("D", R.ROPE_D)
def test_rotary(D, S, dtype):
    fails = []
    B, nh = 2, 3
    cos, sin = R.rope_tables(S, D)
    cosd, sind = bordered(cos), bordered(sin)
    g = torch.Generator().manual_seed(D + S)
    x_cpu, dy_cpu = (torch.randn(B, S, nh, D, generator=g).to(dtype) for _ in range(2))
    for inv in (False, True):
        ref, mag = R.rope_reference(x_cpu, cos, sin, inv, dy_cpu)
        runs = []
        for _ in range(2):
            x = bordered(x_cpu).requires_grad_()
            with sentinels() as (a, calls):
                y = F.apply_rotary(x, cosd, sind, inverse=inv)
                y.backward(bordered(dy_cpu))
                back = F.apply_rotary(y.detach(), cosd, sind, inverse=not inv)
            assert a.intact() and calls == ["pa_rope"] * 3, calls
            runs.append(dict(y=y.detach(), dx=x.grad, back=back))
        for n in ("y", "dx", "back"):
            assert _same_bits(runs[0][n], runs[1][n]), (D, S, inv, n)
        st = {n: R.row_stat(runs[0][n], ref[n], mag[n]) for n in ("y", "dx")}
        # forward then inverse: x again, within the same bound (a rounded y in, a rounded x out)
        st["roundtrip"] = R.row_stat(runs[0]["back"], x_cpu.double(), mag["y"])
        _record("apply_rotary", dtype, st, {n: R.sum_bound(dtype) for n in st}, (D, S, inv), fails)
    _finish(fails)


def _pa_rope(x, x_ts, y, y_ts, cos, sin, pos, B, S, nh, n_rot, D, backward):
    _native.call("pa_rope", _native.dt(x), _native.dt(y), _native.ptr(x), x_ts, _native.ptr(y), y_ts, _native.ptr(cos),
                 _native.ptr(sin), _native.ptr(pos), B, S, nh, n_rot, D, int(backward), _native.stream())
    torch.cuda.synchronize()


def _strided(t_cpu, ts, fill):
    """[B, S, nh, D] -> device [B*S, nh*D] view of a [B*S, ts] parent filled with ``fill``
    (itself inside a border), holding t."""
    B, S, nh, D = t_cpu.shape
    parent = bordered(torch.full((B * S, ts), fill, dtype=t_cpu.dtype), fill)
    v = parent[:, : nh * D]
    v.copy_(t_cpu.reshape(B * S, nh * D))
    return parent, v


def _gap_intact(parent, width, fill=SENT):
    s = torch.full((), fill, dtype=parent.dtype, device=parent.device)
    flat = parent._base
    return bool((parent[:, width:] == s).all() and (flat[:PAD] == s).all() and (flat[PAD + parent.numel():] == s).all())


@pytest.mark.parametrize("case", ["n_rot", "pos", "stride", "alias", "fp32_to_bf16"])
def test_pa_rope_direct(case):
    """pa_rope as the attention wrappers call it: copied heads past n_rot (bit-equal to the
    input), position ids, a token stride over nh * D, in place, fp32 in -> bf16 out."""
    fails = []
    B, S, nh, D = 2, 37, 3, 64
    tab = 50
    cos, sin = R.rope_tables(tab, D)
    cosd, sind = bordered(cos), bordered(sin)
    g = torch.Generator().manual_seed(5)
    in_dt = torch.float32 if case == "fp32_to_bf16" else torch.bfloat16
    x_cpu = torch.randn(B, S, nh, D, generator=g).to(in_dt)
    n_rot = 2 if case == "n_rot" else nh
    pos_cpu = torch.randint(0, tab, (B, S), generator=g) if case == "pos" else None
    ts = nh * D + (64 if case == "stride" else 0)
    for backward in (False, True):
        runs = []
        for _ in range(2):
            if case == "alias":
                # in place: the surroundings of x are the output's, so a sentinel instead of NaN
                yp, yv = xp, xv = _strided(x_cpu, ts, SENT)
            else:
                xp, xv = _strided(x_cpu, ts, float("nan"))
                yp, yv = _strided(torch.full(x_cpu.shape, SENT, dtype=torch.bfloat16), ts, SENT)
            _pa_rope(xv, ts, yv, ts, cosd, sind, None if pos_cpu is None else pos_cpu.to(dev), B, S, nh, n_rot, D,
                     backward)
            assert _gap_intact(yp, nh * D), (case, "stray store")
            runs.append(yv.reshape(B, S, nh, D))
        got = runs[0]
        assert _same_bits(got, runs[1]), (case, backward, "differs between two runs")
        ref, mag = R.rope_reference(x_cpu, cos, sin, backward, None, pos_cpu, n_rot, out_dtype=torch.bfloat16)
        if case == "n_rot":
            assert _same_bits(got[:, :, n_rot:].cpu(), x_cpu[:, :, n_rot:]), "copied heads changed"
        _record("pa_rope " + case, torch.bfloat16, {"y": R.row_stat(got, ref["y"], mag["y"])}, {"y": R.BF16_BOUND},
                (case, backward), fails)
    _finish(fails)


# ====================================================================== SwiGLU
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("N", R.SWIGLU_N)
@pytest.mark.parametrize("I", R.SWIGLU_I)
def test_swiglu(I, N, dtype):
    """Gates of +-30, +-100 and 0 next to ordinary ones: __expf(-g) runs to 0 and to inf, the
    results stay finite and in bound."""
    fails = []
    gu_cpu, dout_cpu = R.swiglu_inputs(N, I, dtype)
    ref, mag = R.swiglu_reference(gu_cpu, dout_cpu)
    runs = []
    for _ in range(2):
        gu = bordered(gu_cpu).requires_grad_()
        with sentinels() as (a, calls):
            out = F.swiglu(gu)
            out.backward(bordered(dout_cpu))
        assert a.intact() and calls == ["pa_swiglu_fwd", "pa_swiglu_bwd"], calls
        runs.append(dict(out=out.detach(), dgu=gu.grad))
    for n in ("out", "dgu"):
        assert torch.isfinite(runs[0][n]).all(), n
        assert _same_bits(runs[0][n], runs[1][n]), n
    st = {n: R.row_stat(runs[0][n], ref[n], mag[n]) for n in ("out", "dgu")}
    _record("swiglu", dtype, st, {n: R.exp_bound(dtype) for n in st}, (I, N), fails)
    _finish(fails)


def test_swiglu_routing():
    """Halves that are not whole 8-element vectors never reach the kernel: I = 12 runs the
    reference path; an odd last dimension (17) has no [gate | up] split at all and is
    refused with a ValueError, instead of the kernel reading rows of 16 out of rows of 17."""
    fails = []
    for dtype in DTYPES:
        gu_cpu, dout_cpu = R.swiglu_inputs(5, 12, dtype)
        ref, mag = R.swiglu_reference(gu_cpu, dout_cpu)
        runs = []
        for _ in range(2):
            gu = bordered(gu_cpu).requires_grad_()
            with sentinels() as (a, calls):
                out = F.swiglu(gu)
                out.backward(bordered(dout_cpu))
            assert calls == [] and a.intact()
            runs.append(dict(out=out.detach(), dgu=gu.grad))
        for n in ("out", "dgu"):
            assert _same_bits(runs[0][n], runs[1][n]), n
        st = {n: R.row_stat(runs[0][n], ref[n], mag[n]) for n in ("out", "dgu")}
        _record("swiglu, reference path", dtype, st, {n: R.exp_bound(dtype) for n in st}, 12, fails)
        with sentinels() as (a, calls):
            with pytest.raises(ValueError):
                F.swiglu(bordered(torch.randn(4, 17).to(dtype)))
        assert calls == []
    _finish(fails)
