"""Every attention kernel path against the per-row float64 oracle (tests/attn_oracle.py)
on adversarial score profiles, at the smallest shapes that straddle each tile edge.

A path is forced through its knob, and the test asserts that it was the one that ran:
the native calls are recorded by a spy and the launchers report the kernel they resolved
to (``pa_fa_fwd_last`` / ``pa_fa_bwd_last``).  Every knob is restored in ``finally``.
O / dQ / dK / dV must meet ``row_stat <= 8u``, LSE 1e-4 (exactly -inf on rows with no
key), everything finite.  Each test prints its worst statistic per path; the module
prints the whole table when it finishes (the one kept in attn_oracle's docstring).
"""
import contextlib
import math

import pytest
import torch

import attn_oracle as AO
from paddle_amd import ops
from paddle_amd.ops import _native
from paddle_amd.ops import fused as F

pytestmark = pytest.mark.gpu

dev = "cuda"
B = 2
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nworst statistic per path (bound %.4e, LSE %.0e)" % (AO.BOUND, AO.LSE_TOL))
    for path in sorted(WORST):
        print("    %-34s " % path + "  ".join(f"{n} {s:.2e}" for n, s in WORST[path].items()))


def _check(path, got, ref, what=""):
    """Record, then assert the bounds on every result in ``got``."""
    st = AO.stats(got, ref)
    w = WORST.setdefault(path, {})
    for n, s in st.items():
        w[n] = max(w.get(n, 0.0), s)
    bad = {n: s for n, s in st.items() if not s <= (AO.LSE_TOL if n == "LSE" else AO.BOUND)}
    return [(path, what, n, s) for n, s in bad.items()]


def _finish(path, failures):
    print(f"{path}: worst " + "  ".join(f"{n} {s:.2e}" for n, s in WORST.get(path, {}).items()))
    assert not failures, failures[:8]


@contextlib.contextmanager
def knobs(fwd=2, bwd=4, split=True):
    """Force the forward kernel, the single-kernel backward variant and the split
    backward on / off; yields the list of native calls made inside."""
    calls = []
    orig = _native.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    old_split = F._FA_SPLIT
    old_fwd, old_bwd = _native.lib().pa_fa_fwd_get_variant(), _native.lib().pa_fa_bwd_get_variant()
    try:
        orig("pa_fa_fwd_set_variant", fwd)
        orig("pa_fa_bwd_set_variant", bwd)
        F._FA_SPLIT = split
        _native.call = spy
        yield calls
    finally:
        _native.call = orig
        F._FA_SPLIT = old_split
        orig("pa_fa_fwd_set_variant", old_fwd)
        orig("pa_fa_bwd_set_variant", old_bwd)


@contextlib.contextmanager
def capture_fwd():
    """Record what every F._fa_fwd call inside was given and returned."""
    seen = []
    orig = F._fa_fwd

    def fwd(q, k, v, causal, scale, out=None):
        o, lse = orig(q, k, v, causal, scale, out=out)
        seen.append((q, k, v, o, lse))
        return o, lse

    F._fa_fwd = fwd
    try:
        yield seen
    finally:
        F._fa_fwd = orig


def _fwd_last():
    return _native.lib().pa_fa_fwd_last()


def _bwd_last():
    return _native.lib().pa_fa_bwd_last()


def run_flash(inp, causal, scale):
    """ops.flash_attention forward + backward; returns the results under the oracle's names."""
    q, k, v, do = (x.to(dev) for x in inp)
    q, k, v = (x.requires_grad_() for x in (q, k, v))
    with capture_fwd() as seen:
        o = ops.flash_attention(q, k, v, causal=causal, scale=scale)
        o.backward(do)
    assert len(seen) == 1
    return dict(O=o.detach(), LSE=seen[0][4], dQ=q.grad, dK=k.grad, dV=v.grad)


def _assert_split(calls):
    assert "pa_fa_bwd_split" in calls and "pa_flash_attn_bwd" not in calls, calls


def _assert_single(calls, D, variant):
    assert "pa_flash_attn_bwd" in calls and "pa_fa_bwd_split" not in calls, calls
    assert _bwd_last() == 10 * D + variant, (_bwd_last(), D, variant)


# ------------------------------------------------------------------ default paths, full product
@pytest.mark.parametrize("Hq,Hk", AO.HEADS)
@pytest.mark.parametrize("Sq,Sk,causal", AO.shape_cases())
def test_default_paths(Sq, Sk, causal, Hq, Hk):
    """fa_fwd_kernel2<128> and the split backward (fa_bwd_split.hip) over the whole
    matrix: every profile and scale at every shape, head configuration and mask."""
    D, path, fails = 128, "fwd2<128> + split bwd", []
    for profile in AO.PROFILES:
        for f in AO.SCALE_FACTORS:
            scale = f / math.sqrt(D)
            inp = AO.make_inputs(profile, B, Sq, Sk, Hq, Hk, D, scale)
            ref = AO.reference(*inp, causal, scale)
            with knobs() as calls:
                got = run_flash(inp, causal, scale)
            assert _fwd_last() == 10 * D + 2
            _assert_split(calls)
            fails += _check(path, got, ref, (profile, f))
    _finish(path, fails)


# ------------------------------------------------------------------ the other forwards
FWD_PATHS = {"fwd1<128>": (128, 1, 1), "fwd1<64>": (64, 2, 1), "fwd1<256>": (256, 2, 1)}  # D, knob, kernel


@pytest.mark.parametrize("Sq,Sk,causal", AO.PATH_SHAPES + [AO.EMPTY_CASE])
@pytest.mark.parametrize("path", list(FWD_PATHS))
def test_forward_paths(path, Sq, Sk, causal):
    D, knob, kern = FWD_PATHS[path]
    fails = []
    for profile, Hq, Hk, scale in AO.path_cases(D, Sq):
        inp, ref = AO.case(profile, B, Sq, Sk, Hq, Hk, D, scale, causal)
        q, k, v, _ = (x.to(dev) for x in inp)
        with knobs(fwd=knob) as calls:
            o, lse = F._fa_fwd(q, k, v, causal, scale)
        assert calls == ["pa_flash_attn_fwd"] and _fwd_last() == 10 * D + kern, (calls, _fwd_last())
        fails += _check(path, dict(O=o, LSE=lse), ref, profile)
    _finish(path, fails)


# ------------------------------------------------------------------ single-kernel backwards
V4_SHAPES = [(65, 257, True), (129, 129, True), (257, 257, True), AO.EMPTY_CASE]  # v4 is causal only
V5_SHAPES = [(128, 256, True), (256, 256, True), (256, 128, True)]  # Sq % 32, Sk % 128; the last has empty rows
BWD_PATHS = [(128, 0), (128, 1), (128, 3), (128, 4), (128, 5), (64, 0), (64, 1), (256, 0)]


def _bwd_cases():
    out = []
    for D, var in BWD_PATHS:
        shapes = V4_SHAPES if var == 4 else V5_SHAPES if var == 5 else AO.PATH_SHAPES + [AO.EMPTY_CASE]
        out += [(D, var, *s) for s in shapes]
    return out


@pytest.mark.parametrize("D,variant,Sq,Sk,causal", _bwd_cases())
def test_backward_variants(D, variant, Sq, Sk, causal):
    """The single-kernel backwards (split path off): variant 0 is also the fallback for
    offsets past 2^31, 3 / 5 are reachable through the A/B knob only."""
    path, fails = f"bwd v{variant}<{D}>", []
    for profile, Hq, Hk, scale in AO.path_cases(D, Sq):
        inp, ref = AO.case(profile, B, Sq, Sk, Hq, Hk, D, scale, causal)
        with knobs(bwd=variant, split=False) as calls:
            got = run_flash(inp, causal, scale)
        _assert_single(calls, D, variant)
        got.pop("O"), got.pop("LSE")  # the forward has its own tests
        fails += _check(path, got, ref, profile)
    _finish(path, fails)


# ------------------------------------------------------------------ split backward with rotary
def _tables(S, D):
    return F.rope_tables(S, D, device=dev)


@pytest.mark.parametrize("Sq,Sk,causal", AO.PATH_SHAPES + [AO.EMPTY_CASE])
def test_split_backward_rotary(Sq, Sk, causal):
    """F._fa_bwd_split with cos / sin: the kernel is given rotated q / k and stores dq / dk
    rotated back.  The profile lives in the rotated q / k (what the kernel sees); the
    reference starts from their exact un-rotated preimage in float64."""
    D, path, fails = 128, "split bwd + rotary", []
    cos, sin = _tables(max(Sq, Sk), D)
    for profile, Hq, Hk, scale in AO.path_cases(D, Sq):
        inp, _ = AO.case(profile, B, Sq, Sk, Hq, Hk, D, scale, causal)
        q, k, v, do = (x.to(dev) for x in inp)
        xq = AO.rotate(inp[0].double(), cos.cpu(), sin.cpu(), -1.0)
        xk = AO.rotate(inp[1].double(), cos.cpu(), sin.cpu(), -1.0)
        ref = AO.reference(xq, xk, inp[2], inp[3], causal, scale, cos, sin)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        with knobs() as calls:
            o, lse = F._fa_fwd(q, k, v, causal, scale)
            assert F._fa_bwd_split(q, k, v, o, do, lse, causal, scale, dq, dk, dv, cos, sin)
        _assert_split(calls)
        fails += _check(path, dict(O=o, LSE=lse, dQ=dq, dK=dk, dV=dv), ref, profile)
    _finish(path, fails)


# ------------------------------------------------------------------ wrappers
def _packed_from(parts):
    Bn, S = parts[0].shape[:2]
    return torch.cat([p.reshape(Bn, S, -1) for p in parts], -1).contiguous()


def _wrapper_check(path, seen, grad, do, causal, scale, Hq, Hk, D, cos, sin, what):
    """Reference from the q / k / v views the forward kernel was actually given (the
    rotated, bf16-rounded values), gradients with respect to the un-rotated input."""
    assert len(seen) == 1
    q, k, v, o, lse = seen[0]
    if cos is not None:
        xq = AO.rotate(q.cpu().double(), cos.cpu(), sin.cpu(), -1.0)
        xk = AO.rotate(k.cpu().double(), cos.cpu(), sin.cpu(), -1.0)
    else:
        xq, xk = q, k
    Bn, S = q.shape[:2]
    ref = AO.reference(xq, xk, v, do.view(Bn, S, Hq, D), causal, scale, cos, sin)
    g4 = grad.view(Bn, S, Hq + 2 * Hk, D)
    got = dict(O=o, LSE=lse, dQ=g4[:, :, :Hq], dK=g4[:, :, Hq:Hq + Hk], dV=g4[:, :, Hq + Hk:])
    return _check(path, got, ref, what)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("S,causal", [(64, True), (129, True), (257, True), (193, False)])
def test_packed_attention(S, causal, split):
    D, H, fails = 128, 2, []
    path = "packed_attention, split " + ("on" if split else "off")
    for profile, _, _, scale in AO.path_cases(D, S):
        inp, _ = AO.case(profile, B, S, S, H, H, D, scale, causal)
        qkv = _packed_from(inp[:3]).to(dev).requires_grad_()
        do = inp[3].to(dev).view(B, S, H * D)
        with knobs(split=split) as calls, capture_fwd() as seen:
            ops.packed_attention(qkv, H, causal=causal, scale=scale).backward(do)
        if split:
            _assert_split(calls)
        else:
            _assert_single(calls, D, 4 if causal else 1)
            # causal: the slab reduce fused with the (identity) rotary and the bf16 store
            assert ("pa_fa_dq_reduce_rope" in calls) == causal, calls
        fails += _wrapper_check(path, seen, qkv.grad, inp[3], causal, scale, H, H, D, None, None, profile)
    _finish(path, fails)


def _unrotated(inp, cos, sin):
    """bf16 q, k whose rotation (rounded to bf16 again by the op) is close to the
    profile's q, k; v and do as they are."""
    q = AO.rotate(inp[0].double(), cos.cpu(), sin.cpu(), -1.0).to(torch.bfloat16)
    k = AO.rotate(inp[1].double(), cos.cpu(), sin.cpu(), -1.0).to(torch.bfloat16)
    return q, k, inp[2]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("S", [64, 129, 257])
def test_rope_attention(S, split):
    D, causal, fails = 128, True, []
    path = "rope_attention, split " + ("on" if split else "off")
    cos, sin = _tables(S, D)
    for profile, Hq, Hk, scale in AO.path_cases(D, S):
        inp, _ = AO.case(profile, B, S, S, Hq, Hk, D, scale, causal)
        qkv = _packed_from(_unrotated(inp, cos, sin)).to(dev).requires_grad_()
        do = inp[3].to(dev).view(B, S, Hq * D)
        with knobs(split=split) as calls, capture_fwd() as seen:
            ops.rope_attention(qkv, cos, sin, Hq, Hk, causal=causal, scale=scale).backward(do)
        if split:
            _assert_split(calls)
        else:
            _assert_single(calls, D, 4)
            assert "pa_fa_dq_reduce_rope" in calls, calls
            assert ("pa_fa_gqa_fold" in calls) == (Hq != Hk), calls
        fails += _wrapper_check(path, seen, qkv.grad, inp[3], causal, scale, Hq, Hk, D, cos, sin, profile)
    _finish(path, fails)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("Bn,S", [(4, 256), (8, 129), (8, 128)])
def test_qkv_rope_attention(Bn, S, split):
    """The projection GEMM with the rotary in its epilogue feeding the attention.  The
    weight is the identity, so the projection is exact in bf16 and y.grad *is* dqkv.
    The fused node needs at least 1024 tokens in a multiple of 8, so these tests run
    B = 4 / 8 (and no odd S times B): all profiles at three shapes."""
    D, causal, fails = 128, True, []
    path = "qkv_rope_attention, split " + ("on" if split else "off")
    cos, sin = _tables(S, D)
    for profile, Hq, Hk, scale in AO.path_cases(D, S):
        inp, _ = AO.case(profile, Bn, S, S, Hq, Hk, D, scale, causal)
        y = _packed_from(_unrotated(inp, cos, sin)).to(dev).requires_grad_()
        W = y.shape[-1]
        w = torch.eye(W, device=dev, dtype=torch.bfloat16).requires_grad_()
        do = inp[3].to(dev).view(Bn, S, Hq * D)
        epi, orig_epi = [], F._G.gemm_epi
        F._G.gemm_epi = lambda *a, **kw: epi.append(a[0]) or orig_epi(*a, **kw)
        try:
            with knobs(split=split) as calls, capture_fwd() as seen:
                ops.qkv_rope_attention(y, w, cos, sin, Hq, Hk, causal=causal, scale=scale).backward(do)
        finally:
            F._G.gemm_epi = orig_epi
        assert epi == [F._G.EPI_ROPE], epi  # the fused node, not rope_attention(linear(...))
        assert "pa_rope" not in calls or not split, calls
        if split:
            _assert_split(calls)
        else:
            _assert_single(calls, D, 4)
            assert "pa_fa_dq_reduce_rope" in calls, calls
        fails += _wrapper_check(path, seen, y.grad, inp[3], causal, scale, Hq, Hk, D, cos, sin, profile)
    _finish(path, fails)


@pytest.mark.parametrize("wrapper", ["rope_attention", "packed_attention", "qkv_rope_attention"])
def test_packed_wrappers_variant5(wrapper):
    """Backward variant 5 (A/B knob) under the packed wrappers with the split path off: it
    leaves the slab reduce to the caller (pa_fa_dq_reduce_rope), which the launcher used
    to refuse for every variant but 4."""
    D, S, causal, fails = 128, 256, True, []
    Bn = 4 if wrapper == "qkv_rope_attention" else B  # the fused projection needs 1024 tokens
    path = wrapper + ", v5"
    cos, sin = _tables(S, D)
    for profile, Hq, Hk, scale in AO.path_cases(D, S):
        if wrapper == "packed_attention":
            Hk = Hq
        inp, _ = AO.case(profile, Bn, S, S, Hq, Hk, D, scale, causal)
        do = inp[3].to(dev).view(Bn, S, Hq * D)
        with knobs(bwd=5, split=False) as calls, capture_fwd() as seen:
            if wrapper == "rope_attention":
                qkv = _packed_from(_unrotated(inp, cos, sin)).to(dev).requires_grad_()
                ops.rope_attention(qkv, cos, sin, Hq, Hk, causal=causal, scale=scale).backward(do)
            elif wrapper == "qkv_rope_attention":
                qkv = _packed_from(_unrotated(inp, cos, sin)).to(dev).requires_grad_()
                w = torch.eye(qkv.shape[-1], device=dev, dtype=torch.bfloat16).requires_grad_()
                ops.qkv_rope_attention(qkv, w, cos, sin, Hq, Hk, causal=causal, scale=scale).backward(do)
                assert "pa_rope" in calls and calls.index("pa_rope") > calls.index("pa_flash_attn_bwd"), calls
            else:
                qkv = _packed_from(inp[:3]).to(dev).requires_grad_()
                ops.packed_attention(qkv, Hq, causal=causal, scale=scale).backward(do)
        _assert_single(calls, D, 5)
        assert "pa_fa_dq_reduce_rope" in calls, calls
        rot = (None, None) if wrapper == "packed_attention" else (cos, sin)
        fails += _wrapper_check(path, seen, qkv.grad, inp[3], causal, scale, Hq, Hk, D, *rot, profile)
    _finish(path, fails)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Hq,Hk", [(2, 2), (4, 1)])
def test_flash_attention_varlen(causal, Hq, Hk):
    """Packed sequences with different q and k lengths: an empty q, a k shorter than q
    (causal: query rows with no key) and lengths across the tile edges."""
    D, path, fails = 128, "flash_attention_varlen", []
    lq, lk = [1, 65, 0, 129], [3, 33, 5, 129]
    cq, ck = [0], [0]
    for a, b_ in zip(lq, lk):
        cq.append(cq[-1] + a)
        ck.append(ck[-1] + b_)
    for i, profile in enumerate(AO.PROFILES):
        scale = AO.SCALE_FACTORS[i % 3] / math.sqrt(D)
        seqs = [AO.make_inputs(profile, 1, max(a, 1), b_, Hq, Hk, D, scale, seed=j)
                for j, (a, b_) in enumerate(zip(lq, lk))]
        seqs = [tuple(x if n in (1, 2) else x[:, :a] for n, x in enumerate(s)) for s, a in zip(seqs, lq)]
        q, k, v, do = (torch.cat([s[n][0] for s in seqs]).to(dev) for n in range(4))
        q, k, v = (x.requires_grad_() for x in (q, k, v))
        with knobs() as calls:
            o = ops.flash_attention_varlen(q, k, v, cq, ck, causal=causal, scale=scale)
            o.backward(do)
        assert calls.count("pa_flash_attn_fwd") == 3 and calls.count("pa_flash_attn_bwd") == 3, calls
        assert "pa_fa_bwd_split" not in calls and _fwd_last() == 10 * D + 2
        assert _bwd_last() == 10 * D + (4 if causal else 1)  # the default single-kernel backward
        for j, s in enumerate(seqs):
            ref = AO.reference(*s, causal, scale)
            got = dict(O=o[cq[j]:cq[j + 1]][None], dQ=q.grad[cq[j]:cq[j + 1]][None],
                       dK=k.grad[ck[j]:ck[j + 1]][None], dV=v.grad[ck[j]:ck[j + 1]][None])
            fails += _check(path, got, ref, (profile, j))
    _finish(path, fails)


# ------------------------------------------------------------------ decode
KV_LEN = [1, 2, 63, 65, 257]


@pytest.mark.parametrize("D,Hq,Hk", [(128, 8, 2), (128, 4, 1), (64, 2, 2)])
def test_decode_attention(D, Hq, Hk):
    """The split-KV decode kernel: every profile and scale, split counts from one to more
    splits than keys (the merge sees empty splits and maxima far apart)."""
    path, fails, S_max, Bn = f"decode<{D}>", [], 264, len(KV_LEN)
    kv_len = torch.tensor(KV_LEN, dtype=torch.int32, device=dev)
    for profile in AO.PROFILES:
        for f in AO.SCALE_FACTORS:
            scale = f / math.sqrt(D)
            rows = [AO.make_inputs(profile, 1, 1, n, Hq, Hk, D, scale, seed=b) for b, n in enumerate(KV_LEN)]
            cache = ops.KVCache(1, Bn, S_max, Hk, D, torch.bfloat16, dev)
            # slots past kv_len hold inf: reading one turns the output into inf / NaN
            cache.k[0].fill_(float("inf"))
            cache.v[0].fill_(float("inf"))
            for b, (r, n) in enumerate(zip(rows, KV_LEN)):
                cache.k[0][b, :n] = r[1][0].to(dev)
                cache.v[0][b, :n] = r[2][0].to(dev)
            q = torch.cat([r[0] for r in rows]).to(dev)
            refs = [AO.reference(*r, False, scale) for r in rows]
            ref = {n: torch.cat([x[n] for x in refs]) for n in ("O", "magO")}
            for ns in (1, 2, 5, 64):
                with knobs() as calls:
                    o = ops.decode_attention(q, cache, 0, scale=scale, num_splits=ns, kv_len=kv_len)
                assert calls == ["pa_attn_decode"], calls
                fails += _check(path, dict(O=o), ref, (profile, f, ns))
    _finish(path, fails)


# ------------------------------------------------------------------ poisoned surroundings
def _in_poison(x, pad_rows=3):
    """x [B, S, H, D] as a view into a NaN-filled parent with padding rows after S and one
    spare head (row stride (H + 1) D: a multiple of 8 elements)."""
    Bn, S, H, D = x.shape
    parent = torch.full((Bn, S + pad_rows, H + 1, D), float("nan"), dtype=x.dtype, device=dev)
    view = parent[:, :S, :H]
    view.copy_(x)
    return view


class _Sentinel:
    """An output view into a sentinel-filled parent; ``intact()`` compares every byte
    outside the view with the sentinel, bitwise."""

    def __init__(self, shape, dtype=torch.bfloat16, pad_rows=3):
        Bn, S, H, D = shape
        self.parent = torch.full((Bn, S + pad_rows, H + 1, D), -7.5, dtype=dtype, device=dev)
        self.view = self.parent[:, :S, :H]
        self.S, self.H = S, H

    def intact(self):
        p = self.parent.clone()
        p[:, :self.S, :self.H] = -7.5
        return torch.equal(p.view(torch.int16), torch.full_like(p, -7.5).view(torch.int16))


class _SentinelFlat:
    """A contiguous fp32 [B, S, H, D] block (the single-kernel backward's dQ accumulator,
    which has no strides) with a sentinel border before and after it."""

    PAD = 4096

    def __init__(self, shape):
        n = math.prod(shape)
        self.parent = torch.full((n + 2 * self.PAD,), -7.5, dtype=torch.float32, device=dev)
        self.view = self.parent[self.PAD:self.PAD + n].view(shape)

    def intact(self):
        edge = torch.cat([self.parent[:self.PAD], self.parent[-self.PAD:]])
        return torch.equal(edge.view(torch.int32), torch.full_like(edge, -7.5).view(torch.int32))


@pytest.mark.parametrize("Sq,Sk,causal", [(65, 257, True), (193, 127, False), (130, 66, True)])
@pytest.mark.parametrize("path", ["fwd2 + split", "fwd1 + v4/v1", "v0"])
def test_poisoned_surroundings(path, Sq, Sk, causal):
    """q / k / v / do bordered by NaN, outputs bordered by a sentinel: a read past a tail
    tile poisons the result, a stray store changes the sentinel."""
    D, Hq, Hk, fails = 128, 4, 1, []
    fwd, bwd, split = {"fwd2 + split": (2, 4, True), "fwd1 + v4/v1": (1, 4, False), "v0": (2, 0, False)}[path]
    for profile in ("flat", "ramp_fast"):
        scale = 1.0 / math.sqrt(D)
        inp, ref = AO.case(profile, B, Sq, Sk, Hq, Hk, D, scale, causal)
        q, k, v, do = (_in_poison(x.to(dev)) for x in inp)
        o = _Sentinel(q.shape)
        dk_heads = Hk if split else Hq  # the single-kernel backward writes dK / dV per query head
        dq = _Sentinel(q.shape) if split else _SentinelFlat(q.shape)
        dk, dv = _Sentinel((B, Sk, dk_heads, D)), _Sentinel((B, Sk, dk_heads, D))
        with knobs(fwd=fwd, bwd=bwd, split=split) as calls:
            _, lse = F._fa_fwd(q, k, v, causal, scale, out=o.view)
            assert _fwd_last() == 10 * D + fwd
            if split:
                assert F._fa_bwd_split(q, k, v, o.view, do, lse, causal, scale, dq.view, dk.view, dv.view)
                got_dq, got_dk, got_dv = dq.view, dk.view, dv.view
            else:
                got_dq = F._fa_bwd(q, k, v, o.view, do, lse, causal, scale, dk.view, dv.view, dq_acc=dq.view)
                assert got_dq is dq.view
                _assert_single(calls, D, (4 if causal else 1) if bwd == 4 else bwd)
                got_dk = dk.view.reshape(B, Sk, Hk, Hq // Hk, D).float().sum(3)
                got_dv = dv.view.reshape(B, Sk, Hk, Hq // Hk, D).float().sum(3)
        if split:
            _assert_split(calls)
        name = "poisoned, " + path
        fails += _check(name, dict(O=o.view, LSE=lse, dQ=got_dq, dK=got_dk, dV=got_dv), ref, profile)
        for n, s in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert s.intact(), f"{path} {profile}: stray store around {n}"
    _finish(name, fails)
