"""The row-kernel oracle itself (tests/row_oracle.py), on the CPU: each reference against
float64 autograd of the textbook formula, the bounds against the fp32 / storage-dtype
emulation at every shape the GPU test runs, the mutations a bound must catch (and the
whole-tensor ratio that misses them), and the routing of the norm wrappers."""
import pytest
import torch
import torch.nn.functional as TF

import row_oracle as R
from paddle_amd.ops import fused as F

DTYPES = [torch.bfloat16, torch.float32]
f64 = torch.float64


def _close(a, b, tol=1e-11):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def _rounded(out, dtype, names):
    """What a kernel with this bug and otherwise exact arithmetic would return."""
    return {n: (out[n].to(dtype) if out.get(n) is not None else None) for n in names}


# ------------------------------------------------------------------ 1. references == float64 autograd
@pytest.mark.parametrize("rms,with_res,use_dh,with_bias", R.NORM_VARIANTS)
def test_norm_reference_is_autograd(rms, with_res, use_dh, with_bias):
    inp = {k: (None if v is None else v.double()) for k, v in R.norm_inputs("flat", 7, 24, f64, with_res, with_bias).items()}
    eps = R.norm_eps(rms)
    ref, _ = R.norm_reference(inp["x"], inp["res"], inp["w"], inp["b"], inp["dy"], inp["dh"] if use_dh else None, eps, rms)
    leaves = {k: inp[k].clone().requires_grad_() for k in ("x", "res", "w", "b") if inp[k] is not None}
    h = leaves["x"] + leaves["res"] if with_res else leaves["x"]
    if rms:
        y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * leaves["w"]
    else:
        y = TF.layer_norm(h, (24,), leaves["w"], leaves.get("b"), eps)
    loss = (y * inp["dy"]).sum() + ((h * inp["dh"]).sum() if use_dh else 0)
    loss.backward()
    _close(ref["y"], y.detach())
    _close(ref["dx"], leaves["x"].grad)
    _close(ref["dw"], leaves["w"].grad)
    if with_res:
        _close(ref["h"], h.detach())
        _close(ref["dx"], leaves["res"].grad)
    if with_bias:
        _close(ref["db"], leaves["b"].grad)
    if not rms:
        _close(ref["mean"], h.detach().mean(-1))
        _close(ref["rstd"], torch.rsqrt(h.detach().var(-1, unbiased=False) + eps))


@pytest.mark.parametrize("reduction", ["mean", "none", "sum"])
@pytest.mark.parametrize("profile", ["flat", "spike", "ties"])
def test_ce_reference_is_autograd(profile, reduction):
    N, V = 11, 29
    x, hot = R.logit_inputs(profile, N, V, f64)
    lab = R.make_labels(x, hot, kinds=("first", "last", "ignored", "random"))
    up = torch.randn(N, dtype=f64) if reduction == "none" else 1.7
    ref, _ = R.ce_reference(x, lab, up, -100, reduction)
    xa = x.clone().requires_grad_()
    out = TF.cross_entropy(xa, lab, ignore_index=-100, reduction=reduction)
    (out * up).sum().backward()
    _close(ref["loss" if reduction == "none" else reduction], out.detach())
    _close(ref["dlogits"], xa.grad)
    _close(ref["lse"], torch.logsumexp(x, -1))


def test_ce_reference_defines_what_torch_leaves_nan():
    x, hot = R.logit_inputs("flat", 6, 13, f64)
    ref, _ = R.ce_reference(x, torch.full((6,), -100), 1.0, -100, "mean")
    assert ref["mean"].item() == 0 and not ref["dlogits"].any() and not ref["loss"].any()
    lab = torch.tensor([13, 5000, -7, 2, 0, 12])
    ref, _ = R.ce_reference(x, lab, 1.0, -100, "mean")
    assert not ref["loss"][:3].any() and not ref["dlogits"][:3].any() and ref["loss"][3:].all()
    _close(ref["mean"], ref["loss"][3:].mean())


@pytest.mark.parametrize("log", [False, True])
def test_softmax_reference_is_autograd(log):
    x, _ = R.logit_inputs("flat", 5, 19, f64)
    dy = torch.randn(5, 19, dtype=f64)
    ref, _ = R.softmax_reference(x, dy, log)
    xa = x.clone().requires_grad_()
    y = torch.log_softmax(xa, -1) if log else torch.softmax(xa, -1)
    y.backward(dy)
    _close(ref["y"], y.detach())
    _close(ref["dx"], xa.grad)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("profile", R.MASKED_PROFILES)
def test_softmax_reference_on_masked_rows_matches_torch(profile, log):
    # torch is finite (or exactly -inf for log) on these rows; the reference agrees
    x, _ = R.logit_inputs(profile, 9, 64, f64)
    ref, mag = R.softmax_reference(x, None, log)
    want = torch.log_softmax(x, -1) if log else torch.softmax(x, -1)
    assert R.masked_row_stat(ref["y"], want, mag["y"]) < 1e-12


def test_embedding_reference_is_autograd():
    W = torch.randn(40, 16, dtype=f64)
    ids = R.id_patterns(33, 40)["padding"]
    dout = torch.randn(33, 16, dtype=f64)
    ref, _ = R.embedding_reference(ids, W, dout, padding_idx=2)
    Wa = W.clone().requires_grad_()
    out = TF.embedding(ids, Wa, padding_idx=2)
    out.backward(dout)
    want = out.detach().clone()
    want[ids == 2] = 0  # the op reads zeros on padding rows whatever the table holds
    _close(ref["out"], want)
    _close(ref["dW"], Wa.grad)


@pytest.mark.parametrize("inverse", [False, True])
def test_rope_reference_is_complex_rotation(inverse):
    B, S, nh, D = 2, 9, 3, 16
    cos, sin = R.rope_tables(S, D)
    x, dy = torch.randn(B, S, nh, D, dtype=f64), torch.randn(B, S, nh, D, dtype=f64)
    ref, _ = R.rope_reference(x, cos, sin, inverse, dy)
    z = torch.complex(cos.double(), sin.double() * (-1 if inverse else 1)).view(1, S, 1, D // 2)
    xa = x.clone().requires_grad_()
    yc = torch.complex(xa[..., : D // 2], xa[..., D // 2:]) * z
    y = torch.cat([yc.real, yc.imag], -1)
    y.backward(dy)
    _close(ref["y"], y.detach())
    _close(ref["dx"], xa.grad)


def test_swiglu_reference_is_autograd():
    gu, dout = R.swiglu_inputs(5, 16, f64)
    ref, _ = R.swiglu_reference(gu, dout)
    ga = gu.clone().requires_grad_()
    g, u = ga.chunk(2, -1)
    out = TF.silu(g) * u
    out.backward(dout)
    _close(ref["out"], out.detach())
    _close(ref["dgu"], ga.grad)


# ------------------------------------------------------------------ 2. feasibility of every bound
def _assert_room(stats, bounds, what):
    bad = {n: (s, bounds[n]) for n, s in stats.items() if not s * R.EMU_MARGIN <= bounds[n]}
    assert not bad, (what, bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", R.NORM_H)
def test_norm_bounds_feasible(H, dtype):
    for N, prof, rms, with_res, use_dh, with_bias in R.norm_cases(H):
        inp = R.norm_inputs(prof, N, H, dtype, with_res, with_bias)
        ref, mag = R.norm_case_reference(inp, rms, use_dh)
        emu = R.norm_emulated(inp["x"], inp["res"], inp["w"], inp["b"], inp["dy"], inp["dh"] if use_dh else None,
                              R.norm_eps(rms), rms)
        _assert_room(R.norm_stats(emu, ref, mag), R.norm_bounds(dtype, N), (N, prof, rms, with_res, use_dh, with_bias))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", R.NORM_BIG)
def test_norm_bounds_feasible_many_rows(N, H, dtype):
    for rms in (True, False):
        inp = R.norm_inputs("flat", N, H, dtype, True, not rms)
        ref, mag = R.norm_case_reference(inp, rms, True)
        emu = R.norm_emulated(inp["x"], inp["res"], inp["w"], inp["b"], inp["dy"], inp["dh"], R.norm_eps(rms), rms)
        _assert_room(R.norm_stats(emu, ref, mag), R.norm_bounds(dtype, N), (N, H, rms))


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_norm_stats_bounds_feasible(dtype):
    """The case of the GPU test's test_layer_norm_stats: y, the saved mean / rstd and the
    backward from them, every profile at (67, 1032)."""
    for prof in R.NORM_PROFILES:
        inp = R.norm_inputs(prof, 67, 1032, dtype, False, True)
        ref, mag = R.norm_case_reference(inp, False, False)
        emu = R.norm_emulated(inp["x"], None, inp["w"], inp["b"], inp["dy"], None, 1e-5, False)
        st = R.norm_stats(emu, ref, mag)
        assert {"y", "mean", "rstd", "dx", "dw", "db"} <= set(st)
        _assert_room(st, R.norm_bounds(dtype, 67), prof)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", R.SOFTMAX_V)
def test_softmax_ce_bounds_feasible(V, dtype):
    for N in R.SOFTMAX_N:
        for prof in R.LOGIT_PROFILES:
            x, hot = R.logit_inputs(prof, N, V, dtype)
            lab = R.make_labels(x, hot)
            for red in ("mean", "none", "sum"):
                up = torch.linspace(-2, 2, N) if red == "none" else 1.0
                ref, mag = R.ce_reference(x, lab, up, -100, red)
                emu = R.ce_emulated(x, lab, up, -100, red)
                chk = R.ce_check(emu, ref, mag, dtype)
                _assert_room({n: s for n, (s, b) in chk.items()}, {n: b for n, (s, b) in chk.items()}, (N, prof, red))
            if prof in R.MASKED_PROFILES or prof == "flat":
                dy = torch.randn(N, V, generator=torch.Generator().manual_seed(V + N)).to(dtype)
                for log in (False, True):
                    ref, mag = R.softmax_reference(x, dy, log)
                    emu = R.softmax_emulated(x, dy, log)
                    st = {n: R.masked_row_stat(emu[n], ref[n], mag[n]) for n in ("y", "dx")}
                    _assert_room(st, {n: R.exp_bound(dtype) for n in st}, (N, prof, log))


@pytest.mark.parametrize("dtype", DTYPES)
def test_embedding_rope_swiglu_bounds_feasible(dtype):
    for n_tok, H in R.EMB_CASES:
        vocab = n_tok + 8
        g = torch.Generator().manual_seed(n_tok + H)
        W = torch.randn(vocab, H, generator=g).to(dtype)
        dout = torch.randn(n_tok, H, generator=g).to(dtype)
        for name, ids in R.id_patterns(n_tok, vocab).items():
            pad = 2 if name == "padding" else -1
            ref, mag = R.embedding_reference(ids, W, dout, pad)
            emu = R.embedding_emulated(ids, W, dout, pad)
            assert torch.equal(emu["out"].double(), ref["out"])
            nmax = int(torch.bincount(ids).max())
            _assert_room({"dW": R.row_stat(emu["dW"], ref["dW"], mag["dW"])}, {"dW": R.acc_bound(dtype, nmax)},
                         (n_tok, H, name))
    for D in R.ROPE_D:
        for S in R.ROPE_S:
            cos, sin = R.rope_tables(S, D)
            g = torch.Generator().manual_seed(D + S)
            x, dy = (torch.randn(2, S, 3, D, generator=g).to(dtype) for _ in range(2))
            for inv in (False, True):
                ref, mag = R.rope_reference(x, cos, sin, inv, dy)
                emu = R.rope_emulated(x, cos, sin, inv, dy)
                st = {n: R.row_stat(emu[n], ref[n], mag[n]) for n in ("y", "dx")}
                _assert_room(st, {n: R.sum_bound(dtype) for n in st}, (D, S, inv))
                # forward then inverse, as the GPU test runs it: two passes, each of which has its
                # factor of 2 above, so their errors together (triangle inequality, the rotation
                # keeps the norm of the first) have to fit the one bound itself.  In true bf16
                # roundoff 2^-8 = 2u the bound 4u is exactly the worst case of the two roundings.
                y = emu["y"].to(dtype)
                back = R.rope_emulated(y, cos, sin, not inv)["y"]
                rt = R.row_stat(back, x.double(), mag["y"])
                assert rt <= R.sum_bound(dtype), (D, S, inv, rt)
    for I in R.SWIGLU_I:
        for N in R.SWIGLU_N:
            gu, dout = R.swiglu_inputs(N, I, dtype)
            ref, mag = R.swiglu_reference(gu, dout)
            emu = R.swiglu_emulated(gu, dout)
            assert all(torch.isfinite(v).all() for v in emu.values())
            st = {n: R.row_stat(emu[n], ref[n], mag[n]) for n in ("out", "dgu")}
            _assert_room(st, {n: R.exp_bound(dtype) for n in st}, (I, N))


# ------------------------------------------------------------------ 3. mutations
def _caught(stats, bounds):
    return any(not s <= bounds[n] for n, s in stats.items())


def _norm_mutant(inp, rms, mut, dtype, use_dh=True):
    ref, mag = R.norm_case_reference(inp, rms, use_dh)
    bad, _ = R.norm_reference(inp["x"], inp["res"], inp["w"], inp["b"], inp["dy"], inp["dh"] if use_dh else None,
                              R.norm_eps(rms), rms, _mut=mut)
    got = _rounded(bad, dtype, ("y", "dx", "dw", "db"))
    got.update(rstd=bad["rstd"].float())
    return got, ref, mag, bad


@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("H", (8, 64, 256) + R.NORM_H[1:])
def test_mutation_rstd_over_h_minus_8(H, rms):
    """One row's rstd from a sum that leaves out its last 8-element vector: a relative
    change d of about 4 / H in that row's rstd and y.  fp32 sees it at every H; bf16 (bound
    4u = 2^-7) exactly where d exceeds the bound, which is up to H of about 512."""
    N, row = 5, 3
    for dtype in DTYPES:
        inp = R.norm_inputs("flat", N, H, dtype)
        got, ref, mag, bad = _norm_mutant(inp, rms, {"rstd_short_row": row}, dtype, use_dh=False)
        d = abs(bad["rstd"][row].item() / ref["rstd"][row].item() - 1)
        got.pop("rstd")  # the public ops do not return it: y, dx and dw have to show the error
        hit = _caught(R.norm_stats(got, ref, mag), R.norm_bounds(dtype, N))
        if dtype == torch.float32:
            assert hit, (H, d)
        else:
            # y's row statistic is d up to the 0.3u of the output rounding and up to 1 / 1.2 from
            # the 1e-6 max-row term and |w|-weighting: decided outside a band round the bound
            if d > 1.25 * R.BF16_BOUND:
                assert hit, (H, d)
            if d < 0.8 * R.BF16_BOUND:
                assert not hit, (H, d)
            if H <= 256:
                assert hit, (H, d)
            if H >= 1024:
                assert not hit, (H, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("H", R.NORM_H)
def test_mutation_dx_with_neighbours_rstd(H, rms, dtype):
    N = 67
    inp = R.norm_inputs("mixed_rows", N, H, dtype, True, not rms)
    # row 21 (scale 1e-3, rstd about 1e3) with row 22's rstd (about 1e2): where rstd is large the
    # normalised term outweighs the dh that is added to it
    got, ref, mag, _ = _norm_mutant(inp, rms, {"dx_rstd_from": (21, 22)}, dtype)
    st = R.norm_stats(got, ref, mag)
    assert not st["dx"] <= R.sum_bound(dtype), st


def _partial_rows(N, rpi=4, blocks="all"):
    parts = [p for _, _, p in R.norm_bwd_blocks(N, rpi) if p]
    assert parts, N
    return sum(parts, []) if blocks == "all" else parts[-1]


def test_norm_bwd_blocks_mirror_the_launcher():
    b = R.norm_bwd_blocks(8193)
    assert len(b) == 482 and b[0][:2] == (0, 17) and b[0][2] == [16] and b[-1][:2] == (8177, 8193) and b[-1][2] is None
    b = R.norm_bwd_blocks(67)
    assert [x[:2] for x in b] == [(0, 14), (14, 28), (28, 42), (42, 56), (56, 67)] and b[-1][2] == [64, 65, 66]
    assert R.norm_bwd_blocks(8193, 2)[0][2] == [16] and R.norm_bwd_blocks(1)[0] == (0, 1, [0])


@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("N,H,dtypes", [(67, H, DTYPES) for H in R.NORM_H] + [(5, H, DTYPES) for H in R.NORM_H]
                         + [(8193, 8, [torch.float32]), (8193, 520, [torch.float32])])
def test_mutation_dw_drops_partial_iterations(N, H, dtypes, rms):
    """Every block leaves out its last, partly filled iteration.  At N = 8193 that is one
    row in 17: a random-sign column sum moves by about sqrt(482) / (0.64 * 8193) = 4e-3 of
    its magnitude, over the fp32 bound (5e-4) and under bf16's 4u, so bf16 is not asserted."""
    rows = _partial_rows(N, 2 if H > 2048 else 4)
    for dtype in dtypes:
        inp = R.norm_inputs("flat", N, H, dtype, False, not rms)
        got, ref, mag, _ = _norm_mutant(inp, rms, {"dw_drop_rows": rows}, dtype, use_dh=False)
        st = R.norm_stats(got, ref, mag)
        assert not st["dw"] <= R.acc_bound(dtype, N), st
        if not rms:
            assert not st["db"] <= R.acc_bound(dtype, N), st


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("profile", ["flat", "masked_tail", "ties"])
@pytest.mark.parametrize("V", [v for v in R.SOFTMAX_V if v >= 8])
def test_mutation_lse_drops_a_chunk(V, profile, dtype):
    x, hot = R.logit_inputs(profile, 3, V, dtype)
    lab = R.make_labels(x, hot, kinds=("random",))
    ref, mag = R.ce_reference(x, lab)
    c0 = int(x[1].float().argmax()) // 8 * 8  # the chunk that holds the row's maximum
    bad, _ = R.ce_reference(x, lab, _mut={"lse_drop_chunk": (1, c0)})
    got = dict(lse=bad["lse"].float(), loss=bad["loss"].float(), mean=bad["mean"].float(), dlogits=bad["dlogits"].to(dtype))
    chk = R.ce_check(got, ref, mag, dtype)
    for n in ("lse", "loss"):
        assert not chk[n][0] <= chk[n][1], (n, chk)
    # every probability of the row is off by the factor exp(lse - lse') - 1 = d: the columns off
    # the label show it where d is over the bound (fp32: always; bf16: d over 4u)
    d = abs(torch.exp(ref["lse"][1] - bad["lse"][1]).item() - 1)
    s, b = chk["dlogits_off"]
    # (tied logits round alike, so the output rounding can take up to 2u off d as a whole)
    if dtype == torch.float32 or d > b + 2 * R.U:
        assert not s <= b, (d, chk)
    if d < b - 2 * R.U:
        assert s <= b, (d, chk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [v for v in R.SOFTMAX_V if v >= 2])
def test_mutation_label_column_shifted(V, dtype):
    x, hot = R.logit_inputs("flat", 3, V, dtype)
    lab = R.make_labels(x, hot, kinds=("random",))
    ref, mag = R.ce_reference(x, lab)
    bad, _ = R.ce_reference(x, lab, _mut={"label_shift": 1})
    got = dict(loss=bad["loss"].float(), dlogits=bad["dlogits"].to(dtype))
    chk = R.ce_check(got, ref, mag, dtype)
    assert not chk["loss"][0] <= chk["loss"][1] and not chk["dlogits"][0] <= chk["dlogits"][1], chk


def _int_dout(n_tok, H, seed=0):
    return torch.randint(-8, 9, (n_tok, H), generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_tok", [8193, 8300])
def test_mutation_embedding_drops_rows_past_8192(n_tok, dtype):
    vocab, H = n_tok + 8, 8
    for name, ids in R.id_patterns(n_tok, vocab).items():
        W = torch.zeros(vocab, H, dtype=dtype)
        dout = torch.randn(n_tok, H, generator=torch.Generator().manual_seed(1)).to(dtype)
        pad = 2 if name == "padding" else -1
        ref, mag = R.embedding_reference(ids, W, dout, pad)
        bad, _ = R.embedding_reference(ids, W, dout, pad, _mut={"drop_rows_past": R.EMB_BWD_ROWS})
        if name == "same":  # one row in 8193 of a single sum: under any rounding bound, the exact test's business
            di = _int_dout(n_tok, H).to(dtype)
            assert not torch.equal(R.embedding_reference(ids, W, di, pad)[0]["dW"],
                                   R.embedding_reference(ids, W, di, pad, _mut={"drop_rows_past": 8192})[0]["dW"])
            continue
        nmax = int(torch.bincount(ids).max())
        assert not R.row_stat(bad["dW"].to(dtype), ref["dW"], mag["dW"]) <= R.acc_bound(dtype, nmax), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_mutation_embedding_drops_the_17th_duplicate(dtype):
    """Row 16 (0-based) of the most frequent id, the first of its second group of
    EMB_BWD_U = 16, left out.  One term in 17 or 33 is over every bound; one in 4000 is
    2.5e-4 of the magnitude, at the fp32 bound and far under bf16's: there the exact integer
    comparison (the GPU test's torch.equal) is what sees it."""
    n_tok, H = 8300, 8
    vocab = n_tok + 8
    W = torch.zeros(vocab, H, dtype=dtype)
    dout = torch.randn(n_tok, H, generator=torch.Generator().manual_seed(2)).to(dtype)
    di = _int_dout(n_tok, H).to(dtype).abs() + 1  # no zero term: dropping any row changes the sum
    for name, ids in R.id_patterns(n_tok, vocab).items():
        if not (name.startswith("dup") or name == "same"):
            continue
        mut = {"drop_nth_dup": R.EMB_BWD_U}
        assert not torch.equal(R.embedding_reference(ids, W, di)[0]["dW"], R.embedding_reference(ids, W, di, _mut=mut)[0]["dW"])
        if name in ("dup17", "dup33"):
            ref, mag = R.embedding_reference(ids, W, dout)
            bad, _ = R.embedding_reference(ids, W, dout, _mut=mut)
            n = int(name[3:])
            assert not R.row_stat(bad["dW"].to(dtype), ref["dW"], mag["dW"]) <= R.acc_bound(dtype, n), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.ROPE_D)
@pytest.mark.parametrize("S", R.ROPE_S)
def test_mutation_rotary(S, D, dtype):
    """Pairs (i, i + 1) instead of (i, i + D/2), and sin not negated in the backward: both
    wrong wherever sin != 0, which is every position but 0 (there the rotation is the
    identity for any pairing), so S = 1 cannot show either."""
    cos, sin = R.rope_tables(S, D)
    g = torch.Generator().manual_seed(S + D)
    x, dy = (torch.randn(2, S, 3, D, generator=g).to(dtype) for _ in range(2))
    ref, mag = R.rope_reference(x, cos, sin, False, dy)
    bad, _ = R.rope_reference(x, cos, sin, False, dy, _mut={"adjacent_pairs": True})
    for n in ("y", "dx"):
        assert (R.row_stat(bad[n].to(dtype), ref[n], mag[n]) <= R.sum_bound(dtype)) == (S == 1), n
    bad, _ = R.rope_reference(x, cos, sin, False, dy, _mut={"bwd_same_sign": True})
    st = R.row_stat(bad["dx"].to(dtype), ref["dx"], mag["dx"])
    if S == 1:
        assert st <= R.sum_bound(dtype)
    else:
        assert not st <= R.sum_bound(dtype)


# ------------------------------------------------------------------ 4. what the whole-tensor ratio hides
def test_global_ratio_misses_the_norm_mutations():
    """The three norm mutations, each over its per-row / per-column bound in fp32, pass the
    2e-2 whole-tensor ratio of test_kernels_gpu.py (there: N = 257 rows, loss = sum y^2, so
    dy = 2 y and dw is a sum of same-sign terms)."""
    dtype, H = torch.float32, 1024
    # one row of 67 with a short rstd
    inp = R.norm_inputs("flat", 67, H, dtype)
    got, ref, mag, _ = _norm_mutant(inp, True, {"rstd_short_row": 11}, dtype, use_dh=False)
    assert R.global_rel(got["y"], ref["y"]) < 2e-2 and R.global_rel(got["dx"], ref["dx"]) < 2e-2
    assert _caught(R.norm_stats(got, ref, mag), R.norm_bounds(dtype, 67))
    # one row's dx ten times too large, among rows whose dx is 10^5 times larger still
    inp = R.norm_inputs("mixed_rows", 67, H, dtype, True, False)
    got, ref, mag, _ = _norm_mutant(inp, True, {"dx_rstd_from": (20, 19)}, dtype)
    assert R.global_rel(got["dx"], ref["dx"]) < 2e-2
    assert not R.norm_stats(got, ref, mag)["dx"] <= R.sum_bound(dtype)
    # the last block's partly filled iteration (one row of 257) missing from dw
    N = 257
    inp = R.norm_inputs("flat", N, H, dtype)
    y = R.norm_reference(inp["x"], None, inp["w"], None, None, None, 1e-6, True)[0]["y"]
    inp["dy"] = (2 * y).to(dtype)
    rows = _partial_rows(N, 4, "last")
    assert rows == [256]
    got, ref, mag, _ = _norm_mutant(inp, True, {"dw_drop_rows": rows}, dtype, use_dh=False)
    assert R.global_rel(got["dw"], ref["dw"]) < 2e-2
    assert not R.norm_stats(got, ref, mag)["dw"] <= R.acc_bound(dtype, N)


# ------------------------------------------------------------------ 5. routing of the norm wrappers
def _x(H, dtype=torch.bfloat16, N=3):
    return torch.zeros(N, H, dtype=dtype)


def test_norm_kernel_ok_refuses(monkeypatch):
    monkeypatch.setattr(F, "_on_gpu", lambda t: True)  # CPU tensors standing in for device ones
    bf, f32 = torch.bfloat16, torch.float32
    ok = F.norm_kernel_ok
    assert ok(_x(1024), torch.ones(1024, dtype=bf)) and ok(_x(8, f32), torch.ones(8, dtype=f32), torch.ones(8, dtype=f32))
    assert ok(_x(8192), torch.ones(8192, dtype=bf), None, _x(8192))
    assert not ok(_x(1004), torch.ones(1004, dtype=bf))                      # H % 8
    assert not ok(_x(4), torch.ones(4, dtype=bf))
    assert not ok(_x(8200), torch.ones(8200, dtype=bf))                      # H > 8192
    assert not ok(_x(1024), torch.ones(1024, dtype=f32))                     # weight of another dtype
    assert not ok(_x(1024), torch.ones(1024, dtype=bf), torch.ones(1024, dtype=f32))   # bias of another dtype
    assert not ok(_x(1024, f32), torch.ones(1024, dtype=f32), torch.ones(1024, dtype=bf))
    assert not ok(_x(1024), torch.ones(1024, dtype=bf), None, _x(1024, f32))  # residual of another dtype
    assert not ok(_x(1024, torch.float16), torch.ones(1024, dtype=torch.float16))
    assert not ok(_x(1024, f64), torch.ones(1024, dtype=f64))
    assert not ok(_x(1024), None)
    assert not ok(_x(1024, N=0), torch.ones(1024, dtype=bf))
    assert not ok(_x(1024), torch.ones(512, dtype=bf))                       # weight of another length
    monkeypatch.setattr(F, "_on_gpu", lambda t: False)
    assert not ok(_x(1024), torch.ones(1024, dtype=bf))


@pytest.mark.parametrize("verdict", [True, False])
def test_rms_norm_and_layer_norm_consult_the_predicate(monkeypatch, verdict):
    asked, ran = [], []
    monkeypatch.setattr(F, "norm_kernel_ok", lambda x, w, b=None, res=None: asked.append((x, w, b, res)) or verdict)

    def fake_apply(fn, *args):
        ran.append(fn)
        return args[0], args[0]

    monkeypatch.setattr(F._tape, "apply", fake_apply)
    x, r = _x(16), _x(16)
    w, b = torch.ones(16, dtype=torch.bfloat16), torch.zeros(16, dtype=torch.bfloat16)
    F.rms_norm(x, w, 1e-6, residual=r)
    F.layer_norm(x, w, b, 1e-5, residual=r)
    assert len(asked) == 2 and asked[0][0] is x and asked[0][1] is w and asked[0][3] is r
    assert asked[1][1] is w and asked[1][2] is b and asked[1][3] is r
    assert ran == [F._NormFn if verdict else F._NormRefFn] * 2


def test_refused_shapes_run_the_reference_path():
    # H % 8 != 0 on the host: _NormRefFn end to end, against the oracle
    inp = R.norm_inputs("flat", 5, 1004, torch.float32, True, False)
    x, r, w = (inp[k].clone().requires_grad_() for k in ("x", "res", "w"))
    y, h = F.rms_norm(x, w, 1e-6, residual=r)
    torch.autograd.backward([y, h], [inp["dy"], inp["dh"]])
    ref, mag = R.norm_case_reference(inp, True, True)
    st = R.norm_stats(dict(y=y, h=h, dx=x.grad, dres=r.grad, dw=w.grad), ref, mag)
    assert not _caught(st, R.norm_bounds(torch.float32, 5)), st


def test_swiglu_refuses_an_odd_last_dimension():
    with pytest.raises(ValueError):
        F.swiglu(torch.zeros(4, 17))
    assert F.swiglu(torch.zeros(4, 24)).shape == (4, 12)
