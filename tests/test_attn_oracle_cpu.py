"""The attention oracle (tests/attn_oracle.py) checks itself: the float64 reference
against torch autograd, the bound against an fp32 / bf16 emulation of the kernels on
every case of the GPU matrix, and the statistic against the bugs it is there to catch."""
import math

import pytest
import torch

import attn_oracle as AO


def _naive(q, k, v, causal, scale):
    B, Sq, Hq, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    ke, ve = k.repeat_interleave(Hq // Hk, 2), v.repeat_interleave(Hq // Hk, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, ke) * scale
    s = s.masked_fill(~AO.allowed(Sq, Sk, causal), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), ve), torch.logsumexp(s, -1)


def _tables(S, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    return f.cos(), f.sin()


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("profile", AO.PROFILES)
@pytest.mark.parametrize("Sq,Sk,causal,Hq,Hk", [(31, 65, True, 4, 1), (65, 70, False, 2, 2), (70, 70, True, 8, 2)])
def test_reference_matches_autograd(Sq, Sk, causal, Hq, Hk, profile, rotary):
    D, scale = 64, 1.7 / 8
    q, k, v, do = AO.make_inputs(profile, 2, Sq, Sk, Hq, Hk, D, scale, seed=1)
    cos, sin = _tables(max(Sq, Sk), D) if rotary else (None, None)
    ref = AO.reference(q, k, v, do, causal, scale, cos, sin)
    qa, ka, va = (x.double().requires_grad_() for x in (q, k, v))
    qr, kr = (AO.rotate(qa, cos, sin), AO.rotate(ka, cos, sin)) if rotary else (qa, ka)
    o, lse = _naive(qr, kr, va, causal, scale)
    o.backward(do.double())
    for n, a in (("O", o), ("LSE", lse), ("dQ", qa.grad), ("dK", ka.grad), ("dV", va.grad)):
        err = ((ref[n] - a.detach()).abs().max() / a.detach().abs().max()).item()
        assert err < 1e-10, (n, err)
    for n in ("O", "dQ", "dK", "dV"):
        # |sum x| <= sum |x|, per row norm (the inverse rotation keeps the norm of a row)
        assert (ref["mag" + n].norm(dim=-1) >= ref[n].norm(dim=-1) * (1 - 1e-12)).all(), n


def _feasibility_cases():
    out = [(128, sq, sk, c) for sq, sk, c in AO.shape_cases()]
    for D in (64, 256):
        out += [(D, sq, sk, c) for sq, sk, c in AO.PATH_SHAPES + [AO.EMPTY_CASE]]
    return out


@pytest.mark.parametrize("D,Sq,Sk,causal", _feasibility_cases())
def test_bound_is_feasible(D, Sq, Sk, causal):
    """The reference is finite and the fp32 / bf16 model of the kernels stays within 4u
    on every case of the GPU matrix: the 8u asked of the kernels is attainable."""
    worst = {}
    for profile, Hq, Hk, scale in AO.path_cases(D, Sq):
        q, k, v, do = AO.make_inputs(profile, 2, Sq, Sk, Hq, Hk, D, scale)
        ref = AO.reference(q, k, v, do, causal, scale)
        for n, t in ref.items():
            if n == "LSE":
                assert not torch.isnan(t).any() and (t < float("inf")).all()
                assert (t == float("-inf")).sum() == 2 * Hq * (max(0, Sq - Sk) if causal else 0)
            else:
                assert torch.isfinite(t).all(), n
        emu = AO.emulated(q, k, v, do, causal, scale)
        for n, s in AO.stats(emu, ref).items():
            worst[n] = max(worst.get(n, 0.0), s)
            assert s <= (AO.LSE_TOL if n == "LSE" else AO.EMU_BOUND), (profile, n, s)
    print("emulated worst", {n: f"{s:.2e}" for n, s in worst.items()})


def _case(profile="ramp_fast", Sq=65, Sk=257, causal=True, Hq=4, Hk=2, D=128, f=1.0):
    scale = f / math.sqrt(D)
    q, k, v, do, t = AO.make_inputs(profile, 2, Sq, Sk, Hq, Hk, D, scale, return_t=True)
    return (q, k, v, do), t, scale, AO.reference(q, k, v, do, causal, scale)


# The profiles with a large c_j put c_j / sqrt(scale) into k[..., 0], so element 0 carries
# most of a dQ row's magnitude there and an error in the other elements weighs less: the
# flat profile (same shapes, k[..., 0] = 0) is the one that watches dQ at full sensitivity.
@pytest.mark.parametrize("profile,names", [("flat", ("O", "dQ", "dK", "dV")), ("ramp_fast", ("O", "dK", "dV"))])
def test_mutation_row_swapped_with_neighbour(profile, names):
    _, _, _, ref = _case(profile=profile)
    for n in names:
        got = ref[n].clone()
        got[1, 40, 1] = ref[n][1, 41, 1]
        assert AO.row_stat(got, ref[n], ref["mag" + n]) > AO.BOUND, n
        assert AO.row_stat(ref[n], ref[n], ref["mag" + n]) == 0.0


def test_mutation_first_key_tile_dropped():
    """A t = -1 row of ramp_fast has its maximum in the first 64-key tile; a kernel that
    loses that tile (a rescale gone wrong) is caught on O."""
    (q, k, v, do), t, scale, ref = _case(causal=False)
    rows = (t == -1.0).nonzero()
    assert len(rows)
    b, i, h = rows[0].tolist()
    tail = AO.reference(q, k[:, 64:], v[:, 64:], do, False, scale)
    got = ref["O"].clone()
    got[b, i, h] = tail["O"][b, i, h]
    assert AO.row_stat(got, ref["O"], ref["magO"]) > AO.BOUND


@pytest.mark.parametrize("profile,names", [("flat", ("O", "dQ", "dK", "dV")), ("ramp_fast", ("O", "dK", "dV"))])
def test_mutation_causal_mask_off_by_one(profile, names):
    (q, k, v, do), _, scale, ref = _case(profile=profile)
    bad = AO.reference(q, k, v, do, True, scale, _mask_shift=1)
    for n, s in AO.stats({n: bad[n] for n in names}, ref).items():
        assert s > AO.BOUND, (n, s)
    assert AO.lse_stat(bad["LSE"], ref["LSE"]) > AO.LSE_TOL


def test_mutation_wrong_gqa_head_map():
    (q, k, v, do), _, scale, ref = _case(profile="flat", Hq=4, Hk=2)
    bad = AO.reference(q, k, v, do, True, scale, _head_map="mod")
    for n, s in AO.stats({n: bad[n] for n in ("O", "dQ", "dK", "dV")}, ref).items():
        assert s > AO.BOUND, (n, s)


@pytest.mark.parametrize("f", [0.3, 1.0, 1.7])
def test_mutation_scale_left_out_of_dk(f):
    _, _, scale, ref = _case(profile="flat", f=f)
    assert AO.row_stat(ref["dK"] / scale, ref["dK"], ref["magdK"]) > AO.BOUND


def test_mutation_nan_on_empty_row():
    _, _, _, ref = _case(profile="flat", Sq=130, Sk=66)
    assert (ref["LSE"][:, :, :64] == float("-inf")).all() and torch.isfinite(ref["LSE"][:, :, 64:]).all()
    assert not ref["O"][:, :64].any() and not ref["dQ"][:, :64].any()
    for n in ("O", "dQ"):
        got = ref[n].clone()
        got[0, 3, 1, 5] = float("nan")
        assert AO.row_stat(got, ref[n], ref["mag" + n]) > AO.BOUND
        got[0, 3, 1, 5] = 1e-3  # any value at all on a row that must be zero
        assert AO.row_stat(got, ref[n], ref["mag" + n]) > AO.BOUND
    lse = ref["LSE"].clone()
    lse[0, 1, 3] = -1e30
    assert AO.lse_stat(lse, ref["LSE"]) == float("inf")


def test_global_ratio_misses_a_wrong_row():
    """On record: at (B, S, Hq) = (2, 2048, 5) the per-tensor Frobenius ratio the older
    attention tests assert (< 2e-2) accepts a row that is entirely wrong."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(2, 2048, 5, 128, generator=g, dtype=torch.float64)
    got = ref.clone()
    got[1, 1000, 2] = ref[1, 1001, 2]
    rel = ((got - ref).norm() / ref.norm()).item()
    assert rel < 2e-2, rel
    assert AO.row_stat(got, ref, ref.abs()) > 50 * AO.BOUND


@pytest.mark.parametrize("scale", [0.0, -0.125, float("nan")])
def test_nonpositive_scale_is_refused(scale):
    """The kernels take the max over raw scores, which is only right for scale > 0: the
    entry points refuse anything else before they look at the device."""
    from paddle_amd import ops

    q = torch.randn(1, 1, 2, 64)
    kv = torch.randn(1, 5, 2, 64)
    with pytest.raises(ValueError, match="scale"):
        ops.flash_attention(q, kv, kv, causal=False, scale=scale)
    with pytest.raises(ValueError, match="scale"):
        ops.flash_attention_varlen(q[0], kv[0], kv[0], [0, 1], [0, 5], causal=False, scale=scale)
    cache = ops.KVCache(1, 1, 8, 2, 64, torch.float32)
    with pytest.raises(ValueError, match="scale"):
        ops.decode_attention(q, cache, 0, scale=scale)
    # a positive scale still runs (CPU reference path)
    assert ops.flash_attention(q, kv, kv, causal=False, scale=0.3).shape == q.shape
