"""Per-row float64 oracle for the attention kernels (CPU only, plain torch).

``reference`` is attention and its analytic backward in float64 on [B, S, H, D]
tensors (GQA, causal with Sq != Sk, optional neox rotary), with rows that have no key
*defined* (O = 0, LSE = -inf, dQ = 0, nothing added to dK / dV) instead of NaN.  Next
to every result it returns a **magnitude** tensor: the same sum with every term replaced
by its absolute value (magO = P |V|, ...).  ``row_stat`` divides the 2-norm of a row's
error by the 2-norm of that row's magnitude: the backward-error form
|fl(sum x) - sum x| <= gamma * sum |x|, which does not depend on how much the sum
cancels (sum_j dS_ij = 0) and so needs no per-case tuning.  A fully wrong row scores
about 1; one wrong element of a D = 128 row about 0.09.

One caveat, for dQ only: the profiles below put c_j / sqrt(scale) into k[..., 0], and
magdQ = scale * dSmag |K| then carries most of a row's norm in element 0.  An error in
the other elements of a dQ row is weighed lighter by |magdQ row| / |magdQ row without
element 0|, measured over the path shapes and scales at D = 128 as (median, max):
flat 1.0 / 1.0, ramp_slow 1.8 / 8.7, ramp_fast 4.0 / 23, spike 5.5 / 20, offset 22 / 43
(D = 64: up to 50).  So only ``flat`` watches dQ at the sensitivity quoted above; every
test runs it at the same shapes.  O, dK, dV and LSE are not affected.

``emulated`` is the same computation in float32 with a bf16 rounding wherever a kernel
rounds (P, dS, the O that feeds delta, every output).  It is the yardstick the bound
8u (u = 2^-9, bf16 unit roundoff) is checked against on the CPU, never an expected value.

The input makers return seeded bf16 q, k, v, do whose scaled scores are
``noise + t_i * c_j``: t_i is drawn per query row from {1, -1, 0, 0.4} (rows of one
32-row wave need different rescales) and c_j follows a key profile (``PROFILES``) that
drives the online softmax through its rescale, lazy-rescale, spike and large-offset
regimes.

Worst statistics measured on the MI355X (tests/test_attention_oracle_gpu.py, bound
8u = 1.5625e-2 for O / dQ / dK / dV, 1e-4 for LSE):

    path                           O        dQ       dK       dV       LSE       asserted through
    bwd v0<128>                    -        7.01e-4  8.83e-4  3.59e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v0<256>                    -        3.69e-4  6.74e-4  3.86e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v0<64>                     -        8.29e-4  1.28e-3  3.79e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v1<128>                    -        7.01e-4  8.83e-4  3.59e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v1<64>                     -        8.29e-4  1.28e-3  3.79e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v3<128>                    -        7.01e-4  8.83e-4  3.59e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v4<128>                    -        7.01e-4  8.83e-4  3.59e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    bwd v5<128>                    -        5.39e-4  8.90e-4  3.77e-3  -         pa_flash_attn_bwd + pa_fa_bwd_last
    decode<128>                    1.85e-3  -        -        -        -         pa_attn_decode
    decode<64>                     1.60e-3  -        -        -        -         pa_attn_decode
    flash_attention_varlen         3.20e-3  5.97e-4  6.11e-4  3.88e-3  -         pa_fa_fwd_last + pa_fa_bwd_last (x 3)
    fwd1<128>                      3.54e-3  -        -        -        3.17e-7   pa_fa_fwd_last
    fwd1<256>                      3.44e-3  -        -        -        5.47e-7   pa_fa_fwd_last
    fwd1<64>                       3.41e-3  -        -        -        2.79e-7   pa_fa_fwd_last
    fwd2<128> + split bwd          4.35e-3  1.25e-3  1.49e-3  4.56e-3  5.00e-7   pa_fa_fwd_last + pa_fa_bwd_split
    packed_attention, split off    3.54e-3  5.82e-4  8.83e-4  4.14e-3  3.32e-7   pa_fa_bwd_last + pa_fa_dq_reduce_rope
    packed_attention, split on     3.54e-3  5.86e-4  1.22e-3  4.14e-3  3.32e-7   pa_fa_bwd_split
    packed_attention, v5           3.23e-3  5.39e-4  8.90e-4  3.85e-3  3.62e-7   pa_fa_bwd_last + pa_fa_dq_reduce_rope
    poisoned, fwd1 + v4/v1         1.91e-3  3.17e-4  5.02e-4  3.12e-3  1.99e-7   pa_fa_fwd_last + pa_fa_bwd_last
    poisoned, fwd2 + split         1.91e-3  3.36e-4  4.21e-4  3.29e-3  1.99e-7   pa_fa_fwd_last + pa_fa_bwd_split
    poisoned, v0                   1.91e-3  3.16e-4  5.02e-4  3.12e-3  1.99e-7   pa_fa_fwd_last + pa_fa_bwd_last
    qkv_rope_attention, split off  4.21e-3  7.71e-4  1.17e-3  3.93e-3  4.37e-7   EPI_ROPE + pa_fa_dq_reduce_rope
    qkv_rope_attention, split on   4.21e-3  7.70e-4  1.01e-3  3.93e-3  4.37e-7   EPI_ROPE + pa_fa_bwd_split
    qkv_rope_attention, v5         3.02e-3  7.71e-4  1.17e-3  3.53e-3  3.90e-7   pa_fa_bwd_last + pa_fa_dq_reduce_rope
    rope_attention, split off      3.91e-3  7.30e-4  1.02e-3  3.90e-3  3.53e-7   pa_fa_dq_reduce_rope (+ pa_fa_gqa_fold)
    rope_attention, split on       3.91e-3  7.31e-4  8.98e-4  3.90e-3  3.53e-7   pa_fa_bwd_split
    rope_attention, v5             2.70e-3  5.37e-4  9.86e-4  3.41e-3  4.02e-7   pa_fa_bwd_last + pa_fa_dq_reduce_rope
    split bwd + rotary             3.54e-3  4.64e-4  8.08e-4  3.64e-3  3.06e-7   pa_fa_bwd_split

(Every "split off" row also asserts pa_fa_bwd_last.  fwd1 / fwd2 = fa_fwd_kernel /
fa_fwd_kernel2, "bwd vN<D>" = single-kernel backward variant N with the split path off,
"poisoned" = inputs bordered by NaN and outputs by a sentinel.  The CPU emulation of the
same cases stays under 4.3e-3.)
"""
import math

import torch

U = 2.0 ** -9          # bf16 unit roundoff
BOUND = 8 * U          # GPU bound on row_stat for O, dQ, dK, dV
EMU_BOUND = 4 * U      # what the fp32 / bf16 emulation must meet on the CPU
LSE_TOL = 1e-4

PROFILES = ("flat", "ramp_fast", "ramp_slow", "spike", "offset")
T_VALUES = (1.0, -1.0, 0.0, 0.4)

# (Sq, Sk): straddle 128 query rows per workgroup / 32 per wave, 64-key forward tiles,
# 32-key dQ tiles, 64-query dK/dV slices, 128 keys per backward workgroup
SHAPES = [(1, 1), (1, 129), (33, 1), (31, 65), (64, 64), (65, 257), (129, 129), (193, 127), (128, 256), (257, 257)]
NONCAUSAL_ONLY = {(193, 127)}
EMPTY_SHAPES = [(130, 66), (200, 8)]  # causal only: Sq - Sk leading query rows see no key
HEADS = [(2, 2), (4, 1), (8, 2)]
SCALE_FACTORS = (1.0, 0.3, 1.7)  # times 1 / sqrt(D)


def shape_cases():
    """Every (Sq, Sk, causal) of the full matrix."""
    out = []
    for sq, sk in SHAPES:
        out.append((sq, sk, False))
        if (sq, sk) not in NONCAUSAL_ONLY:
            out.append((sq, sk, True))
    return out + [(sq, sk, True) for sq, sk in EMPTY_SHAPES]


# the three shapes every non-default path runs (all profiles), plus the empty-row shape
PATH_SHAPES = [(65, 257, True), (193, 127, False), (257, 257, True)]
EMPTY_CASE = (130, 66, True)


def path_cases(D, Sq):
    """(profile, Hq, Hk, scale) of the five cases a non-default path runs at one shape:
    every profile, the head configurations and scale factors rotating through them."""
    return [(p, *HEADS[i % 3], SCALE_FACTORS[(i + Sq) % 3] / math.sqrt(D)) for i, p in enumerate(PROFILES)]


_CACHE = {}


def case(profile, B, Sq, Sk, Hq, Hk, D, scale, causal, seed=0):
    """(inputs, reference) of one case, computed once and shared between the tests that
    run different kernels on it.  Treat both as read-only."""
    key = (profile, B, Sq, Sk, Hq, Hk, D, round(scale, 9), causal, seed)
    if key not in _CACHE:
        inp = make_inputs(profile, B, Sq, Sk, Hq, Hk, D, scale, seed)
        _CACHE[key] = (inp, reference(*inp, causal, scale))
    return _CACHE[key]


def key_profile(profile, Sk):
    j = torch.arange(Sk, dtype=torch.float64)
    if profile == "flat":
        return torch.zeros(Sk, dtype=torch.float64)
    if profile == "ramp_fast":   # a rescale on every 64-key forward tile
        return 12 * math.log(2) * j / 64
    if profile == "ramp_slow":   # under the 2^8 laziness threshold for a tile, then across it
        return 5 * math.log(2) * j / 64
    if profile == "spike":
        c = torch.zeros(Sk, dtype=torch.float64)
        for s in (0, 63, 64, Sk - 1):
            if 0 <= s < Sk:
                c[s] = 30.0
        return c
    if profile == "offset":
        return torch.full((Sk,), 60.0, dtype=torch.float64)
    raise ValueError(profile)


def make_inputs(profile, B, Sq, Sk, Hq, Hk, D, scale, seed=0, return_t=False):
    """bf16 q [B, Sq, Hq, D], k / v [B, Sk, Hk, D], do [B, Sq, Hq, D] on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Sq + 13 * Sk + Hq + D + PROFILES.index(profile))
    q = torch.randn(B, Sq, Hq, D, generator=g, dtype=torch.float64)
    k = torch.randn(B, Sk, Hk, D, generator=g, dtype=torch.float64)
    v = torch.randn(B, Sk, Hk, D, generator=g, dtype=torch.float64)
    do = torch.randn(B, Sq, Hq, D, generator=g, dtype=torch.float64)
    t = torch.tensor(T_VALUES, dtype=torch.float64)[torch.randint(0, 4, (B, Sq, Hq), generator=g)]
    rs = math.sqrt(scale)
    q[..., 0] = t / rs
    k[..., 0] = (key_profile(profile, Sk) / rs).view(1, Sk, 1)
    out = tuple(x.to(torch.bfloat16) for x in (q, k, v, do))
    return out + (t,) if return_t else out


def rotate(x, cos, sin, sign=1.0):
    """neox rotation of x [B, S, H, D] at positions 0..S-1, in x's dtype."""
    S, D = x.shape[1], x.shape[-1]
    c = cos[:S].to(x.dtype).view(1, S, 1, D // 2)
    s = sin[:S].to(x.dtype).view(1, S, 1, D // 2) * sign
    a, b = x[..., : D // 2], x[..., D // 2:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def allowed(Sq, Sk, causal, shift=0):
    """[Sq, Sk] bool: key j visible to query i (causal: j <= i + Sk - Sq)."""
    if not causal:
        return torch.ones(Sq, Sk, dtype=torch.bool)
    i = torch.arange(Sq).view(Sq, 1)
    j = torch.arange(Sk).view(1, Sk)
    return j <= i + (Sk - Sq) + shift


def _expand(x, Hq, head_map):
    Hk = x.shape[2]
    if head_map == "group":
        idx = torch.arange(Hq) // (Hq // Hk)
    else:  # the wrong map, for the mutation test
        idx = torch.arange(Hq) % Hk
    return x[:, :, idx], idx


def _fold(x_e, idx, Hk):
    out = torch.zeros(x_e.shape[0], x_e.shape[1], Hk, x_e.shape[3], dtype=x_e.dtype)
    return out.index_add_(2, idx, x_e)


def _attention(q, k, v, do, causal, scale, cos, sin, dtype, rnd, mags, mask_shift=0, head_map="group"):
    q, k, v, do = (x.detach().cpu().to(dtype) for x in (q, k, v, do))
    B, Sq, Hq, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    if cos is not None:
        cos, sin = cos.detach().cpu(), sin.detach().cpu()
        q, k = rotate(q, cos, sin), rotate(k, cos, sin)
    ke, idx = _expand(k, Hq, head_map)
    ve, _ = _expand(v, Hq, head_map)
    ok = allowed(Sq, Sk, causal, mask_shift).view(1, 1, Sq, Sk)
    s = torch.einsum("bqhd,bkhd->bhqk", q, ke) * scale
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = m == float("-inf")
    e = torch.exp(s - torch.where(empty, torch.zeros_like(m), m))  # empty rows: exp(-inf) = 0
    l = e.sum(-1, keepdim=True)
    lsafe = torch.where(empty, torch.ones_like(l), l)
    lse = torch.where(empty, m, m + torch.log(lsafe)).squeeze(-1)  # [B, Hq, Sq]
    # forward: a kernel rounds the unnormalised exp to bf16 and divides by the fp32 sum
    o = torch.einsum("bhqk,bkhd->bqhd", rnd(e), ve) / lsafe.squeeze(-1).transpose(1, 2).unsqueeze(-1)
    p = e / lsafe
    o_in = rnd(o)  # the stored O feeds delta
    delta = (do * o_in).sum(-1).transpose(1, 2).unsqueeze(-1)  # [B, Hq, Sq, 1]
    dp = torch.einsum("bqhd,bkhd->bhqk", do, ve)
    ds = rnd(p * (dp - delta))
    pr = rnd(p)
    dq = scale * torch.einsum("bhqk,bkhd->bqhd", ds, ke)
    dk = _fold(scale * torch.einsum("bhqk,bqhd->bkhd", ds, q), idx, Hk)
    dv = _fold(torch.einsum("bhqk,bqhd->bkhd", pr, do), idx, Hk)
    res = {}
    if mags:
        # magnitudes before the inverse rotation: it preserves the row 2-norm of an error
        ao, ado = o.abs(), do.abs()
        dsm = p * (torch.einsum("bqhd,bkhd->bhqk", ado, ve.abs())
                   + (ado * ao).sum(-1).transpose(1, 2).unsqueeze(-1))
        res["magO"] = torch.einsum("bhqk,bkhd->bqhd", p, ve.abs())
        res["magdQ"] = scale * torch.einsum("bhqk,bkhd->bqhd", dsm, ke.abs())
        res["magdK"] = _fold(scale * torch.einsum("bhqk,bqhd->bkhd", dsm, q.abs()), idx, Hk)
        res["magdV"] = _fold(torch.einsum("bhqk,bqhd->bkhd", p, ado), idx, Hk)
    if cos is not None:
        dq, dk = rotate(dq, cos, sin, -1.0), rotate(dk, cos, sin, -1.0)
    res.update(O=rnd(o), LSE=lse, dQ=rnd(dq), dK=rnd(dk), dV=rnd(dv))
    return res


def reference(q, k, v, do, causal, scale, cos=None, sin=None, _mask_shift=0, _head_map="group"):
    """float64 attention forward + backward.  Returns a dict: O, dQ [B, Sq, Hq, D],
    dK, dV [B, Sk, Hk, D], LSE [B, Hq, Sq] and magO / magdQ / magdK / magdV.
    (The underscore arguments build deliberately wrong results for the mutation tests.)"""
    return _attention(q, k, v, do, causal, scale, cos, sin, torch.float64, lambda x: x, True,
                      _mask_shift, _head_map)


def _bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def emulated(q, k, v, do, causal, scale, cos=None, sin=None):
    """The kernels' arithmetic model: fp32 with bf16 roundings of P, dS, O and the outputs."""
    return _attention(q, k, v, do, causal, scale, cos, sin, torch.float32, _bf16_round, False)


def row_stat(got, ref, mag):
    """max over (b, s, h) rows of |got - ref|_2 / (|mag|_2 + 1e-6 max_rows |mag|_2);
    inf when ``got`` holds a non-finite value."""
    got, ref, mag = (x.detach().cpu().double() for x in (got, ref, mag))
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    num = (got - ref).norm(dim=-1)
    mn = mag.norm(dim=-1)
    den = mn + 1e-6 * mn.max()
    stat = torch.where(num == 0, torch.zeros_like(num), num / den)  # 0 / 0 (nothing anywhere) is no error
    return stat.max().item()


def lse_stat(got, ref):
    """max |got - ref| / max(1, |ref|) over rows with a key; inf unless the rows without
    one are exactly -inf and everything else is finite."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    empty = ref == float("-inf")
    if not (got[empty] == float("-inf")).all() or not torch.isfinite(got[~empty]).all():
        return float("inf")
    if (~empty).sum() == 0:
        return 0.0
    d = (got[~empty] - ref[~empty]).abs() / ref[~empty].abs().clamp_min(1.0)
    return d.max().item()


def stats(got, ref):
    """row_stat of every gradient / output present in ``got`` (a dict with the keys of
    ``reference``), lse_stat for LSE."""
    out = {}
    for n in ("O", "dQ", "dK", "dV"):
        if n in got:
            out[n] = row_stat(got[n], ref[n], ref["mag" + n])
    if "LSE" in got:
        out["LSE"] = lse_stat(got["LSE"], ref["LSE"])
    return out
