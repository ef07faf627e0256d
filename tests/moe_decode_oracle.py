"""float64 oracle of ``ops.moe_decode_route`` / ``ops.moe_decode_ffn`` (helper, no tests).

Inputs come from a seeded ``torch.Generator``: ``x ~ N(0, 1)``, expert weights ``0.05 N(0, 1)`` in
bf16, ``gate_w`` ``0.05 N(0, 1)`` in fp32.

Reference: ``ref_t = sum_j w_tj (a_j . down_e)`` in float64 with unrounded ``a``.  Per-element
bound, in the form of ``test_skinny_gemm_gpu.check_bound``:

    2^-8 |ref| + 2 sum_j w_j (da_j . |down_e|) + I 2^-22 mag_y
    da = 2^-9 |a| + H 2^-22 (1.1 |u| mag_g + |silu(g)| mag_u)

``mag_*`` are the products of absolute values.  The terms: one rounding of ``a`` to bf16, the
first-order fp32 accumulation error of both products (|d silu / dg| <= 1.1), one output rounding.

Router decisions are compared only under a margin: the float64 gap between the k-th and the
(k+1)-th logit must exceed ``2 H 2^-23 max_e(|x| . |gate_w|)`` (twice the first-order fp32
accumulation error of one logit).  With the recipe above every row of every case the tests use
meets it; the tests assert that first and leave out no row.
"""
import torch

BF16 = torch.bfloat16
CASES = [(16, 256, 128, 8, 2), (16, 264, 136, 64, 6), (5, 640, 384, 64, 6)]  # (M, H, I, E, k)


def make_inputs(M, H, I, E, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=g).to(BF16)
    gate_up = (0.05 * torch.randn(E, H, 2 * I, generator=g)).to(BF16)
    down = (0.05 * torch.randn(E, I, H, generator=g)).to(BF16)
    gate_w = 0.05 * torch.randn(H, E, generator=g)
    return tuple(t.to(device) for t in (x, gate_w, gate_up, down))


def route_oracle(x, gate_w, k, renorm=True):
    """-> (idx [M, k] int64, w [M, k] float64, gap [M], need [M]); a row's decision is comparable
    when gap > need (k == E: gap is inf)."""
    xd, gd = x.double().cpu(), gate_w.double().cpu()
    H, E = gd.shape
    logits = xd @ gd
    sl, si = torch.sort(logits, dim=-1, descending=True, stable=True)
    idx, sel = si[:, :k], sl[:, :k]
    w = torch.softmax(sel, -1) if renorm else torch.softmax(logits, -1).gather(1, idx)
    gap = sl[:, k - 1] - sl[:, k] if k < E else torch.full((xd.shape[0],), float("inf"), dtype=torch.float64)
    need = 2.0 * H * 2.0 ** -23 * (xd.abs() @ gd.abs()).max(-1).values
    return idx, w, gap, need


def ffn_oracle(x, gate_up, down, idx, w):
    """-> (ref [M, H], bound [M, H]) in float64 for the routing (idx, w)."""
    xd = x.double().cpu()
    M, H = xd.shape
    I = down.shape[1]
    ref = torch.zeros(M, H, dtype=torch.float64)
    t2 = torch.zeros(M, H, dtype=torch.float64)
    mag_y = torch.zeros(M, H, dtype=torch.float64)
    for t in range(M):
        for j in range(idx.shape[1]):
            e = int(idx[t, j])
            gu, dn = gate_up[e].double().cpu(), down[e].double().cpu()
            h = xd[t] @ gu
            mag = xd[t].abs() @ gu.abs()
            g, u = h[:I], h[I:]
            silu = g * torch.sigmoid(g)
            a = silu * u
            da = 2.0 ** -9 * a.abs() + H * 2.0 ** -22 * (1.1 * u.abs() * mag[:I] + silu.abs() * mag[I:])
            wj = float(w[t, j])
            ref[t] += wj * (a @ dn)
            t2[t] += wj * (da @ dn.abs())
            mag_y[t] += wj * (a.abs() @ dn.abs())
    bound = 2.0 ** -8 * ref.abs() + 2.0 * t2 + I * 2.0 ** -22 * mag_y
    return ref, bound


def check_bound(got, ref, bound, what):
    got = got.double().cpu()
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err/bound {worst:.3f}")
    assert torch.isfinite(got).all(), what
    assert (err <= bound).all(), f"{what}: err/bound {worst:.3f}"
    return worst
