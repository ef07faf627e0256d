"""The two reductions of the LLaMA training step that used float atomics, the
embedding weight gradient (``pa_embedding_bwd``) and the global-norm sum of squares
(``pa_sumsq``), add in a fixed order: two launches on the same data give the same
bits, which is what makes two runs of ``bench.py`` comparable output for output.
Values are checked against float64 with the bound of a recursive fp32 sum of n
terms, (n - 1) * 2^-24 * sum|x|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _emb_bwd(ids, d, dW, pad=-1):
    from paddle_amd.ops import _native as N

    N.call("pa_embedding_bwd", N.dt(d), N.ptr(ids), N.ptr(d), N.ptr(dW), ids.numel(), d.shape[1], pad, N.stream())
    return dW


# one launch covers 8192 rows; a block covers 4096 columns per pass and sums 16 rows at a
# time; a width that is no multiple of 4 takes the scalar path
@pytest.mark.parametrize("rows,H", [(1, 264), (63, 264), (8192, 264), (8192 + 777, 264), (200, 4096 + 264),
                                    (300, 262)])
def test_embedding_bwd_repeated_ids_same_bits(rows, H):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(rows)
    V, pad = 37, 5  # few ids: every dW row sums many token rows, across the range boundary too
    ids = torch.randint(0, V, (rows,), generator=g).to(dev)
    d = torch.randn(rows, H, generator=g).to(dev)
    base = torch.randn(V, H, generator=g).to(dev)  # the accumulator already holds a gradient
    a = _emb_bwd(ids, d, base.clone(), pad)
    b = _emb_bwd(ids, d, base.clone(), pad)
    assert torch.equal(a, b)
    keep = ids != pad
    ref = base.double().index_add_(0, ids[keep], d[keep].double())
    mag = base.double().abs().index_add_(0, ids[keep], d[keep].double().abs())
    n = torch.bincount(ids[keep], minlength=V).double().unsqueeze(1)  # terms added to the held value
    assert bool(((a.double() - ref).abs() <= n * U * mag).all())
    assert torch.equal(a[pad], base[pad])


def test_embedding_bwd_bf16_gradient():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 11, (300,), generator=g).to(dev)
    d = torch.randn(300, 512, generator=g).to(dev).bfloat16()
    a = _emb_bwd(ids, d, torch.zeros(11, 512, device=dev))
    b = _emb_bwd(ids, d, torch.zeros(11, 512, device=dev))
    assert torch.equal(a, b)
    ref = torch.zeros(11, 512, dtype=torch.float64, device=dev).index_add_(0, ids, d.double())
    mag = torch.zeros(11, 512, dtype=torch.float64, device=dev).index_add_(0, ids, d.double().abs())
    n = torch.bincount(ids, minlength=11).double().unsqueeze(1)
    assert bool(((a.double() - ref).abs() <= n * U * mag).all())


@pytest.mark.parametrize("n", [5, 2048 * 8 + 3, (1 << 22) + 13])  # one block; tail; the full 2048-block grid
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sumsq_same_bits(n, dtype):
    from paddle_amd.ops import optim

    dev = torch.device("cuda", 0)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev).to(dtype)
    a = optim.sumsq(x)
    b = optim.sumsq(x)
    assert torch.equal(a, b)
    ref = x.double().pow(2).sum().item()
    # longest chain of fp32 roundings behind the result: a thread's own terms (8 per
    # grid-stride trip + 1 tail element), the wave and block trees (6 + 4), then the
    # second pass over <= 2048 partials (8 per thread, 6 + 4) and the add into out
    n8 = (n + 7) // 8
    blocks = min(2048, (n8 + 255) // 256)
    depth = 8 * ((n8 + blocks * 256 - 1) // (blocks * 256)) + 1 + 10 + 8 + 10 + 1
    assert abs(a.double().item() - ref) <= depth * U * ref
    c = optim.sumsq(x, out=a.clone())  # accumulates into out
    assert abs(c.double().item() - 2 * ref) <= 2 * (depth + 1) * U * ref
