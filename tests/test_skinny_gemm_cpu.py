"""ops.skinny_* off the GPU: every call must evaluate exactly the expression the models
used before these ops existed, ``skinny_ok`` must say no, and the split count must be a
host-side function of (layout, N, K)."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.utils import flags


def _inputs(dtype, rows=(3, 1), K=64, N=96):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(*rows, K, generator=g).to(dtype)
    w = (torch.randn(K, N, generator=g) * 0.1).to(dtype)
    b = torch.randn(N, generator=g).to(dtype)
    return x, w, b


def _swiglu_parent(x, w):
    gu = ops.linear(x, w)
    g, u = ops.deinterleave_gate_up(gu)
    return (torch.nn.functional.silu(g.float()) * u.float()).to(x.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_results_are_the_parent_expressions(dtype):
    x, w, b = _inputs(dtype)
    with torch.no_grad():
        assert torch.equal(ops.skinny_linear(x, w), ops.linear(x, w))
        assert torch.equal(ops.skinny_linear(x, w, b), ops.linear(x, w, b))
        assert torch.equal(ops.skinny_linear(x, w, b, act="gelu_tanh"), ops.linear_gelu(x, w, b))
        got = ops.skinny_linear(x, w, act="swiglu_interleaved")
        assert got.shape == (3, 1, 48) and torch.equal(got, _swiglu_parent(x, w))
        wt = w.t().contiguous()  # [N, K]
        assert torch.equal(ops.skinny_linear_t(x, wt), ops.linear_t(x, wt))
    assert ops.skinny_linear(x, w).shape == (3, 1, 96)
    assert not ops.skinny_linear(x, w).requires_grad


def test_seventeen_rows_return_the_parent_result():
    x, w, b = _inputs(torch.bfloat16, rows=(17,))
    assert not ops.skinny_ok(x, w, bias=b)
    with torch.no_grad():
        assert torch.equal(ops.skinny_linear(x, w, b), ops.linear(x, w, b))
        assert torch.equal(ops.skinny_linear_t(x, w.t().contiguous()), ops.linear_t(x, w.t().contiguous()))


def test_skinny_ok_refusals_on_cpu():
    x, w, b = _inputs(torch.bfloat16)
    assert not ops.skinny_ok(x, w)  # CPU tensors
    assert not ops.skinny_ok(x, w, bias=b, act="gelu_tanh")
    assert not ops.skinny_ok(x, w.t().contiguous(), b_kmaj=True)
    x17, _, _ = _inputs(torch.bfloat16, rows=(17,))
    assert not ops.skinny_ok(x17, w)
    xk, wk, _ = _inputs(torch.bfloat16, K=60)  # K % 8 != 0
    assert not ops.skinny_ok(xk, wk)
    xs, ws, _ = _inputs(torch.bfloat16, N=80)  # SwiGLU needs N % 32 == 0
    assert not ops.skinny_ok(xs, ws, act="swiglu_interleaved")


def test_native_ok_refusals_by_size():
    """The kernel's own gate, on sizes and made-up (aligned) addresses: nothing is allocated."""
    from paddle_amd.ops import _native as N

    ok = N.lib().pa_gemm_skinny_ok
    A, B, C = 0x10000, 0x20000, 0x30000

    def call(b_kmaj=0, M=4, Nn=256, K=64, lda=64, ldb=None, ldc=None, epi=0, splits=1, a=A, b=B, c=C, bias=None):
        ldb = (K if b_kmaj else Nn) if ldb is None else ldb
        ldc = (Nn // 2 if epi == 3 else Nn) if ldc is None else ldc
        return bool(ok(b_kmaj, M, Nn, K, lda, ldb, ldc, epi, splits, a, b, c, bias))

    assert call() and call(M=1) and call(M=16) and call(b_kmaj=1, Nn=257)
    assert not call(M=17) and not call(M=0)
    assert not call(K=60, lda=60)
    assert not call(Nn=260)  # MN-major: N % 8
    assert call(epi=3) and not call(epi=3, Nn=272)  # N % 32
    assert not call(b_kmaj=1, epi=3)
    assert not call(a=A + 2) and not call(b=B + 8)
    assert not call(epi=1) and call(epi=1, bias=0x40000)
    assert not call(splits=0)
    # an operand of 4 GiB or more
    assert call(K=8192, lda=8192, Nn=131080) and not call(K=16384, lda=16384, Nn=131080)
    assert not call(b_kmaj=1, Nn=262144, K=8192, lda=8192)


def test_flag_off_refuses_and_env_name():
    x, w, _ = _inputs(torch.bfloat16)
    assert flags.get("skinny_gemm") is True
    assert "FLAGS_skinny_gemm" in flags.get_flags("skinny_gemm")
    flags.set("skinny_gemm", False)
    try:
        assert not ops.skinny_ok(x, w)
        with torch.no_grad():
            assert torch.equal(ops.skinny_linear(x, w), ops.linear(x, w))
    finally:
        flags.set("skinny_gemm", True)


def test_default_splits_is_a_host_function_of_layout_n_k():
    shapes = [(False, 12288, 4096), (False, 4096, 4096), (False, 22016, 4096), (False, 4096, 11008),
              (False, 32000, 4096), (True, 50257, 4096), (True, 512, 4096), (False, 8, 8), (True, 1, 8)]
    first = [ops.skinny_default_splits(*s) for s in shapes]
    assert first == [ops.skinny_default_splits(*s) for s in shapes]
    assert all(isinstance(v, int) and 1 <= v <= 64 for v in first)
    assert ops.skinny_default_splits(False, 8, 8) == 1  # one slice of 8 rows at most
    assert ops.skinny_default_splits(True, 50257, 4096) == 1  # N alone fills the chip
    assert ops.skinny_default_splits(False, 4096, 4096) > 1  # 32 column tiles do not
    # slices are never shorter than 256 rows (MN-major) / 1024 (K-major)
    for kmaj, n, k in shapes:
        s = ops.skinny_default_splits(kmaj, n, k)
        assert s == 1 or k // s >= (1024 if kmaj else 256)
