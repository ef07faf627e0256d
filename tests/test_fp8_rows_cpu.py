"""ops/rows_fp8.py without a GPU: the fall-back, the host split rule and ``cached_linear``'s routing."""
import pytest
import torch

from paddle_amd import ops
from paddle_amd.models.generation import cached_linear
from paddle_amd.ops import rows_fp8
from paddle_amd.utils import flags


def _weight():
    g = torch.Generator().manual_seed(1)
    w8 = ops.quantize_weight_fp8((torch.randn(688, 256, generator=g) * 688 ** -0.5).bfloat16())
    return w8, torch.randn(20, 688, generator=g), torch.randn(256, generator=g)


@pytest.mark.parametrize("use_bias,act", [(False, None), (True, "gelu_tanh"), (False, "swiglu_interleaved")])
def test_op_is_skinny_linear_on_the_cpu(use_bias, act):
    w8, x, b = _weight()
    bias = b if use_bias else None
    assert not ops.fp8_linear_ok(x, w8, bias, act)
    got = ops.fp8_linear(x, w8, bias, act)
    assert got.shape == (20, 128 if act == "swiglu_interleaved" else 256)
    assert torch.equal(got, ops.skinny_linear(x, w8, bias, act))
    with pytest.raises(ValueError):
        ops.fp8_linear(x, w8, act="relu")


def test_default_splits_come_from_n_and_k_alone():  # workgroups x splits <= 512, slices >= 512 k, at most 8
    assert [ops.rows_fp8_default_splits(n, k) for n, k in
            [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (80, 4112), (272, 400), (16, 16)]] \
        == [4, 8, 2, 8, 8, 1, 1]


def test_cached_linear_routes_an_fp8_weight_above_16_rows():
    w8, _, _ = _weight()
    R = rows_fp8.ROUTED_ROWS
    assert rows_fp8.MIN_ROUTED_ROWS == 17 <= R <= rows_fp8.MAX_ROWS == 256
    for n in (1, 16, 17, R, R + 1, 300):
        want = ops.fp8_linear if 16 < n <= R else ops.skinny_linear
        assert cached_linear(w8, n) is want, n
        assert cached_linear(w8.dequant(), n) is ops.skinny_linear
    flags.set("fp8_rows", False)
    try:
        assert cached_linear(w8, 17) is ops.skinny_linear
    finally:
        flags.set("fp8_rows", True)
