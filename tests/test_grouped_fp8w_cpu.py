"""``ops.grouped_swiglu_mlp_fp8w`` without a GPU: its plain-torch definition against the float64
oracle of moe_decode_oracle.py (``ffn_oracle`` with one expert per row and weight 1 is this op's
definition; its bound as it is), and the argument checks.  ``case`` also serves the GPU tests."""
import pytest
import torch

import moe_decode_oracle as O
from paddle_amd import ops
from paddle_amd.ops.grouped_fp8w import TM

PATTERNS = ("zero_or_one", "tile_edges", "all_on_last", "random_100")
_cases = {}


def counts_of(pattern, E):
    if pattern == "zero_or_one":
        return [int(e % 3 != 1) for e in range(E)]
    if pattern == "tile_edges":  # TM - 1, TM and TM + 1 rows on three experts, the rest none
        return [{1: TM - 1, E // 2: TM, E - 2: TM + 1}.get(e, 0) for e in range(E)]
    if pattern == "all_on_last":
        return [0] * (E - 1) + [3 * TM + 5]
    g = torch.Generator().manual_seed(5)  # 100 rows over a seeded half of the experts
    live = torch.randperm(E, generator=g)[:E // 2]
    return torch.bincount(live[torch.randint(0, E // 2, (100,), generator=g)], minlength=E).tolist()


def case(H, I, E, pattern, seed=0):
    """Sorted rows, the quantised stacks (a seeded power of two per (expert, column): no two
    scales of a tile need be equal), the counts and the oracle on the dequantised stacks."""
    key = (H, I, E, pattern)
    if key not in _cases:
        counts = pattern if isinstance(pattern, tuple) else counts_of(pattern, E)
        R = sum(counts)
        x, _, gate_up, down = O.make_inputs(R, H, I, E, seed)
        g = torch.Generator().manual_seed(17)
        gu8 = ops.quantize_experts_fp8(gate_up.float() * 2.0 ** torch.randint(-6, 7, (E, 1, 2 * I), generator=g))
        dn8 = ops.quantize_experts_fp8(down.float() * 2.0 ** torch.randint(-6, 7, (E, 1, H), generator=g))
        e_of_row = torch.repeat_interleave(torch.arange(E), torch.tensor(counts))
        ref, bound = O.ffn_oracle(x, gu8.dequant(), dn8.dequant(), e_of_row[:, None], torch.ones(R, 1))
        _cases[key] = dict(x=x, gu=gu8, dn=dn8, counts=counts, ref=ref, bound=bound)
    return _cases[key]


def test_the_definition_is_inside_the_oracle_bound():
    c = case(256, 128, 8, "random_100")
    assert 0 in c["counts"] and sum(c["counts"]) == 100
    assert not ops.grouped_fp8w_ok(c["x"], c["gu"], c["dn"])  # CPU tensors
    for counts in (c["counts"], torch.tensor(c["counts"])):
        y = ops.grouped_swiglu_mlp_fp8w(c["x"], c["gu"], c["dn"], counts)
        assert y.shape == c["x"].shape and y.dtype == torch.bfloat16
        O.check_bound(y, c["ref"], c["bound"], "plain-torch definition, 100 rows")


def test_argument_checks():
    c = case(256, 128, 8, "random_100")
    x, gu, dn, counts = c["x"], c["gu"], c["dn"], c["counts"]
    short = counts[:-1] + [counts[-1] + 1]
    other = ops.quantize_experts_fp8(torch.zeros(8, 64, 256))
    for args in ((x, gu, dn, short), (x, gu, dn, torch.tensor(short)), (x, gu, dn, counts[:-1]),
                 (x, gu, other, counts), (x[:, :128], gu, dn, counts),
                 (x, gu.dequant(), dn, counts), (x, gu, dn.dequant(), counts)):
        with pytest.raises(ValueError):
            ops.grouped_swiglu_mlp_fp8w(*args)
