"""Every operator type the reference registers (REGISTER_OPERATOR /
REGISTER_OP_WITHOUT_GRADIENT / REGISTER_ACTIVATION_OP under paddle/fluid/operators)
has a kernel here, except the TensorRT engine op (no gfx950 backend; README
non-goals).  The registered type names are stored, one per line, in
tests/golden/fluid_op_types.txt."""
import os

import paddle_amd.operators  # noqa: F401
from paddle_amd.framework import registry as R

NAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fluid_op_types.txt")


def test_every_reference_op_type_is_registered():
    with open(NAMES) as fh:
        names = {l.strip() for l in fh if l.strip()}
    fwd = {n for n in names if not n.endswith("_grad")} - {"tensorrt_engine"}
    missing = sorted(n for n in fwd if n not in R.OP_REGISTRY)
    assert len(fwd) > 150
    assert not missing, missing
