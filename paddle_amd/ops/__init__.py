"""paddle_amd operator library: fused gfx950 HIP kernels with CPU reference paths."""
from . import fused, optim  # noqa: F401
from .fused import (apply_rotary, embedding, flash_attention, flash_attention_varlen, layer_norm, linear, linear_t,  # noqa: F401
                    linear_gelu, rms_norm, packed_attention, rope_attention, rope_tables, softmax, softmax_cross_entropy, swiglu,
                    deinterleave_gate_up, interleave_gate_up, qkv_rope_attention, swiglu_mlp, add, scale,
                    position_add, mean_valid, cross_entropy_tokens, reshape, stack_mean,
                    row_gather, concat_rows)
from .decode import KVCache, PagedKVCache, kv_append, decode_attention  # noqa: F401
from .decode import extend_attention, default_extend_splits  # noqa: F401
from .kv_fp8 import quantize_kv_fp8, dequantize_kv_fp8  # noqa: F401
from . import skinny  # noqa: F401
from .skinny import skinny_ok, skinny_linear, skinny_linear_t, skinny_default_splits  # noqa: F401
from . import skinny_fp8  # noqa: F401
from .skinny_fp8 import Fp8Weight, quantize_weight_fp8, skinny_fp8_ok, skinny_fp8_default_splits  # noqa: F401
from . import sampling  # noqa: F401
from .sampling import SamplerState, philox_uniform, sample_step, sample_tokens  # noqa: F401
from . import speculative  # noqa: F401
from .speculative import SpecState, spec_commit, spec_judge, spec_kernel_ok, spec_margins, spec_verify  # noqa: F401
from . import moe_decode  # noqa: F401
from .moe_decode import moe_decode_ok, moe_decode_route, moe_decode_ffn, moe_decode_default_splits  # noqa: F401
