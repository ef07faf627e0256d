"""The KV-cache decode kernels (csrc/kernels/attn_decode.hip) against the fp32 torch
reference paths of ops/decode.py."""
import math

import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import decode as DEC

pytestmark = pytest.mark.gpu

dev = "cuda"


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


KV_LEN = [1, 2, 63, 64, 65, 300, 384]


@pytest.mark.parametrize("D,Hq,Hk", [(128, 8, 2), (128, 4, 4), (64, 2, 2), (128, 8, 1)])
def test_decode_attention(D, Hq, Hk):
    torch.manual_seed(0)
    B, S_max = len(KV_LEN), 384
    cache = ops.KVCache(1, B, S_max, Hk, D, torch.bfloat16, dev)
    cache.k[0].copy_(torch.randn(B, S_max, Hk, D, device=dev))
    cache.v[0].copy_(torch.randn(B, S_max, Hk, D, device=dev))
    # slots beyond kv_len hold inf: reading one would turn the output into inf / NaN
    for b, n in enumerate(KV_LEN):
        cache.k[0][b, n:] = float("inf")
        cache.v[0][b, n:] = float("inf")
    kv_len = torch.tensor(KV_LEN, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    ref = DEC._decode_attention_ref(q.float(), cache.k[0].float(), cache.v[0].float(), kv_len, scale)
    assert ref.dtype == torch.float32 and torch.isfinite(ref).all()
    assert DEC.N.lib().pa_attn_decode_ok(B, S_max, Hq, Hk, D, 5, DEC.ctypes_long_array([q.stride(0), q.stride(2)]))
    outs = {}
    for ns in (1, 2, 5):
        o = ops.decode_attention(q, cache, 0, num_splits=ns, kv_len=kv_len)
        assert o.shape == (B, 1, Hq, D) and o.dtype == torch.bfloat16
        assert not torch.isnan(o).any(), f"NaN with {ns} splits"
        e = _rel(o, ref)
        print(f"decode_attention D={D} Hq={Hq} Hk={Hk} splits={ns}: rel {e:.3e}")
        assert e < 1e-2
        again = ops.decode_attention(q, cache, 0, num_splits=ns, kv_len=kv_len)
        assert torch.equal(o, again), f"{ns} splits: two runs differ"
        outs[ns] = o
    assert _rel(outs[2], outs[1]) < 1e-2 and _rel(outs[5], outs[1]) < 1e-2
    # the default split count (chosen from the shape alone) and the default kv_len = lens + 1
    cache.set_lens([n - 1 for n in KV_LEN])
    assert _rel(ops.decode_attention(q, cache, 0), ref) < 1e-2


def test_decode_attention_empty_row_and_fallback():
    torch.manual_seed(0)
    B, S_max, Hq, Hk, D = 2, 64, 2, 2, 64
    cache = ops.KVCache(1, B, S_max, Hk, D, torch.bfloat16, dev)
    cache.k[0].copy_(torch.randn(B, S_max, Hk, D, device=dev))
    cache.v[0].copy_(torch.randn(B, S_max, Hk, D, device=dev))
    kv_len = torch.tensor([0, 9], dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    o = ops.decode_attention(q, cache, 0, num_splits=2, kv_len=kv_len)
    assert torch.equal(o[0], torch.zeros_like(o[0]))  # kv_len == 0 writes zeros
    ref = DEC._decode_attention_ref(q.float(), cache.k[0].float(), cache.v[0].float(), kv_len, 1.0 / math.sqrt(D))
    assert _rel(o[1], ref[1]) < 1e-2
    # a group size the kernel does not cover is refused by the query (reference path)
    assert not DEC.N.lib().pa_attn_decode_ok(B, S_max, 6, 2, D, 1, DEC.ctypes_long_array([6 * D, D]))


def test_cache_offsets_past_2g_elements():
    """The last batch row of this cache starts 2^31 elements into k / v: append one token
    there and attend to it (a 32-bit offset would land in another row or out of range)."""
    torch.manual_seed(0)
    B, S_max, H, D, n = 5, 65536, 64, 128, 300
    assert (B - 1) * S_max * H * D >= 2 ** 31
    cache = ops.KVCache(1, B, S_max, H, D, torch.bfloat16, dev)
    cache.k[0][B - 1, : n - 1].copy_(torch.randn(n - 1, H, D, device=dev))
    cache.v[0][B - 1, : n - 1].copy_(torch.randn(n - 1, H, D, device=dev))
    cache.set_lens([0] * (B - 1) + [n - 1])
    cos, sin = ops.rope_tables(n, D, device=dev)
    qkv = torch.randn(B, 1, 3 * H * D, device=dev, dtype=torch.bfloat16)
    q = ops.kv_append(qkv, cache, 0, H, H, cos, sin)
    x = qkv.view(B, 1, 3 * H, D)
    want_k = DEC._rope_at(x[B - 1:, :, H:2 * H].float(), cos, sin, torch.tensor([[n - 1]], device=dev))
    assert _rel(cache.k[0][B - 1, n - 1], want_k[0, 0]) < 1e-2
    assert torch.equal(cache.v[0][B - 1, n - 1], x[B - 1, 0, 2 * H:])
    assert not cache.k[0][B - 1, n:n + 2].any() and not cache.k[0][B - 2, -2:].any()
    o = ops.decode_attention(q, cache, 0, num_splits=2)
    ref = DEC._decode_attention_ref(q[B - 1:].float(), cache.k[0][B - 1:, :n].float(), cache.v[0][B - 1:, :n].float(),
                                    torch.tensor([n]), 1.0 / math.sqrt(D))
    assert _rel(o[B - 1:], ref) < 1e-2


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("Hq,Hk,D", [(4, 2, 128), (2, 2, 64)])
def test_kv_append(Hq, Hk, D, T):
    torch.manual_seed(0)
    B, S_max, pos = 2, 64, [0, 37]
    W = (Hq + 2 * Hk) * D
    cos, sin = ops.rope_tables(S_max, D, device=dev)
    # a column slice of a wider tensor: non-contiguous rows
    wide = torch.randn(B, T, W + 64, device=dev, dtype=torch.bfloat16)
    qkv = wide[:, :, 32:32 + W]
    assert not qkv.is_contiguous()
    sentinel = -7.5

    def fresh(dtype):
        c = ops.KVCache(1, B, S_max, Hk, D, dtype, dev)
        c.k[0].fill_(sentinel)
        c.v[0].fill_(sentinel)
        c.set_lens(pos)
        return c

    ref_cache = fresh(torch.float32)  # fp32: the reference path
    q_ref = ops.kv_append(qkv.float(), ref_cache, 0, Hq, Hk, cos, sin)
    cache = fresh(torch.bfloat16)
    q = ops.kv_append(qkv, cache, 0, Hq, Hk, cos, sin)
    x = qkv.reshape(B, T, Hq + 2 * Hk, D)
    assert _rel(q, q_ref) < 1e-2
    outside = torch.ones(B, S_max, dtype=torch.bool, device=dev)
    for b in range(B):
        sl = slice(pos[b], pos[b] + T)
        outside[b, sl] = False
        assert _rel(cache.k[0][b, sl], ref_cache.k[0][b, sl]) < 1e-2
        assert torch.equal(cache.v[0][b, sl], x[b, :, Hq + Hk:])
    for t in (cache.k[0], cache.v[0]):
        assert torch.equal(t[outside], torch.full_like(t[outside], sentinel))
    # no rotation: q and k are the input bits
    cache = fresh(torch.bfloat16)
    q = ops.kv_append(qkv, cache, 0, Hq, Hk)
    assert torch.equal(q, x[:, :, :Hq])
    for b in range(B):
        sl = slice(pos[b], pos[b] + T)
        assert torch.equal(cache.k[0][b, sl], x[b, :, Hq:Hq + Hk])
        assert torch.equal(cache.v[0][b, sl], x[b, :, Hq + Hk:])
    for t in (cache.k[0], cache.v[0]):
        assert torch.equal(t[outside], torch.full_like(t[outside], sentinel))
    # the lengths advance on the device
    cache.advance(T)
    assert cache.lens.tolist() == [p + T for p in pos]
