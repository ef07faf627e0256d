"""The MFMA decode attention (csrc/kernels/attn_decode_gqa.hip) against the float64 attention
oracle, its promised bit equalities, its routing behind ``ops.decode_attention`` and a graph-
replayed ERNIE-MoE with 5 query heads per KV head."""
import math

import pytest
import torch

import attn_oracle as AO
import test_kv_fp8_cpu as K
import test_kv_fp8_gpu as G8
from paddle_amd import ops
from paddle_amd.ops import decode as DEC
from test_extend_gpu import i32, pool, qdq, slab, store
from test_moe_decode_cpu import make_ernie

pytestmark = pytest.mark.gpu

dev = "cuda"
KT = 32  # the kernel's per-wave key tile
LENS = (0, 1, KT - 1, KT, KT + 1, 257)
SENTINEL, PAD = -7.5, 1024


def run(q, cache, scale, ns, kv_len):
    """The kernel, whatever the routing says, into a buffer bordered by a sentinel."""
    n = q.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.bfloat16, device=dev)
    out = buf[PAD:PAD + n].view(q.shape)
    with G8.knobs() as calls:
        o = DEC._decode_mfma_kernel(q, cache, 0, float(scale), ns, kv_len, out=out)
    assert o is not None and calls == ["pa_attn_decode_mfma"], calls
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all()), "a store outside o"
    return o.clone()


def rows_of(i, Hq, Hk, D):
    """Per row of LENS ((q, k, v, do), reference); the row without a key borrows a q."""
    scale = AO.SCALE_FACTORS[i % 3] / math.sqrt(D)
    rows = [AO.case(AO.PROFILES[(i + b) % 5], 1, 1, max(n, 1), Hq, Hk, D, scale, True, seed=b)
            for b, n in enumerate(LENS)]
    return scale, rows


def filled(c, rows, f=lambda x: x):
    for b, (inp, _) in enumerate(rows):
        if LENS[b]:
            store(c, b, f(inp[1][0]), f(inp[2][0]))
    return c


HEADS = ((5, 1), (10, 2), (7, 1), (16, 1), (6, 2), (4, 1))


@pytest.mark.parametrize("i,Hq,Hk,D", [(i, *h, D) for i, (h, D) in enumerate((h, D) for D in (64, 128) for h in HEADS)])
def test_oracle(i, Hq, Hk, D):
    """Every row within the oracle's bound of the float64 reference for 1, 3 and the default
    number of splits over a cache that holds NaN beyond each row's length; no key: zeros."""
    scale, rows = rows_of(i, Hq, Hk, D)
    c = filled(slab(len(LENS), Hk, D), rows)
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    worst = 0.0
    for ns in (1, 3, None):
        o = run(q, c, scale, ns, i32(LENS))
        assert torch.isfinite(o).all() and not o[0].any(), ns
        for b, (_, ref) in enumerate(rows[1:], 1):
            st = AO.row_stat(o[b:b + 1], ref["O"], ref["magO"])
            print(f"decode gqa D {D} Hq {Hq} Hk {Hk} splits {ns} keys {LENS[b]}: {st:.2e}")
            worst = max(worst, st)
    assert worst < AO.BOUND, worst


@pytest.mark.parametrize("i,Hq,Hk,D", [(0, 10, 2, 128), (1, 16, 1, 64)])
def test_bit_equalities(i, Hq, Hk, D):
    scale, rows = rows_of(i, Hq, Hk, D)
    B, kv_len = len(LENS), i32(LENS)
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    c8 = filled(slab(B, Hk, D, "fp8_e4m3"), rows)
    c16 = filled(slab(B, Hk, D), rows, qdq)  # what c8.dequant(0) holds below each row's length
    pools = [filled(pool(B, Hk, D, bs, seed=i, kv_dtype="fp8_e4m3"), rows) for bs in (16, 64)]
    pools += [filled(pool(B, Hk, D, bs, seed=i + 1), rows, qdq) for bs in (16, 64)]
    for ns in (1, 3, None):
        o16 = run(q, c16, scale, ns, kv_len)
        assert K.same_bits(run(q, c8, scale, ns, kv_len), o16), f"splits {ns}: e4m3 != bf16 over the dequantised cache"
        for pg in pools:
            assert K.same_bits(run(q, pg, scale, ns, kv_len), o16), \
                f"splits {ns} block {pg.block_size} quantised {pg.quantized}: paged != contiguous"
        assert K.same_bits(run(q, c16, scale, ns, kv_len), o16), "run to run"
    # row b of the batch is the 1-row call
    o16 = run(q, c16, scale, 3, kv_len)
    for b in (2, 5):
        c1 = slab(1, Hk, D)
        store(c1, 0, qdq(rows[b][0][1][0]), qdq(rows[b][0][2][0]))
        assert K.same_bits(run(q[b:b + 1], c1, scale, 3, i32(LENS[b:b + 1])), o16[b:b + 1]), b
    # a paged row whose only block is out of range sees nothing; the other rows do not move
    pg = pools[3]
    pg.block_table[4, 0] = pg.num_blocks + 3
    o = run(q, pg, scale, 3, kv_len)
    assert not o[4].any() and K.same_bits(o[[1, 2, 3, 5]], o16[[1, 2, 3, 5]])


NAMES = {(False, None): "pa_attn_decode", (True, None): "pa_attn_decode_paged",
         (False, "fp8_e4m3"): "pa_attn_decode_f8", (True, "fp8_e4m3"): "pa_attn_decode_paged_f8"}


@pytest.mark.parametrize("paged,kv_dtype", list(NAMES))
def test_routing(paged, kv_dtype):
    """5 heads per KV head: one recorded call under the existing name, the bits of the MFMA kernel.
    (2, 2) stays on the VALU kernel: the same name, and not the MFMA kernel's bits."""
    D, kv_len = 128, i32(LENS)
    for Hq, Hk, moved in ((5, 1, True), (2, 2, False)):
        scale, rows = rows_of(2, Hq, Hk, D)
        c = pool(len(LENS), Hk, D, 16, seed=5, kv_dtype=kv_dtype) if paged else slab(len(LENS), Hk, D, kv_dtype)
        filled(c, rows)
        q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
        with G8.knobs() as calls:
            o = ops.decode_attention(q, c, 0, scale=scale, num_splits=3, kv_len=kv_len)
        assert calls == [NAMES[paged, kv_dtype]], calls
        assert K.same_bits(o, run(q, c, scale, 3, kv_len)) == moved
        if not moved:
            f = qdq if kv_dtype else (lambda x: x)
            for b, (inp, _) in enumerate(rows[1:], 1):
                ref = AO.reference(inp[0], f(inp[1]), f(inp[2]), inp[3], True, scale)
                assert AO.row_stat(o[b:b + 1], ref["O"], ref["magO"]) < AO.BOUND, b


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
def test_ernie_moe_graph_generation(cache):
    """10 / 2 heads of 64: a captured decode step cannot hold the reference attention (it reads
    the lengths on the host), so graph=True giving the tokens of graph=False shows the kernel."""
    m = make_ernie("grouped", dev, "bfloat16", hidden_size=640, num_attention_heads=10)
    g = torch.Generator().manual_seed(3)
    lens = [9, 17, 4]
    ids = torch.zeros(3, max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
    ids = ids.to(dev)
    kw = dict(prompt_lens=lens, cache=cache, sampler="philox")
    want, _ = m.generate(ids, 6, **kw)
    got, _ = m.generate(ids, 6, graph=True, **kw)
    assert torch.equal(got, want)
    c = m.init_cache(3, 64, paged=True, block_size=16) if cache == "paged" else m.init_cache(3, 64)
    m.prefill(ids, c, lens)
    with G8.knobs() as calls:
        m.decode_step(want[:, 0], c)
    name = "pa_attn_decode_paged" if cache == "paged" else "pa_attn_decode"
    assert calls.count(name) == m.cfg.num_hidden_layers, calls
