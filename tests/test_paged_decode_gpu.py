"""The paged KV-cache kernels (pa_kv_append_paged / pa_attn_decode_paged of
csrc/kernels/attn_decode.hip) against the contiguous kernels, bit for bit, and the models
on a paged cache against the same models on a contiguous one."""
import math

import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import decode as DEC
from test_generation_cpu import MODELS
from test_generation_gpu import _check_consistent, model_pair

pytestmark = pytest.mark.gpu

dev = "cuda"

KV_LEN = [0, 1, 2, 63, 64, 65, 300, 384]
S_MAX = 384


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _shuffled_table(lens, bs, max_blocks, num_blocks, seed):
    """Block ids in random order, dealt to the rows round-robin: no row's blocks are
    monotone or adjacent, and neighbouring ids belong to different rows."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(num_blocks, generator=g).tolist()
    need = [-(-n // bs) for n in lens]
    table = [[-1] * max_blocks for _ in lens]
    for j in range(max(need)):
        for b in range(len(lens)):
            if j < need[b]:
                table[b][j] = ids.pop()
    return table


_slabs = {}


def _slab(D, Hq, Hk):
    """The contiguous cache, q and the contiguous kernel's outputs per split count: computed
    once per shape, shared by both block sizes, left unchanged."""
    key = (D, Hq, Hk)
    if key not in _slabs:
        torch.manual_seed(0)
        B = len(KV_LEN)
        cache = ops.KVCache(1, B, S_MAX, Hk, D, torch.bfloat16, dev)
        cache.k[0].copy_(torch.randn(B, S_MAX, Hk, D, device=dev))
        cache.v[0].copy_(torch.randn(B, S_MAX, Hk, D, device=dev))
        for b, n in enumerate(KV_LEN):
            cache.k[0][b, n:] = float("inf")
            cache.v[0][b, n:] = float("inf")
        kv_len = torch.tensor(KV_LEN, dtype=torch.int32, device=dev)
        q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
        want = {ns: ops.decode_attention(q, cache, 0, num_splits=ns, kv_len=kv_len) for ns in (1, 2, 5, None)}
        _slabs[key] = (cache, q, kv_len, want)
    return _slabs[key]


@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("D,Hq,Hk", [(128, 8, 2), (128, 4, 4), (64, 2, 2), (128, 8, 1)])
def test_paged_attention_bit_identical(D, Hq, Hk, bs):
    slab, q, kv_len, want = _slab(D, Hq, Hk)
    B = len(KV_LEN)
    need = sum(-(-n // bs) for n in KV_LEN)
    pg = ops.PagedKVCache(1, B, S_MAX, Hk, D, torch.bfloat16, dev, block_size=bs, num_blocks=need + 5)
    table = _shuffled_table(KV_LEN, bs, pg.max_blocks, pg.num_blocks, seed=bs)
    pg.load_block_table(table)
    # every pool slot that holds no valid token is inf
    pg.k[0].fill_(float("inf"))
    pg.v[0].fill_(float("inf"))
    for b, n in enumerate(KV_LEN):
        for j in range(-(-n // bs)):
            cnt = min(bs, n - j * bs)
            pg.k[0][table[b][j], :cnt] = slab.k[0][b, j * bs:j * bs + cnt]
            pg.v[0][table[b][j], :cnt] = slab.v[0][b, j * bs:j * bs + cnt]
    gk, gv = pg.gather(0)
    for b, n in enumerate(KV_LEN):
        assert torch.equal(gk[b, :n], slab.k[0][b, :n]) and torch.equal(gv[b, :n], slab.v[0][b, :n])
    lib = DEC.N.lib()
    qst = DEC.ctypes_long_array([q.stride(0), q.stride(2)])
    assert lib.pa_attn_decode_paged_ok(B, S_MAX, Hq, Hk, D, 5, qst, bs, pg.max_blocks, pg.num_blocks)
    past = torch.tensor([[j >= -(-n // bs) for j in range(pg.max_blocks)] for n in KV_LEN], device=dev)
    for poison in (-1, pg.num_blocks + 7):
        pg.block_table[past] = poison  # entries past each row's last block
        for ns in (1, 2, 5, None):
            o = ops.decode_attention(q, pg, 0, num_splits=ns, kv_len=kv_len)
            assert o.shape == (B, 1, Hq, D) and o.dtype == torch.bfloat16
            assert torch.isfinite(o).all(), f"splits {ns}, table tail {poison}"
            assert torch.equal(o, want[ns]), f"splits {ns}, table tail {poison}: paged != contiguous"
            assert torch.equal(ops.decode_attention(q, pg, 0, num_splits=ns, kv_len=kv_len), o)
            assert torch.equal(o[0], torch.zeros_like(o[0]))  # kv_len == 0
    # the default kv_len = lens + 1
    pg.block_table[past] = -1
    full = [b for b, n in enumerate(KV_LEN) if n >= 1]
    pg.set_lens([max(n - 1, 0) for n in KV_LEN])
    o = ops.decode_attention(q, pg, 0)
    assert torch.equal(o[full], want[None][full])


def test_paged_attention_stale_entry_inside_a_row():
    """A key below kv_len whose table entry is out of range is masked, never read: the
    output is that of a row without those keys, and finite."""
    D, Hq, Hk, bs = 128, 8, 2, 16
    slab, q, kv_len, _ = _slab(D, Hq, Hk)
    B = len(KV_LEN)
    pg = ops.PagedKVCache(1, B, S_MAX, Hk, D, torch.bfloat16, dev, block_size=bs)
    pg.reserve(KV_LEN)
    gk, gv = slab.k[0], slab.v[0]
    for b, n in enumerate(KV_LEN):
        for j, blk in enumerate(pg.row_blocks(b)):
            pg.k[0][blk] = gk[b, j * bs:(j + 1) * bs]
            pg.v[0][blk] = gv[b, j * bs:(j + 1) * bs]
    # row 6 (300 keys) loses its blocks 2 and 17: keys 32..47 and 272..287 are gone
    pg.block_table[6, 2] = pg.num_blocks
    pg.block_table[6, 17] = -5
    o = ops.decode_attention(q, pg, 0, num_splits=2, kv_len=kv_len)
    keep = torch.ones(300, dtype=torch.bool, device=dev)
    keep[32:48] = False
    keep[272:288] = False
    ref = DEC._decode_attention_ref(q[6:7].float(), gk[6:7, :300][:, keep].float(), gv[6:7, :300][:, keep].float(),
                                    torch.tensor([int(keep.sum())]), 1.0 / math.sqrt(D))
    assert torch.isfinite(o).all()
    assert _rel(o[6:7], ref) < 1e-2


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("T", [1, 5])
def test_paged_append_matches_contiguous_kernel(T, rope):
    torch.manual_seed(0)
    B, S_max, pos, bs = 3, 64, [0, 37, 45], 16  # 45 + 5 crosses the block boundary at 48
    Hq, Hk, D = 4, 2, 128
    W = (Hq + 2 * Hk) * D
    cos, sin = ops.rope_tables(S_max, D, device=dev) if rope else (None, None)
    wide = torch.randn(B, T, W + 64, device=dev, dtype=torch.bfloat16)
    qkv = wide[:, :, 32:32 + W]  # a column slice: non-contiguous rows
    assert not qkv.is_contiguous()
    sentinel = -7.5

    def slab():
        c = ops.KVCache(1, B, S_max, Hk, D, torch.bfloat16, dev)
        c.k[0].fill_(sentinel)
        c.v[0].fill_(sentinel)
        c.set_lens(pos)
        return c

    def pool():
        c = ops.PagedKVCache(1, B, S_max, Hk, D, torch.bfloat16, dev, block_size=bs, num_blocks=13)
        c.load_block_table([[5, 2, 7, 0], [3, 6, 1, 4], [11, 9, 12, 10]])  # block 8 belongs to nobody
        c.k[0].fill_(sentinel)
        c.v[0].fill_(sentinel)
        c.set_lens(pos)
        return c

    def check(pg, ref, drop=()):
        gk, gv = pg.gather(0)
        written = torch.zeros(B, S_max, dtype=torch.bool, device=dev)
        for b in range(B):
            written[b, pos[b]:pos[b] + T] = True
        for b, t in drop:
            written[b, t] = False
        assert torch.equal(gk[written], ref.k[0][written]) and torch.equal(gv[written], ref.v[0][written])
        assert (gk[~written] == sentinel).all() and (gv[~written] == sentinel).all()
        assert (pg.k[0][8] == sentinel).all() and (pg.v[0][8] == sentinel).all()

    ref = slab()
    q_ref = ops.kv_append(qkv, ref, 0, Hq, Hk, cos, sin)
    pg = pool()
    q = ops.kv_append(qkv, pg, 0, Hq, Hk, cos, sin)
    assert torch.equal(q, q_ref)
    check(pg, ref)
    pg.advance(T)
    assert pg.lens.tolist() == [p + T for p in pos] and pg.host_lens == [p + T for p in pos]
    # rows=[1, 0, 2]: input row 0 goes to cache row 1 and the other way round
    ref = slab()
    q_ref = ops.kv_append(qkv[[1, 0, 2]], ref, 0, Hq, Hk, cos, sin)
    pg = pool()
    q = ops.kv_append(qkv, pg, 0, Hq, Hk, cos, sin, rows=[1, 0, 2])
    assert torch.equal(q, q_ref[[1, 0, 2]])
    check(pg, ref)
    # an unassigned block: its tokens are dropped, the others land
    if T == 5:
        ref = slab()
        ops.kv_append(qkv, ref, 0, Hq, Hk, cos, sin)
        pg = pool()
        pg.block_table[2, 3] = -1  # tokens 48..63 of row 2 (block 10) have no slot
        ops.kv_append(qkv, pg, 0, Hq, Hk, cos, sin)
        assert (pg.k[0][10] == sentinel).all() and (pg.v[0][10] == sentinel).all()
        pg.block_table[2, 3] = 10  # look at block 10 through gather again
        check(pg, ref, drop=[(2, 48), (2, 49)])


def test_paged_pool_offsets_past_2g_elements():
    """The pool's last block starts 2^31 elements into k / v.  A row that owns it appends a
    token into it and attends over it (a 32-bit offset would land elsewhere)."""
    torch.manual_seed(0)
    B, S_max, H, D, bs, n = 2, 512, 8, 128, 256, 300
    nb = 8193
    assert (nb - 1) * bs * H * D >= 2 ** 31
    pg = ops.PagedKVCache(1, B, S_max, H, D, torch.bfloat16, dev, block_size=bs, num_blocks=nb, zero_fill=False)
    pg.load_block_table([[3, nb - 1], [-1, -1]])  # tokens 256.. of row 0 live in the last block
    pg.k[0][3].copy_(torch.randn(bs, H, D, device=dev))
    pg.v[0][3].copy_(torch.randn(bs, H, D, device=dev))
    pg.k[0][nb - 1].copy_(torch.randn(bs, H, D, device=dev))
    pg.v[0][nb - 1].copy_(torch.randn(bs, H, D, device=dev))
    pg.k[0][0].zero_()  # what gather() reads for "no block" before it masks it
    pg.v[0][0].zero_()
    before_k = pg.k[0][nb - 1].clone()
    pg.set_lens([n - 1, 0])
    cos, sin = ops.rope_tables(n, D, device=dev)
    qkv = torch.randn(B, 1, 3 * H * D, device=dev, dtype=torch.bfloat16)
    q = ops.kv_append(qkv, pg, 0, H, H, cos, sin)
    x = qkv.view(B, 1, 3 * H, D)
    slot = n - 1 - bs
    want_k = DEC._rope_at(x[:1, :, H:2 * H].float(), cos, sin, torch.tensor([[n - 1]], device=dev))
    assert _rel(pg.k[0][nb - 1, slot], want_k[0, 0]) < 1e-2
    assert torch.equal(pg.v[0][nb - 1, slot], x[0, 0, 2 * H:])
    others = torch.ones(bs, dtype=torch.bool, device=dev)
    others[slot] = False
    assert torch.equal(pg.k[0][nb - 1][others], before_k[others])
    o = ops.decode_attention(q, pg, 0, num_splits=2)
    gk, gv = pg.gather(0)
    ref = DEC._decode_attention_ref(q[:1].float(), gk[:1, :n].float(), gv[:1, :n].float(), torch.tensor([n]),
                                    1.0 / math.sqrt(D))
    assert torch.isfinite(o[:1]).all()
    assert _rel(o[:1], ref) < 1e-2


def test_paged_fallback_group_of_six():
    torch.manual_seed(0)
    B, S_max, Hq, Hk, D, bs = 2, 64, 12, 2, 64, 16
    lib = DEC.N.lib()
    qst = DEC.ctypes_long_array([Hq * D, D])
    assert lib.pa_attn_decode_paged_ok(B, S_max, 8, Hk, D, 1, qst, bs, 4, 8)
    assert not lib.pa_attn_decode_paged_ok(B, S_max, Hq, Hk, D, 1, qst, bs, 4, 8)  # Hq / Hk = 6
    assert not lib.pa_attn_decode_paged_ok(B, S_max, 8, Hk, D, 1, qst, 48, 4, 8)  # not a block size
    assert not lib.pa_attn_decode_paged_ok(B, S_max, 8, Hk, D, 1, qst, bs, 3, 8)  # table shorter than S_max
    pg = ops.PagedKVCache(1, B, S_max, Hk, D, torch.bfloat16, dev, block_size=bs)
    pg.reserve([9, 40])
    pg.k[0].copy_(torch.randn_like(pg.k[0]))
    pg.v[0].copy_(torch.randn_like(pg.v[0]))
    kv_len = torch.tensor([9, 40], dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    o = ops.decode_attention(q, pg, 0, kv_len=kv_len)  # the reference path over gather()
    gk, gv = pg.gather(0)
    assert torch.equal(o, DEC._decode_attention_ref(q, gk, gv, kv_len, 1.0 / math.sqrt(D)))


# ------------------------------------------------------------------ models
@pytest.mark.parametrize("kind", MODELS)
def test_models_paged_equals_contiguous_gpu(kind):
    model, _ = model_pair(kind)
    torch.manual_seed(3)
    B, S, P = 2, 24, 8
    ids = torch.randint(1, model.cfg.vocab_size, (B, S), device=dev)

    def forced(**kw):
        cache = model.init_cache(B, S, **kw)
        out = [model.prefill(ids[:, :P], cache)]
        for t in range(P, S):
            out.append(model.decode_step(ids[:, t], cache))
        return torch.stack(out, 1), cache

    want, _ = forced()
    got, cache = forced(paged=True, block_size=16)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert cache.lens.tolist() == [S, S] and cache.blocks_used == 4
    # generate: greedy with ragged prompts
    padded = ids[:, :7].clone()
    padded[0, 3:] = 0
    want, want_len = model.generate(padded, 8, prompt_lens=[3, 7])
    got, got_len = model.generate(padded, 8, prompt_lens=[3, 7], cache="paged", block_size=16)
    assert torch.equal(got, want) and torch.equal(got_len, want_len)


@pytest.mark.parametrize("kind", MODELS)
def test_admission_gpu(kind):
    """Prefill two rows, decode 3 steps, replace row 0 by a new prompt, decode 5 more.
    Row 1's logits are bit-equal to a run without the replacement (decode attention, the
    skinny GEMMs and the norms compute a batch row from that row alone); row 0's new
    tokens are consistent with the full forward over the new prompt."""
    model, ref = model_pair(kind)
    torch.manual_seed(6)
    V = model.cfg.vocab_size
    ids = torch.randint(1, V, (2, 5), device=dev)
    new_prompt = torch.randint(1, V, (1, 9), device=dev)

    def run(replace):
        cache = model.init_cache(2, 40, paged=True, block_size=16)
        logits = model.prefill(ids, cache)
        row1, row0 = [logits[1]], []
        for step in range(8):
            if step == 3 and replace:
                held = cache.row_blocks(1)
                first = model.prefill(new_prompt, cache, rows=[0])
                assert cache.row_blocks(1) == held and cache.host_lens == [9, 8]
                logits = torch.cat([first, logits[1:]], 0)
            tok = logits.float().argmax(-1)
            if step >= 3:
                row0.append(tok[0])
            logits = model.decode_step(tok, cache)
            row1.append(logits[1])
        return torch.stack(row1), torch.stack(row0), cache

    kept1, _, _ = run(False)
    got1, got0, cache = run(True)
    assert torch.equal(got1, kept1)
    assert cache.lens.tolist() == [14, 13]
    _check_consistent(model, ref, torch.cat([new_prompt, got0[None]], 1), got0[None], [9], f"admitted row {kind}")
