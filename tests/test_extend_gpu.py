"""pa_attn_extend (csrc/kernels/attn_extend.hip) against the float64 attention oracle, its bit
equalities (paged = contiguous, e4m3 = bf16 over the dequantised cache, run to run, row
independence, rows=), its edges, and ``model.extend`` / chunked prefill in bf16."""
import math

import pytest
import torch

import attn_oracle as AO
import test_kv_fp8_cpu as K
import test_kv_fp8_gpu as G8
from paddle_amd import ops
from paddle_amd.ops import _native
from paddle_amd.ops import decode as DEC
from test_generation_cpu import MODELS, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
LENS = (0, 63, 257)  # cached tokens per row before the chunk
S_MAX = 512
TS = (1, 5, 16, 33, 130)
HEADS = ((2, 2), (4, 1), (8, 2), (8, 1))
SENTINEL, PAD = -7.5, 1024


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------- caches
def slab(B, Hk, D, kv_dtype=None, S_max=S_MAX):
    """A contiguous cache whose every slot is poisoned: NaN, or NaN codes with an inf scale."""
    c = ops.KVCache(1, B, S_max, Hk, D, torch.bfloat16, dev, kv_dtype=kv_dtype)
    poison(c)
    return c


def pool(B, Hk, D, bs, seed, kv_dtype=None, S_max=S_MAX):
    """A poisoned paged cache with a shuffled, fully assigned table; no row owns pool block 0."""
    mb = -(-S_max // bs)
    c = ops.PagedKVCache(1, B, S_max, Hk, D, torch.bfloat16, dev, block_size=bs, num_blocks=B * mb + 1,
                         kv_dtype=kv_dtype)
    g = torch.Generator().manual_seed(seed)
    c.load_block_table((torch.randperm(B * mb, generator=g) + 1).view(B, mb).int())
    poison(c)
    return c


def poison(c):
    if c.quantized:
        for t in (c.k[0], c.v[0]):
            t.view(torch.uint8).fill_(G8.NAN_CODE)
        c.k_scale[0].fill_(float("inf"))
        c.v_scale[0].fill_(float("inf"))
    else:
        c.k[0].fill_(float("nan"))
        c.v[0].fill_(float("nan"))


def store(c, b, k, v):
    """k / v [n, Hk, D] bf16 (CPU) as the first n tokens of row b: as they are, or quantised."""
    n = k.shape[0]
    if c.quantized:
        (kq, ks), (vq, vs) = ops.quantize_kv_fp8(k), ops.quantize_kv_fp8(v)
        G8.store_row(c, b, kq, ks, vq, vs)
    elif getattr(c, "paged", False):
        sl = G8.pool_slots(c, b, n)
        K.flat(c, c.k[0])[sl] = k.to(dev)
        K.flat(c, c.v[0])[sl] = v.to(dev)
    else:
        c.k[0][b, :n] = k.to(dev)
        c.v[0][b, :n] = v.to(dev)


def qdq(x):
    c, s = ops.quantize_kv_fp8(x)
    return ops.dequantize_kv_fp8(c, s, torch.bfloat16)


def run(q, cache, scale, ns, base, rows_t=None):
    """The kernel into a buffer bordered by a sentinel, which must survive."""
    n = q.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.bfloat16, device=dev)
    out = buf[PAD:PAD + n].view(q.shape)
    with G8.knobs() as calls:
        o = DEC._extend_kernel(q, cache, 0, float(scale), ns, base, rows_t, out=out)
    assert o is not None and calls == ["pa_attn_extend"], calls
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all()), "a store outside o"
    return o.clone()


def oracle_rows(i, T, D):
    """Case i at chunk length T: the head configuration and the scale rotate with i, the
    profile with i and the row.  Per row ((q, k, v, do), reference) from the oracle's cache."""
    Hq, Hk = HEADS[i % 4]
    scale = AO.SCALE_FACTORS[i % 3] / math.sqrt(D)
    rows = [AO.case(AO.PROFILES[(i + b) % 5], 1, T, n + T, Hq, Hk, D, scale, True, seed=b)
            for b, n in enumerate(LENS)]
    return Hq, Hk, scale, rows


CASES = [(i, T, D) for i, (T, D) in enumerate((T, D) for D in (64, 128) for T in TS)]


# ---------------------------------------------------------------------- oracle
@pytest.mark.parametrize("i,T,D", CASES)
def test_oracle(i, T, D):
    """Every row within the oracle's bound of the float64 reference, for 1, 3 and the default
    number of splits; the slots at and beyond n_b + T hold NaN."""
    Hq, Hk, scale, rows = oracle_rows(i, T, D)
    c = slab(len(LENS), Hk, D)
    for b, (inp, _) in enumerate(rows):
        store(c, b, inp[1][0], inp[2][0])
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    base = i32(LENS)
    worst = 0.0
    for ns in (1, 3, None):
        o = run(q, c, scale, ns, base)
        assert torch.isfinite(o).all(), ns
        for b, (_, ref) in enumerate(rows):
            st = AO.row_stat(o[b:b + 1], ref["O"], ref["magO"])
            print(f"extend T {T} D {D} Hq {Hq} Hk {Hk} splits {ns} row {b}: {st:.2e}")
            worst = max(worst, st)
    assert worst < AO.BOUND, worst
    # the public op takes the same path
    assert K.same_bits(ops.extend_attention(q, c, 0, scale=scale, num_splits=3, base_len=base), run(q, c, scale, 3, base))


# ---------------------------------------------------------------------- bit equalities
def adversarial(D):
    a = K.adversarial_vectors(D)
    return a[torch.isfinite(a.float()).all(-1)]  # zero vectors, the +-448 clamp, exponents near +-100


@pytest.mark.parametrize("i,T,D", [(0, 5, 128), (1, 33, 64), (2, 130, 128), (3, 16, 128), (5, 1, 64)])
def test_bit_equalities(i, T, D):
    Hq, Hk, scale, rows = oracle_rows(i, T, D)
    B = len(LENS)
    kv = []
    for b, (inp, _) in enumerate(rows):
        k, v = inp[1][0].clone(), inp[2][0].clone()
        if b == 2:  # adversarial vectors among the cached keys and values
            adv = adversarial(D)
            k[40:40 + len(adv)] = adv[:, None]
            v[:len(adv)] = adv[:, None]
        kv.append((k, v))
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    base = i32(LENS)
    c8, c16 = slab(B, Hk, D, "fp8_e4m3"), slab(B, Hk, D)
    pools8 = [pool(B, Hk, D, bs, seed=i, kv_dtype="fp8_e4m3") for bs in (16, 64)]
    pools16 = [pool(B, Hk, D, bs, seed=i + 1) for bs in (16, 64)]
    for b, (k, v) in enumerate(kv):
        for c in [c8] + pools8:
            store(c, b, k, v)
        for c in pools16:
            store(c, b, qdq(k), qdq(v))
    dk, dv = c8.dequant(0)
    c16.k[0].copy_(dk)
    c16.v[0].copy_(dv)
    for ns in (1, 3, None):
        o16 = run(q, c16, scale, ns, base)
        o8 = run(q, c8, scale, ns, base)
        assert K.same_bits(o8, o16), f"splits {ns}: e4m3 != bf16 over cache.dequant()"
        for pg in pools16 + pools8:
            assert K.same_bits(run(q, pg, scale, ns, base), o16), \
                f"splits {ns} block {pg.block_size} quantised {pg.quantized}: paged != contiguous"
        assert K.same_bits(run(q, c16, scale, ns, base), o16) and K.same_bits(run(q, c8, scale, ns, base), o8)
    # a rows= subset is those rows of the full call
    pg = pools16[0]
    full = run(q, pg, scale, 3, base)
    sub = run(q[[2, 0]].contiguous(), pg, scale, 3, i32([LENS[2], LENS[0]]), rows_t=i32([2, 0]))
    assert K.same_bits(sub, full[[2, 0]])
    assert K.same_bits(ops.extend_attention(q[[2, 0]], pg, 0, scale=scale, num_splits=3, rows=[2, 0],
                                            base_len=i32([LENS[2], LENS[0]])), sub)
    # row 2 does not depend on what the other rows hold, ask or how long they are
    o = run(q, c16, scale, 3, base)
    q2 = q.clone()
    q2[:2] = torch.randn_like(q2[:2])
    c16.k[0][:2] = torch.randn_like(c16.k[0][:2])
    c16.v[0][:2] = 3.0
    o2 = run(q2, c16, scale, 3, i32([200, 5, LENS[2]]))
    assert K.same_bits(o2[2], o[2]) and not K.same_bits(o2[:2], o[:2])


def test_strided_q_and_default_splits():
    """q as kv_append's view of a wider buffer (8-element-aligned strides), and the split rule."""
    T, D, Hq, Hk = 5, 128, 4, 1
    _, _, scale, rows = oracle_rows(1, T, D)
    c = slab(len(LENS), Hk, D)
    for b, (inp, _) in enumerate(rows):
        store(c, b, inp[1][0], inp[2][0])
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    wide = torch.zeros(len(LENS), T, Hq + 2, D + 8, dtype=torch.bfloat16, device=dev)
    qs = wide[:, :, 1:1 + Hq, 8:]
    qs.copy_(q)
    assert not qs.is_contiguous()
    base = i32(LENS)
    assert K.same_bits(run(qs, c, scale, 2, base), run(q, c, scale, 2, base))
    for B, Hk_, T_, S in ((1, 8, 4, 8192), (8, 32, 16, 2048), (3, 1, 130, 512), (1, 1, 1, 64)):
        ns = ops.default_extend_splits(B, Hk_, T_, S)
        assert 1 <= ns <= 64 and ns <= max(1, S // 256)
    # one rule for both layouts: the default of a paged call is the default of a contiguous one
    pg = pool(len(LENS), Hk, D, 64, seed=3)
    for b, (inp, _) in enumerate(rows):
        store(pg, b, inp[1][0], inp[2][0])
    assert K.same_bits(ops.extend_attention(q, pg, 0, scale=scale, base_len=base),
                       ops.extend_attention(q, c, 0, scale=scale, base_len=base))


# ---------------------------------------------------------------------- edges
@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"])
def test_masked_table_entries(kv_dtype):
    """Entries of -1 and num_blocks in the middle of a row over a NaN-poisoned pool: finite, and
    the oracle's bound against the reference with those keys removed."""
    i, T, D, bs = 2, 33, 128, 16
    Hq, Hk, scale, rows = oracle_rows(i, T, D)
    pg = pool(len(LENS), Hk, D, bs, seed=9, kv_dtype=kv_dtype)
    for b, (inp, _) in enumerate(rows):
        k, v = inp[1][0], inp[2][0]
        store(pg, b, k, v)
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    pg.block_table[2, 2] = -1               # row 2 (257 cached) loses keys 32..47
    pg.block_table[2, 9] = pg.num_blocks    # ... and 144..159
    gone = list(range(32, 48)) + list(range(144, 160))
    inp = rows[2][0]
    keep = torch.ones(LENS[2] + T, dtype=torch.bool)
    keep[gone] = False
    k, v = (qdq(inp[1][0]), qdq(inp[2][0])) if kv_dtype else (inp[1][0], inp[2][0])
    ref = AO.reference(inp[0], k[None][:, keep], v[None][:, keep], inp[3], True, scale)
    for ns in (1, 3):
        o = run(q, pg, scale, ns, i32(LENS))
        assert torch.isfinite(o).all()
        st = AO.row_stat(o[2:3], ref["O"], ref["magO"])
        print(f"masked entries, {kv_dtype}, splits {ns}: {st:.2e}")
        assert st < AO.BOUND, (ns, st)
        whole = AO.row_stat(o[2:3], rows[2][1]["O"], rows[2][1]["magO"])
        assert whole > st  # the removed keys matter


@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"])
def test_no_visible_key_gives_zeros(kv_dtype):
    i, T, D = 0, 5, 64
    Hq, Hk, scale, rows = oracle_rows(i, T, D)
    pg = pool(len(LENS), Hk, D, 16, seed=4, kv_dtype=kv_dtype)
    for b, (inp, _) in enumerate(rows):
        store(pg, b, inp[1][0], inp[2][0])
    q = torch.cat([inp[0] for inp, _ in rows]).to(dev)
    pg.block_table[1].fill_(-1)  # row 1: no key has a block
    pg.block_table[0, 0] = pg.num_blocks + 3  # row 0: its only block (5 keys) is out of range
    for ns in (1, 3):
        o = run(q, pg, scale, ns, i32(LENS))
        assert torch.isfinite(o).all() and not o[:2].any() and bool(o[2].any())
    # a q row mapped outside the cache sees nothing either
    o = run(q, pg, scale, 1, i32(LENS), rows_t=i32([0, 7, 2]))
    assert not o[:2].any() and bool(o[2].any())


@pytest.mark.parametrize("D,Hq,Hk,dtype", [(96, 2, 2, torch.bfloat16), (128, 6, 1, torch.bfloat16),
                                           (128, 4, 2, torch.float32)])
@pytest.mark.parametrize("paged", [False, True])
def test_refused_shapes_take_the_reference(D, Hq, Hk, dtype, paged):
    torch.manual_seed(0)
    B, T, S_max, lens = 2, 5, 40, [7, 30]
    if dtype == torch.bfloat16:
        qst = DEC.ctypes_long_array([T * Hq * D, Hq * D, D])
        assert not _native.lib().pa_attn_extend_ok(B, T, S_max, Hq, Hk, D, 1, qst, 16 if paged else 0, 3, 6)
    kw = dict(block_size=16) if paged else {}
    c = (ops.PagedKVCache if paged else ops.KVCache)(1, B, S_max, Hk, D, dtype, dev, **kw)
    ops.kv_append(torch.randn(B, 36, (Hq + 2 * Hk) * D, device=dev, dtype=dtype), c, 0, Hq, Hk)
    q = torch.randn(B, T, Hq, D, device=dev, dtype=dtype)
    base = i32(lens)
    with G8.knobs() as calls:
        o = ops.extend_attention(q, c, 0, base_len=base)
    assert "pa_attn_extend" not in calls, calls
    k, v = c.dequant(0)
    want = DEC._extend_attention_ref(q, k, v, base, 1.0 / math.sqrt(D))
    assert K.same_bits(o, want) and bool(o.any())


def test_cache_offsets_past_2g_elements():
    """The last row of this cache starts 2^31 elements into k / v: append a chunk there and
    attend to it (a 32-bit offset would land in another row or out of range)."""
    torch.manual_seed(0)
    B, S_max, H, D, n, T = 5, 65536, 64, 128, 300, 5
    assert (B - 1) * S_max * H * D >= 2 ** 31
    cache = ops.KVCache(1, B, S_max, H, D, torch.bfloat16, dev)
    cache.k[0][B - 1, :n].copy_(torch.randn(n, H, D, device=dev))
    cache.v[0][B - 1, :n].copy_(torch.randn(n, H, D, device=dev))
    cache.set_lens([0] * (B - 1) + [n])
    qkv = torch.randn(B, T, 3 * H * D, device=dev, dtype=torch.bfloat16)
    q = ops.kv_append(qkv, cache, 0, H, H)
    with G8.knobs() as calls:
        o = ops.extend_attention(q, cache, 0, num_splits=2)
    assert calls == ["pa_attn_extend"], calls
    ref = DEC._extend_attention_ref(q[B - 1:].float(), cache.k[0][B - 1:, :n + T].float(),
                                    cache.v[0][B - 1:, :n + T].float(), torch.tensor([n]), 1.0 / math.sqrt(D))
    err = (o[B - 1:].float() - ref).abs().max() / ref.abs().max()
    assert float(err) < 1e-2, float(err)
    # the rows before it attend to their own chunk only
    ref0 = DEC._extend_attention_ref(q[:1].float(), cache.k[0][:1, :T].float(), cache.v[0][:1, :T].float(),
                                     torch.tensor([0]), 1.0 / math.sqrt(D))
    assert float((o[:1].float() - ref0).abs().max() / ref0.abs().max()) < 1e-2


# ---------------------------------------------------------------------- models
PROMPT_LENS = [23, 40, 9]
S = 40
_models = {}


def gpu_model(kind):
    """A bf16 model on the GPU, its fp32 CPU copy and one ragged [3, 40] prompt batch."""
    if kind not in _models:
        m = make_model(kind, dev, "bfloat16")
        ref = make_model(kind, "cpu", "float32")
        ref.load_state_dict({n: t.detach().float().cpu() for n, t in m.state_dict().items()})
        g = torch.Generator().manual_seed(21)
        ids = torch.zeros(3, S, dtype=torch.long)
        for b, n in enumerate(PROMPT_LENS):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        _models[kind] = (m, ref, ids)
    return _models[kind]


def new_cache(model, layout, max_len=64, **kw):
    if layout == "paged":
        return model.init_cache(3, max_len, paged=True, block_size=16, **kw)
    return model.init_cache(3, max_len, **kw)


@pytest.mark.parametrize("kind", MODELS)
def test_model_bit_equalities(kind):
    """prefill(chunk >= S) is prefill(); paged and contiguous give the same logits bits for
    extend and for chunked prefill; an e4m3 cache gives the bits of the twin run."""
    model, _, ids = gpu_model(kind)
    ids = ids.to(dev)
    nl = [4, 1, 6]
    turn = torch.randint(1, model.cfg.vocab_size, (3, 6), generator=torch.Generator().manual_seed(4)).to(dev)
    got = {}
    for layout in ("contiguous", "paged"):
        c = new_cache(model, layout)
        one = model.prefill(ids, c, PROMPT_LENS)
        for chunk in (S, S + 7):
            c2 = new_cache(model, layout)
            assert K.same_bits(model.prefill(ids, c2, PROMPT_LENS, chunk=chunk), one), (layout, chunk)
        c3 = new_cache(model, layout)
        with G8.knobs() as calls:
            chunked = model.prefill(ids, c3, PROMPT_LENS, chunk=16)
        assert "pa_attn_extend" in calls
        assert c3.lens.tolist() == PROMPT_LENS
        ext = model.extend(turn, c3, nl, all_logits=True)
        nxt = model.decode_step(ext[:, 0].float().argmax(-1), c3)
        got[layout] = (chunked, torch.stack([ext[b, n - 1] for b, n in enumerate(nl)]), nxt)
        assert c3.lens.tolist() == [n + m + 1 for n, m in zip(PROMPT_LENS, nl)]
    for name, a, b in zip(("chunked prefill", "extend", "next step"), got["contiguous"], got["paged"]):
        assert K.same_bits(a, b), f"{name}: paged != contiguous"

    def run8(layout, **kw):
        c = new_cache(model, layout, **kw)
        a = model.prefill(ids, c, PROMPT_LENS, chunk=16)
        e = model.extend(turn, c, nl, all_logits=True)
        return a, torch.stack([e[b, n - 1] for b, n in enumerate(nl)])

    for layout in ("contiguous", "paged"):
        got8 = run8(layout, kv_dtype="fp8_e4m3")
        with K.twin_append():
            want8 = run8(layout)
        for name, a, b in zip(("chunked prefill", "extend"), got8, want8):
            assert K.same_bits(a, b), f"{layout}, {name}: e4m3 cache != twin"


@pytest.mark.parametrize("kind", MODELS)
def test_chunked_prefill_accuracy(kind):
    """e0 = max |prefill() on the GPU - the fp32 CPU copy|, e1 the same for prefill(chunk=c),
    c in {3, 16}: e1 <= 2 e0 (another summation order in one of many equally rounded stages;
    a wrong mask, position or row mapping moves logits by the order of the logits).

    Observed on an MI355X: e1 / e0 = 1.00 for every kind, layout and chunk (e0 = e1 = 5.1e-3
    llama, 6.3e-3 llama-kv1, 5.6e-3 gpt, |logit| up to 1.2-1.5): the largest error is the bf16
    rounding of the same logit on both paths."""
    model, ref, ids = gpu_model(kind)
    with torch.no_grad():
        want = ref.prefill(ids, ref.init_cache(3, 64), PROMPT_LENS).float()
    e0 = float((model.prefill(ids.to(dev), new_cache(model, "contiguous"), PROMPT_LENS).float().cpu() - want).abs().max())
    for c in (3, 16):
        for layout in ("contiguous", "paged"):
            got = model.prefill(ids.to(dev), new_cache(model, layout), PROMPT_LENS, chunk=c).float().cpu()
            e1 = float((got - want).abs().max())
            print(f"{kind} {layout} chunk {c}: e0 {e0:.3e} e1 {e1:.3e} e1/e0 {e1 / e0:.2f} "
                  f"(logits up to {float(want.abs().max()):.2f})")
            assert e1 <= 2 * e0, (kind, layout, c, e0, e1)
