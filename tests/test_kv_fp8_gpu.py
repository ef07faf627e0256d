"""The e4m3 KV-cache kernels of csrc/kernels/attn_decode.hip against the plain-torch contract
(ops/kv_fp8.py) and against the bf16 kernels, bit for bit:

  append     codes, scales == quantize_kv_fp8(what pa_kv_append[_paged] stores), q == its q
  attention  pa_attn_decode_f8 == pa_attn_decode over a bf16 cache holding the dequantised
             values; the paged kernel == the contiguous one; both within the oracle's bound
  models     generate(kv_dtype="fp8_e4m3") == the twin run of tests/test_kv_fp8_cpu.py
"""
import contextlib
import math

import pytest
import torch

import attn_oracle as AO
import test_kv_fp8_cpu as K
from paddle_amd import ops
from paddle_amd.ops import _native
from paddle_amd.ops import decode as DEC

pytestmark = pytest.mark.gpu

dev = "cuda"
FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7F


@contextlib.contextmanager
def knobs():
    """Yields the list of native calls made inside (the spy of test_attention_oracle_gpu.py)."""
    calls = []
    orig = _native.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    try:
        _native.call = spy
        yield calls
    finally:
        _native.call = orig


# ---------------------------------------------------------------------- append
# paged: 4 cache rows, input row i -> cache row ROWS[i]; a shuffled table; cache row 2 has no
# second block, so its tokens at positions 16.. are dropped
TABLE = [[9, 4, 11], [2, 7, -1], [5, -1, -1], [10, 0, 6]]
ROWS = [2, 0, 3]
PAGED_LENS = [9, 3, 14, 30]  # cache rows; row 1 is not appended to
SLAB_LENS = [0, 14, 33]


def run_append(paged, qkv, Hq, Hk, D, cos, sin):
    """The same append into a quantised cache and a bf16 one, both on the kernels."""
    B, T = qkv.shape[:2]
    if paged:
        cq, cb = K.make_caches(True, 4, 40, Hk, D, PAGED_LENS, dev, table=torch.tensor(TABLE, dtype=torch.int32))
    else:
        cq, cb = K.make_caches(False, B, 40, Hk, D, SLAB_LENS, dev)
    out = []
    for c, name in ((cq, "pa_kv_append_paged_f8" if paged else "pa_kv_append_f8"),
                    (cb, "pa_kv_append_paged" if paged else "pa_kv_append")):
        with knobs() as calls:
            if paged:
                with c.prefilling(ROWS):
                    out.append(ops.kv_append(qkv, c, 0, Hq, Hk, cos, sin))
            else:
                out.append(ops.kv_append(qkv, c, 0, Hq, Hk, cos, sin))
        assert calls == [name], calls
    slots = K.new_slots(cb, T, torch.tensor(ROWS) if paged else None)
    assert K.same_bits(out[0], out[1]), "q differs from the bf16 kernel's"
    K.check_append_result(cq, cb, slots)
    return slots


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("Hq,Hk", [(4, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_append_kernel(D, Hq, Hk, T, rotary, paged):
    torch.manual_seed(D + T)
    B = 3
    cos, sin = ops.rope_tables(64, D, device=dev) if rotary else (None, None)
    wide = torch.randn(B, T, (Hq + 2 * Hk) * D + 64) * torch.exp(3 * torch.randn(B, T, 1))
    qkv = wide.to(dev, torch.bfloat16)[:, :, 32:32 + (Hq + 2 * Hk) * D]  # a column slice: strided rows
    slots = run_append(paged, qkv, Hq, Hk, D, cos, sin)
    # paged, T = 5: cache row 2 keeps positions 14, 15 and drops 16..18
    assert slots.numel() == (B * T if not paged or T == 1 else B * T - 3)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_append_kernel_adversarial_vectors(D, paged):
    """The edges of the contract through the kernel, rotary off: the input is the stored value."""
    adv = K.adversarial_vectors(D)
    B, T, Hq, Hk = 3, 5, 2, 2
    n = B * T * Hk
    assert 2 * n >= adv.shape[0]
    idx = torch.arange(2 * n) % adv.shape[0]
    kv = adv[idx].view(2, B, T, Hk, D)  # every vector at least once, among the k and the v heads
    q = torch.randn(B, T, Hq, D).bfloat16()
    qkv = torch.cat([q, kv[0], kv[1]], 2).reshape(B, T, -1).to(dev)
    run_append(paged, qkv, Hq, Hk, D, None, None)


def test_append_refused_head_size_takes_the_reference():
    B, T, Hq, Hk, D = 2, 3, 2, 1, 48  # three lanes per vector: not a power of two
    assert not _native.lib().pa_kv_append_f8_ok(D) and _native.lib().pa_kv_append_f8_ok(128)
    qkv = torch.randn(B, T, (Hq + 2 * Hk) * D, device=dev, dtype=torch.bfloat16)
    cq, cb = K.make_caches(False, B, 16, Hk, D, [0, 5], dev)
    with knobs() as calls:
        q = ops.kv_append(qkv, cq, 0, Hq, Hk)
    assert calls == []
    assert K.same_bits(q, ops.kv_append(qkv, cb, 0, Hq, Hk))
    K.check_append_result(cq, cb, K.new_slots(cb, T))


# ---------------------------------------------------------------------- attention
KV_LEN = [1, 2, 63, 65, 257]
S_MAX = 264
SPLITS = (1, 2, 5, 64)


def poisoned_fp8_slab(Hk, D):
    c = ops.KVCache(1, len(KV_LEN), S_MAX, Hk, D, torch.bfloat16, dev, kv_dtype="fp8_e4m3")
    for t in (c.k[0], c.v[0]):
        t.view(torch.uint8).fill_(NAN_CODE)
    c.k_scale[0].fill_(float("inf"))
    c.v_scale[0].fill_(float("inf"))
    return c


def poisoned_fp8_pool(Hk, D, bs, seed):
    """A paged e4m3 cache with a shuffled, fully assigned table except pool block 0, which no
    row owns; every slot holds NaN codes and an inf scale."""
    B = len(KV_LEN)
    mb = -(-S_MAX // bs)
    c = ops.PagedKVCache(1, B, S_MAX, Hk, D, torch.bfloat16, dev, block_size=bs, num_blocks=B * mb + 1,
                         kv_dtype="fp8_e4m3")
    g = torch.Generator().manual_seed(seed)
    c.load_block_table((torch.randperm(B * mb, generator=g) + 1).view(B, mb).int())
    c._pool.view(torch.uint8).fill_(NAN_CODE)
    c._scale_pool.fill_(float("inf"))
    return c


def pool_slots(c, b, n):
    """Flat pool slots of the first n tokens of row b."""
    t = torch.arange(n)
    return (c.host_table[b].long()[t // c.block_size] * c.block_size + t % c.block_size).to(dev)


def store_row(c, b, kq, ks, vq, vs):
    """Codes [n, Hk, D] / scales [n, Hk] of row b's first n tokens into either cache."""
    n = kq.shape[0]
    for codes, scales, q8, s in ((c.k[0], c.k_scale[0], kq, ks), (c.v[0], c.v_scale[0], vq, vs)):
        if getattr(c, "paged", False):
            sl = pool_slots(c, b, n)
            K.flat(c, codes.view(torch.uint8))[sl] = q8.view(torch.uint8).to(dev)
            K.flat(c, scales)[sl] = s.to(dev)
        else:
            codes.view(torch.uint8)[b, :n] = q8.view(torch.uint8).to(dev)
            scales[b, :n] = s.to(dev)


def quantised_case(profile, Hq, Hk, D, scale):
    """Per row of KV_LEN: the oracle's q and its k / v quantised by the reference."""
    rows = []
    for b, n in enumerate(KV_LEN):
        q, k, v, do = AO.make_inputs(profile, 1, 1, n, Hq, Hk, D, scale, seed=b)
        (kq, ks), (vq, vs) = ops.quantize_kv_fp8(k[0]), ops.quantize_kv_fp8(v[0])
        dk = ops.dequantize_kv_fp8(kq, ks, torch.bfloat16)
        dv = ops.dequantize_kv_fp8(vq, vs, torch.bfloat16)
        rows.append(dict(q=q, do=do, kq=kq, ks=ks, vq=vq, vs=vs, dk=dk, dv=dv))
    return rows


@pytest.mark.parametrize("D,Hq,Hk", [(128, 8, 2), (128, 4, 1), (64, 2, 2), (128, 8, 1)])
def test_attention_kernel(D, Hq, Hk):
    """(a) the bits of the bf16 kernel over the dequantised values, finite; (b) the oracle's
    bound against the float64 reference on the dequantised values; (c) the paged kernel at
    block 16 and 64 returns the contiguous kernel's bits; (e) a second run returns the same."""
    fails, worst = [], 0.0
    kv_len = torch.tensor(KV_LEN, dtype=torch.int32, device=dev)
    for pi, profile in enumerate(AO.PROFILES):
        for f in AO.SCALE_FACTORS:
            scale = f / math.sqrt(D)
            rows = quantised_case(profile, Hq, Hk, D, scale)
            c8 = poisoned_fp8_slab(Hk, D)
            pools = [poisoned_fp8_pool(Hk, D, bs, seed=pi) for bs in (16, 64)]
            c16 = ops.KVCache(1, len(KV_LEN), S_MAX, Hk, D, torch.bfloat16, dev)  # the poison removed: zeros
            for b, r in enumerate(rows):
                for c in [c8] + pools:
                    store_row(c, b, r["kq"], r["ks"], r["vq"], r["vs"])
                c16.k[0][b, :KV_LEN[b]] = r["dk"].to(dev)
                c16.v[0][b, :KV_LEN[b]] = r["dv"].to(dev)
            dk, dv = c8.dequant(0)
            for b, r in enumerate(rows):
                assert K.same_bits(dk[b, :KV_LEN[b]].cpu(), r["dk"]) and K.same_bits(dv[b, :KV_LEN[b]].cpu(), r["dv"])
            q = torch.cat([r["q"] for r in rows]).to(dev)
            refs = [AO.reference(r["q"], r["dk"][None], r["dv"][None], r["do"], False, scale) for r in rows]
            ref = {n: torch.cat([x[n] for x in refs]) for n in ("O", "magO")}
            for ns in SPLITS:
                with knobs() as calls:
                    o = ops.decode_attention(q, c8, 0, scale=scale, num_splits=ns, kv_len=kv_len)
                assert calls == ["pa_attn_decode_f8"], calls
                assert torch.isfinite(o).all(), (profile, f, ns)
                with knobs() as calls:
                    want = ops.decode_attention(q, c16, 0, scale=scale, num_splits=ns, kv_len=kv_len)
                assert calls == ["pa_attn_decode"], calls
                assert K.same_bits(o, want), f"{profile} x{f} splits {ns}: fp8 != bf16 over the dequantised cache"
                st = AO.stats(dict(O=o), ref)["O"]
                worst = max(worst, st)
                if not st <= AO.BOUND:
                    fails.append((profile, f, ns, st))
                for pg in pools:
                    with knobs() as calls:
                        op = ops.decode_attention(q, pg, 0, scale=scale, num_splits=ns, kv_len=kv_len)
                    assert calls == ["pa_attn_decode_paged_f8"], calls
                    assert K.same_bits(op, o), f"{profile} x{f} splits {ns} block {pg.block_size}: paged != contiguous"
                assert K.same_bits(ops.decode_attention(q, c8, 0, scale=scale, num_splits=ns, kv_len=kv_len), o)
    print(f"decode_f8<{D}> Hq {Hq} Hk {Hk}: worst O {worst:.2e} (bound {AO.BOUND:.2e})")
    assert not fails, fails[:8]


def _filled(profile="flat", D=128, Hq=8, Hk=2, bs=16):
    scale = 1.0 / math.sqrt(D)
    rows = quantised_case(profile, Hq, Hk, D, scale)
    c8, pg = poisoned_fp8_slab(Hk, D), poisoned_fp8_pool(Hk, D, bs, seed=7)
    for b, r in enumerate(rows):
        for c in (c8, pg):
            store_row(c, b, r["kq"], r["ks"], r["vq"], r["vs"])
    q = torch.cat([r["q"] for r in rows]).to(dev)
    return rows, c8, pg, q, scale


def test_attention_out_of_range_table_entry_is_masked():
    """(d) keys below kv_len whose table entry is out of range are masked while pool slot 0,
    which their lanes read instead, holds NaN codes and an inf scale."""
    D, Hq, Hk, bs = 128, 8, 2, 16
    rows, _, pg, q, scale = _filled(D=D, Hq=Hq, Hk=Hk, bs=bs)
    assert bool((pg.k[0].view(torch.uint8)[0] == NAN_CODE).all()) and bool(torch.isinf(pg.v_scale[0][0]).all())
    kv_len = torch.tensor(KV_LEN, dtype=torch.int32, device=dev)
    pg.block_table[4, 2] = pg.num_blocks  # row 4 (257 keys) loses keys 32..47 and 240..255
    pg.block_table[4, 15] = -5
    pg.block_table[3, 0] = pg.num_blocks + 9  # row 3 (65 keys) loses keys 0..15
    # the bf16 paged kernel over the dequantised pool, with the same table
    p16 = ops.PagedKVCache(1, len(KV_LEN), S_MAX, Hk, D, torch.bfloat16, dev, block_size=bs,
                           num_blocks=pg.num_blocks)
    p16.load_block_table(pg.host_table)
    p16.block_table.copy_(pg.block_table)
    for b, r in enumerate(rows):
        sl = pool_slots(pg, b, KV_LEN[b])
        K.flat(p16, p16.k[0])[sl] = r["dk"].to(dev)
        K.flat(p16, p16.v[0])[sl] = r["dv"].to(dev)
    for ns in (1, 2, 5):
        with knobs() as calls:
            o = ops.decode_attention(q, pg, 0, scale=scale, num_splits=ns, kv_len=kv_len)
        assert calls == ["pa_attn_decode_paged_f8"], calls
        assert torch.isfinite(o).all()
        assert K.same_bits(o, ops.decode_attention(q, p16, 0, scale=scale, num_splits=ns, kv_len=kv_len))
        for b, gone in ((4, list(range(32, 48)) + list(range(240, 256))), (3, list(range(16)))):
            keep = torch.ones(KV_LEN[b], dtype=torch.bool)
            keep[gone] = False
            r = rows[b]
            ref = DEC._decode_attention_ref(r["q"].float(), r["dk"][None][:, keep].float(), r["dv"][None][:, keep].float(),
                                            torch.tensor([int(keep.sum())]), scale)
            err = (o[b:b + 1].float().cpu() - ref).abs().max() / ref.abs().max()
            assert float(err) < 1e-2, (ns, b, float(err))


def test_attention_no_keys_gives_zeros():
    """(f) kv_len 0, and a negative one."""
    _, c8, pg, q, scale = _filled()
    kv_len = torch.tensor([0, 2, 0, -3, 257], dtype=torch.int32, device=dev)
    for c in (c8, pg):
        for ns in (1, 5):
            o = ops.decode_attention(q, c, 0, scale=scale, num_splits=ns, kv_len=kv_len)
            assert torch.isfinite(o).all() and not o[[0, 2, 3]].any() and bool(o[[1, 4]].any())


@pytest.mark.parametrize("D,Hq,Hk", [(128, 6, 1), (96, 2, 2)])
@pytest.mark.parametrize("paged", [False, True])
def test_attention_refused_shapes_take_the_reference(D, Hq, Hk, paged):
    """(g) shapes pa_attn_decode_f8_ok refuses."""
    torch.manual_seed(0)
    B, S_max, lens = 2, 40, [7, 33]
    qst = DEC.ctypes_long_array([Hq * D, D])
    assert not _native.lib().pa_attn_decode_f8_ok(B, S_max, Hq, Hk, D, 1, qst)
    assert not _native.lib().pa_attn_decode_paged_f8_ok(B, S_max, Hq, Hk, D, 1, qst, 16, 3, 6)
    kw = dict(block_size=16) if paged else {}
    c = (ops.PagedKVCache if paged else ops.KVCache)(1, B, S_max, Hk, D, torch.bfloat16, dev, kv_dtype="fp8_e4m3", **kw)
    qkv = torch.randn(B, 34, (Hq + 2 * Hk) * D, device=dev, dtype=torch.bfloat16)
    ops.kv_append(qkv, c, 0, Hq, Hk)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    with knobs() as calls:
        o = ops.decode_attention(q, c, 0, kv_len=kv_len)
    assert not [n for n in calls if "attn_decode" in n], calls
    k, v = c.dequant(0)
    want = DEC._decode_attention_ref(q, k, v, kv_len, 1.0 / math.sqrt(D))
    assert K.same_bits(o, want) and bool(o.any())


# ---------------------------------------------------------------------- models
@pytest.mark.parametrize("cache", ["contiguous", "paged"])
@pytest.mark.parametrize("kind", K.KINDS)
def test_generate_equals_the_twin(kind, cache):
    model, ids = K.model_and_prompts(kind, dev, "bfloat16")
    kw = dict(cache=cache, block_size=16) if cache == "paged" else dict(cache=cache)
    with knobs() as calls:
        toks, lengths = K.check_against_twin(model, ids, cache)
    f8 = [n for n in calls if n.endswith("_f8")]
    tail = "_paged_f8" if cache == "paged" else "_f8"
    assert set(f8) == {"pa_kv_append" + tail, "pa_attn_decode" + tail}, set(calls)
    g_toks, g_len = model.generate(ids, 12, prompt_lens=K.PROMPT_LENS, kv_dtype="fp8_e4m3", graph=True, **kw)
    p_toks, p_len = model.generate(ids, 12, prompt_lens=K.PROMPT_LENS, kv_dtype="fp8_e4m3", sampler="philox", **kw)
    assert torch.equal(g_toks, p_toks) and torch.equal(g_len, p_len)
    assert torch.equal(g_toks, toks) and torch.equal(g_len, lengths)


def test_replacing_a_row_mid_run_leaves_the_others_alone():
    model, ids = K.model_and_prompts("llama", dev, "bfloat16")
    tok = torch.tensor([5, 9, 11], device=dev)

    def run(replace):
        cache = model.init_cache(3, 32, paged=True, block_size=16, kv_dtype="fp8_e4m3")
        model.prefill(ids, cache, K.PROMPT_LENS)
        for _ in range(3):
            model.decode_step(tok, cache)
        if replace:
            model.prefill(ids[0:1, :3], cache, [3], rows=[1])
        return model.decode_step(tok, cache)

    a, b = run(False), run(True)
    assert K.same_bits(a[[0, 2]], b[[0, 2]]) and not torch.equal(a[1], b[1])
