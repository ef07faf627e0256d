"""The fp8 (e4m3) KV cache on the CPU: the quantisation contract of ops/kv_fp8.py, the cache
objects and the plain-torch ``kv_append`` / ``decode_attention`` over them, and generation
against a twin run whose bf16-layout cache holds the quantise-dequantise image of every
appended token.  Everything is compared bit for bit; the one inequality is the contract's
error bound.  The helpers here are shared with tests/test_kv_fp8_gpu.py."""
import contextlib

import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import decode as D_
from test_generation_cpu import MODELS, make_model

FP8 = torch.float8_e4m3fn
KINDS = MODELS + ["llama-w8"]  # tiny llama (GQA, one kv head), tiny GPT, weight-quantised llama
PROMPT_LENS = [3, 7, 5]


def bits(t):
    """A tensor's bytes, for exact comparison (NaN payloads and the sign of zero included)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def random_vectors(n=4096, D=128, seed=0):
    """bf16 rows whose magnitudes are spread by exp(8 * randn)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, D, generator=g) * torch.exp(8 * torch.randn(n, 1, generator=g))).to(torch.bfloat16)


def adversarial_vectors(D=128):
    """bf16 [n, D]: the edges of the scale rule and of the code range, one per row, on top of a
    small random background that never holds the row's amax (a few rows replace it)."""
    g = torch.Generator().manual_seed(1)
    rows = []

    def row(amax, fill=None, at=5):
        if fill is not None:
            r = torch.full((D,), float(fill))
        else:
            r = torch.rand(D, generator=g) * 0.5 - 0.25
            if abs(amax) < float("inf"):  # neither inf nor NaN
                r = r * abs(amax)
        r[at] = amax
        rows.append(r)

    for e in (-20, -3, 0, 1, 9, 30):
        row(1.75 * 2.0 ** e)                # m == 1.75 exactly: the exponent stays
        row(-1.7578125 * 2.0 ** e, at=D - 1)  # one bf16 step above: plus one
        row(1.9921875 * 2.0 ** e)           # the largest mantissa
        row(2.0 ** e, at=0)                 # the smallest
    rows.append(torch.zeros(D))                                   # scale 1
    rows.append(-torch.zeros(D))
    row(float(torch.finfo(torch.bfloat16).max), fill=1.0)         # exponent clamps at +100
    row(2.0 ** 120, fill=-(2.0 ** 110))                           # above 448 * 2^100: saturates
    row(2.0 ** -110, fill=2.0 ** -112)                            # amax below 2^-100: clamps at -100
    row(2.0 ** -130, fill=-(2.0 ** -133))                         # bf16 subnormals
    row(float("inf"), fill=3.0)                                   # inf saturates, amax counts as finite
    row(float("-inf"), fill=-(2.0 ** 109), at=1)
    row(float("nan"))                                             # NaN is ignored by amax and kept as a code
    row(float("nan"), fill=0.0, at=2)                             # a zero vector apart from it
    r = torch.rand(D, generator=g)
    r[3], r[9], r[D - 2] = float("nan"), float("inf"), -448.0
    rows.append(r)
    return torch.stack(rows).to(torch.bfloat16)


def rule_scale(x):
    """The scale by the integer rule on the bits of amax (fp32): exponent - 8, plus one when
    the mantissa is above 1.75, clamped; 1 for zero.  Independent of frexp / log2."""
    a = x.float().abs()
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(-1).clamp(max=torch.finfo(torch.float32).max)
    b = amax.view(torch.int32)
    e = ((b >> 23) & 0xFF) - 127 - 8 + ((b & 0x7FFFFF) > 0x600000).int()
    e = torch.where(((b >> 23) & 0xFF) == 0, torch.full_like(e, -100), e).clamp(-100, 100)  # fp32 subnormal
    return torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))


# ---------------------------------------------------------------------- contract
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_scale_rule(dtype):
    for x in (random_vectors(), adversarial_vectors()):
        x = x.to(dtype)
        codes, scale = ops.quantize_kv_fp8(x)
        assert codes.dtype == FP8 and codes.shape == x.shape
        assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
        m, _ = torch.frexp(scale)
        assert bool((m == 0.5).all())  # powers of two
        assert same_bits(scale, rule_scale(x))
        assert float(scale.min()) >= 2.0 ** -100 and float(scale.max()) <= 2.0 ** 100


def test_scale_at_the_mantissa_edge():
    for e in (-20, 0, 9, 30):
        at, above = torch.zeros(2, 16), torch.zeros(2, 16)
        at[:, 4], above[:, 4] = 1.75 * 2.0 ** e, 1.7578125 * 2.0 ** e  # one bf16 step
        assert ops.quantize_kv_fp8(at.bfloat16())[1].tolist() == [2.0 ** (e - 8)] * 2
        assert ops.quantize_kv_fp8(above.bfloat16())[1].tolist() == [2.0 ** (e - 7)] * 2
    # ceil(log2(amax / 448)) in float64 wherever that is safely away from an integer
    x = random_vectors(512)
    amax = x.double().abs().amax(-1)
    lg = torch.log2(amax / 448)
    safe = (lg - lg.round()).abs() > 1e-6
    want = torch.ceil(lg).clamp(-100, 100)
    got = torch.log2(ops.quantize_kv_fp8(x)[1].double())
    assert torch.equal(got[safe], want[safe])


def test_zero_and_clamped_exponents():
    z = torch.zeros(2, 32, dtype=torch.bfloat16)
    codes, scale = ops.quantize_kv_fp8(z)
    assert scale.tolist() == [1.0, 1.0] and not bits(codes).any()
    big = torch.full((1, 32), torch.finfo(torch.bfloat16).max, dtype=torch.bfloat16)
    codes, scale = ops.quantize_kv_fp8(big)
    assert scale.item() == 2.0 ** 100 and bool((codes.float() == 448).all())
    tiny = torch.full((1, 32), 2.0 ** -110, dtype=torch.bfloat16)
    codes, scale = ops.quantize_kv_fp8(tiny)
    assert scale.item() == 2.0 ** -100 and bool((codes.float() == 0).all())  # 2^-10 ties to even: 0


def test_codes_error_bound_and_exact_dequant():
    x = random_vectors()
    codes, scale = ops.quantize_kv_fp8(x)
    assert not torch.isnan(codes.float()).any()
    dq = ops.dequantize_kv_fp8(codes, scale, torch.float32)
    # exactly representable in bf16: the two dequants agree, and bf16 -> fp32 is exact
    assert torch.equal(ops.dequantize_kv_fp8(codes, scale, torch.bfloat16).float(), dq)
    assert torch.equal(dq, codes.double().mul(scale.double().unsqueeze(-1)).float())
    err = (x.double() - dq.double()).abs()
    bound = torch.maximum(x.double().abs() * 2.0 ** -4, scale.double().unsqueeze(-1) * 2.0 ** -10)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(codes.float().abs().max()) <= 448
    # the edges too: exact in bf16 over the whole exponent range
    codes, scale = ops.quantize_kv_fp8(adversarial_vectors())
    dq = ops.dequantize_kv_fp8(codes, scale, torch.float32)
    dq16 = ops.dequantize_kv_fp8(codes, scale, torch.bfloat16).float()
    nan = torch.isnan(dq)
    assert torch.equal(torch.isnan(dq16), nan) and torch.equal(bits(dq16)[~nan], bits(dq)[~nan])  # -0 included


def test_finite_input_gives_no_nan_code():
    x = adversarial_vectors()
    codes, _ = ops.quantize_kv_fp8(x)
    assert torch.equal(torch.isnan(codes.float()), torch.isnan(x.float()))


def test_nan_is_kept_and_ignored():
    x = random_vectors(64, 32, seed=3)
    y = x.clone()
    hit = torch.zeros_like(x, dtype=torch.bool)
    hit[::3, 7] = True
    hit[5, :] = True  # a vector of NaN only: scale 1
    y[hit] = float("nan")
    x[hit] = 0
    cx, sx = ops.quantize_kv_fp8(x)
    cy, sy = ops.quantize_kv_fp8(y)
    assert same_bits(sx, sy) and sy[5].item() == 1.0
    assert bool(torch.isnan(cy.float())[hit].all())
    assert torch.equal(bits(cx)[~hit], bits(cy)[~hit])


def test_inf_saturates():
    x = torch.ones(3, 16, dtype=torch.bfloat16)
    x[0, 2], x[1, 3], x[2, 4] = float("inf"), float("-inf"), 2.0 ** 120
    codes, scale = ops.quantize_kv_fp8(x)
    assert scale.tolist() == [2.0 ** 100] * 3
    dq = ops.dequantize_kv_fp8(codes, scale, torch.bfloat16).float()
    top = 448 * 2.0 ** 100
    assert dq[0, 2].item() == top and dq[1, 3].item() == -top and dq[2, 4].item() == top
    assert not torch.isnan(dq).any()


def test_unknown_kv_dtype_raises():
    with pytest.raises(ValueError):
        ops.KVCache(1, 1, 8, 1, 16, kv_dtype="int8")
    with pytest.raises(ValueError):
        ops.PagedKVCache(1, 1, 8, 1, 16, kv_dtype="fp8_e5m2", block_size=16)
    model, ids = model_and_prompts("llama")
    with pytest.raises(ValueError):
        model.init_cache(2, 16, kv_dtype="fp8")
    with pytest.raises(ValueError):
        model.generate(ids, 2, kv_dtype="fp4")
    assert not ops.KVCache(1, 1, 8, 1, 16).quantized and ops.KVCache(1, 1, 8, 1, 16, kv_dtype=None).kv_dtype is None


# ---------------------------------------------------------------------- cache objects
def new_slots(cache, T, rows=None):
    """Flat indices, into the [slots, Hk, ...] view of a layer's storage, of the slots an append
    of T tokens at ``cache.lens`` writes (``rows``: the input-row -> cache-row map of a paged
    cache; tokens without a block are dropped)."""
    lens, dev = cache.lens.long(), cache.lens.device
    if not getattr(cache, "paged", False):
        pos = lens[:, None] + torch.arange(T, device=dev)
        return (torch.arange(cache.batch, device=dev)[:, None] * cache.max_len + pos).reshape(-1)
    crow = torch.arange(cache.batch, device=dev) if rows is None else rows.long().to(dev)
    pos = lens[crow][:, None] + torch.arange(T, device=dev)
    ok = pos < cache.max_len
    bs = cache.block_size
    blk = cache.block_table.long()[crow[:, None].expand_as(pos), (pos // bs).clamp(max=cache.max_blocks - 1)]
    ok = ok & (blk >= 0) & (blk < cache.num_blocks)
    return (blk * bs + pos % bs)[ok]


def flat(cache, t):
    """A layer's codes / values [.., Hk, D] or scales [.., Hk] with the slots flattened."""
    Hk = cache.num_kv_heads
    return t.view(-1, Hk, cache.head_dim) if t.dim() == 4 else t.view(-1, Hk)


def qdq(x):
    """The quantise-dequantise image of x [..., D], computed on the CPU."""
    c, s = ops.quantize_kv_fp8(x.cpu())
    return ops.dequantize_kv_fp8(c, s, x.dtype).to(x.device)


CODE_SENTINEL, SCALE_SENTINEL, VALUE_SENTINEL = 0x55, -7.5, -7.5


def make_caches(paged, B, S_max, Hk, D, lens, device="cpu", table=None, dtype=torch.bfloat16):
    """A quantised cache and its bf16 twin at the same lengths (and block table), every slot
    and scale holding a sentinel."""
    out = []
    for kv_dtype in ("fp8_e4m3", None):
        if paged:
            c = ops.PagedKVCache(1, B, S_max, Hk, D, dtype, device, block_size=16, kv_dtype=kv_dtype)
            if table is None:
                c.reserve(lens)
            else:
                c.load_block_table(table)
            c.set_lens(lens)
        else:
            c = ops.KVCache(1, B, S_max, Hk, D, dtype, device, kv_dtype=kv_dtype)
            c.set_lens(lens)
        if kv_dtype:
            for t in (c.k[0], c.v[0]):
                t.view(torch.uint8).fill_(CODE_SENTINEL)
            c.k_scale[0].fill_(SCALE_SENTINEL)
            c.v_scale[0].fill_(SCALE_SENTINEL)
        else:
            c.k[0].fill_(VALUE_SENTINEL)
            c.v[0].fill_(VALUE_SENTINEL)
        out.append(c)
    return out


def check_append_result(cq, cb, slots):
    """cq (quantised) against cb (bf16) after the same append, which wrote ``slots``: written
    slots hold quantize_kv_fp8 of what cb holds (any NaN code for a NaN), the rest the sentinel."""
    mask = torch.zeros(flat(cq, cq.k_scale[0]).shape[0], dtype=torch.bool)
    mask[slots.cpu()] = True
    for codes, scales, vals in ((cq.k[0], cq.k_scale[0], cb.k[0]), (cq.v[0], cq.v_scale[0], cb.v[0])):
        codes = flat(cq, codes.view(torch.uint8)).cpu()  # bytes: indexing is not defined on fp8
        scales, vals = flat(cq, scales).cpu(), flat(cb, vals).cpu()
        want_c, want_s = ops.quantize_kv_fp8(vals[mask])
        assert same_bits(scales[mask], want_s)
        got_c = codes[mask]
        nan = torch.isnan(want_c.float())
        assert torch.equal(torch.isnan(got_c.view(FP8).float()), nan)
        assert torch.equal(got_c[~nan], bits(want_c)[~nan])
        assert bool((codes[~mask] == CODE_SENTINEL).all()), "a stray store of codes"
        assert bool((scales[~mask] == SCALE_SENTINEL).all()), "a stray store of a scale"
        assert bool((vals[~mask] == VALUE_SENTINEL).all())


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("paged", [False, True])
def test_kv_append_quantises_what_the_bf16_cache_holds(paged, T, rotary):
    torch.manual_seed(T)
    B, Hq, Hk, D, S_max, lens = 3, 4, 2, 32, 40, [0, 7, 33]
    cos, sin = ops.rope_tables(64, D) if rotary else (None, None)
    qkv = (torch.randn(B, T, (Hq + 2 * Hk) * D) * torch.exp(3 * torch.randn(B, T, 1))).bfloat16()
    cq, cb = make_caches(paged, B, S_max, Hk, D, lens)
    q = ops.kv_append(qkv, cq, 0, Hq, Hk, cos, sin)
    want_q = ops.kv_append(qkv, cb, 0, Hq, Hk, cos, sin)
    slots = new_slots(cb, T)  # after the append: a paged one reserves the blocks it needs
    assert same_bits(q, want_q) and slots.numel() == B * T
    check_append_result(cq, cb, slots)
    # dequant (and gather) return codes * scale in the cache's dtype, in the slab's layout
    assert cq.quantized and cq.dtype == torch.bfloat16 and cq.k[0].dtype == FP8
    k, v = cq.dequant(0)
    assert k.shape == (B, S_max, Hk, D) and k.dtype == torch.bfloat16
    wk, wv = cb.gather(0) if paged else (cb.k[0], cb.v[0])
    for b, n in enumerate(lens):
        assert same_bits(k[b, n:n + T], qdq(wk[b, n:n + T])) and same_bits(v[b, n:n + T], qdq(wv[b, n:n + T]))
    if paged:
        gk, gv = cq.gather(0)
        assert same_bits(gk, k) and same_bits(gv, v)
    assert cq.nbytes == 2 * (cq.num_blocks * 16 if paged else B * S_max) * Hk * (D + 4)  # codes plus scales


def test_dropped_tokens_write_nothing():
    """A paged row whose table has no block for some of the new tokens (and one mapped by
    ``rows``): the dropped tokens leave codes and scales alone."""
    B, T, Hq, Hk, D, S_max = 3, 5, 2, 1, 32, 40
    table = torch.tensor([[4, 1, -1], [6, -1, -1], [0, 2, 5]], dtype=torch.int32)
    lens = [14, 14, 30]  # row 1: positions 16..18 have no block
    qkv = torch.randn(2, T, (Hq + 2 * Hk) * D).bfloat16()
    cq, cb = make_caches(True, B, S_max, Hk, D, lens, table=table)
    rows = torch.tensor([1, 2], dtype=torch.int32)
    slots = new_slots(cb, T, rows)
    assert slots.numel() == 2 + 5
    for c in (cq, cb):
        with c.prefilling([1, 2]):
            ops.kv_append(qkv, c, 0, Hq, Hk)
    check_append_result(cq, cb, slots)
    # a slot never written by anyone dequantises to 0: fresh caches have zero scales
    fresh = ops.PagedKVCache(1, 2, 32, 1, 16, block_size=16, kv_dtype="fp8_e4m3")
    fresh.reserve([20, 3])
    assert not fresh.dequant(0)[0].any() and not ops.KVCache(1, 2, 8, 1, 16, kv_dtype="fp8_e4m3").dequant(0)[1].any()


@pytest.mark.parametrize("paged", [False, True])
def test_decode_attention_is_the_reference_over_dequant(paged):
    torch.manual_seed(2)
    B, Hq, Hk, D, S_max, lens = 3, 4, 2, 32, 40, [1, 9, 33]
    cq, _ = make_caches(paged, B, S_max, Hk, D, [0, 0, 0])
    for t in (cq.k_scale[0], cq.v_scale[0]):
        t.zero_()
    qkv = torch.randn(B, 36, (Hq + 2 * Hk) * D).bfloat16()
    ops.kv_append(qkv, cq, 0, Hq, Hk)
    q = torch.randn(B, 1, Hq, D).bfloat16()
    kv_len = torch.tensor(lens, dtype=torch.int32)
    o = ops.decode_attention(q, cq, 0, kv_len=kv_len)
    k, v = cq.dequant(0)
    want = D_._decode_attention_ref(q, k, v, kv_len, D ** -0.5)
    assert same_bits(o, want) and o.dtype == torch.bfloat16 and bool(o.float().abs().sum() > 0)


# ---------------------------------------------------------------------- models
_models = {}


def model_and_prompts(kind, device="cpu", dtype="float32"):
    """One model and one ragged right-padded prompt batch per kind, shared and left unchanged
    (tests/test_decode_graph_cpu.py's, plus a weight-quantised llama)."""
    key = (kind, device, dtype)
    if key not in _models:
        m = make_model("llama" if kind == "llama-w8" else kind, device, dtype)
        if kind == "llama-w8":
            m.quantize_weights()
        g = torch.Generator().manual_seed(3)
        ids = torch.zeros(3, 7, dtype=torch.long)
        for b, n in enumerate(PROMPT_LENS):
            ids[b, :n] = torch.randint(1, m.cfg.vocab_size, (n,), generator=g)
        _models[key] = (m, ids.to(device))
    return _models[key]


@contextlib.contextmanager
def twin_append():
    """``ops.kv_append`` appends to the (unquantised) cache and then overwrites the new slots
    with their quantise-dequantise image: the cache holds what a quantised one dequantises to."""
    orig = ops.kv_append

    def append(qkv, cache, layer, num_heads, num_kv_heads=None, cos=None, sin=None, rows=None):
        assert not cache.quantized
        q = orig(qkv, cache, layer, num_heads, num_kv_heads, cos, sin, rows)
        rows_t = getattr(cache, "_prefill_rows", None)
        if rows is not None:
            rows_t = torch.tensor([int(r) for r in rows])
        slots = new_slots(cache, qkv.shape[1], rows_t)  # after the call: a paged append may reserve
        for t in (cache.k[layer], cache.v[layer]):
            f = flat(cache, t)
            f[slots] = qdq(f[slots])
        return q

    ops.kv_append = append
    try:
        yield
    finally:
        ops.kv_append = orig


@contextlib.contextmanager
def recorded_logits(model):
    """Every ``_lm_logits`` result of ``model`` inside (the prefill's, then one per step)."""
    seen, orig = [], model._lm_logits
    model._lm_logits = lambda y: seen.append(orig(y).clone()) or seen[-1]
    try:
        yield seen
    finally:
        del model._lm_logits


def run_generate(model, ids, new_tokens, **kw):
    with recorded_logits(model) as logits:
        toks, lengths = model.generate(ids, new_tokens, prompt_lens=PROMPT_LENS, **kw)
    return toks, lengths, logits


def check_against_twin(model, ids, cache, new_tokens=12):
    kw = dict(cache=cache, block_size=16) if cache == "paged" else dict(cache=cache)
    toks, lengths, logits = run_generate(model, ids, new_tokens, kv_dtype="fp8_e4m3", **kw)
    with twin_append():
        want, want_len, want_logits = run_generate(model, ids, new_tokens, **kw)
    assert torch.equal(toks, want) and torch.equal(lengths, want_len)
    assert len(logits) == len(want_logits) == new_tokens
    for step, (a, b) in enumerate(zip(logits, want_logits)):
        assert same_bits(a, b), f"logits of step {step}"
    return toks, lengths


@pytest.mark.parametrize("cache", ["contiguous", "paged"])
@pytest.mark.parametrize("kind", KINDS)
def test_generate_equals_the_twin(kind, cache):
    model, ids = model_and_prompts(kind)
    toks, lengths = check_against_twin(model, ids, cache)
    kw = dict(cache=cache, block_size=16) if cache == "paged" else dict(cache=cache)
    g_toks, g_len = model.generate(ids, 12, prompt_lens=PROMPT_LENS, kv_dtype="fp8_e4m3", graph=True, **kw)
    assert torch.equal(g_toks, toks) and torch.equal(g_len, lengths)


def pool_bytes(cache):
    return cache._pool.view(torch.uint8).clone(), cache._scale_pool.clone()


def test_readmitting_a_row_leaves_the_others_alone():
    model, ids = model_and_prompts("llama")
    cache = model.init_cache(3, 24, paged=True, block_size=16, kv_dtype="fp8_e4m3")
    assert cache.quantized and cache.dtype == torch.float32
    model.prefill(ids, cache, PROMPT_LENS)
    codes, scales = pool_bytes(cache)
    keep = [b for r in (0, 2) for b in cache.row_blocks(r)]
    cache.free_rows([1])
    model.prefill(ids[2:3], cache, [5], rows=[1])
    codes2, scales2 = pool_bytes(cache)
    assert torch.equal(codes[:, :, keep], codes2[:, :, keep])
    assert torch.equal(bits(scales[:, :, keep]), bits(scales2[:, :, keep]))
    assert cache.host_lens == [3, 5, 5]
    k, v = cache.dequant(0)
    assert same_bits(k[1, :5], k[2, :5]) and same_bits(v[1, :5], v[2, :5])  # the same prompt, requantised
