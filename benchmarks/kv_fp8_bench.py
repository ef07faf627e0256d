"""What the fp8 (e4m3) KV cache buys: ``ops.decode_attention`` over a quantised cache against
the same call over the bf16 cache, in one process, for

    B in {1, 8}  x  Hq/Hk in {32/32, 32/8}  x  D = 128  x  cached length in {2048, 8192}
    x  {contiguous, paged with blocks of 64}

with the same ``num_splits`` on both sides.  The ceiling from bytes alone is
2 D / (D + 4) = 256 / 132 = 1.94x at D 128: per key and kv head the bf16 cache reads 2 D bytes
of K and as many of V, the fp8 cache D codes and one 4-byte scale of each.

Method (that of paged_decode_bench.py): every variant rotates over a set of caches larger
than twice the 256 MiB last-level cache *in fp8 bytes*, so both dtypes read from HBM; the
calls of one pass are captured once into a HIP graph and the replay is timed with HIP events.
Every graph is warmed up, then ``--repeats`` rounds each time every variant once (bf16, fp8,
bf16 paged, fp8 paged: interleaved, so drift hits all alike) over a window of at least
``--window-ms``.  Reported: the median over the rounds; the bf16 kernel's run-to-run spread
is (max - min) / median of its rounds.  The goal at a shape is met when the fp8 median is
below the bf16 median by more than that spread.  Before any timing the fp8 output is checked
bit-equal to the bf16 kernel over a cache holding the dequantised values, and the paged fp8
output to the contiguous one.

Also: ``kv_append`` at T = 1 (``--append``), one llama-7b ``decode_step`` at context 512 and
4096 as a launch loop and as a graph replay, a 512-token prefill and the cache bytes
(``--step``), and the greedy-token agreement with the bf16 cache on the tiny test models
(``--agree``).

    python benchmarks/kv_fp8_bench.py --append --step --agree --md kv_fp8_bench_table.md
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddle_amd import ops  # noqa: E402
from paddle_amd.ops.paged import DEFAULT_BLOCK_SIZE  # noqa: E402
from benchmarks.paged_decode_bench import LLC_BYTES, Variant, shuffled_table  # noqa: E402

FP8 = torch.float8_e4m3fn
KV = "fp8_e4m3"


def _spread(us):
    return round(100 * (max(us) - min(us)) / statistics.median(us), 2)


def _quantise_layer(x, chunk=1 << 22):
    """quantize_kv_fp8 of a big [.., Hk, D] tensor in pieces (the reference makes fp32 copies)."""
    flat = x.reshape(-1, x.shape[-1])
    codes = torch.empty(flat.shape, dtype=FP8, device=x.device)
    scale = torch.empty(flat.shape[0], dtype=torch.float32, device=x.device)
    for i in range(0, flat.shape[0], chunk):
        c, s = ops.quantize_kv_fp8(flat[i:i + chunk])
        codes[i:i + chunk], scale[i:i + chunk] = c, s
    return codes.view(x.shape), scale.view(x.shape[:-1])


@torch.no_grad()
def bench_shape(B, Hq, Hk, D, L, repeats, window_ms, bs=DEFAULT_BLOCK_SIZE, dev="cuda"):
    f8_bytes = 2 * B * L * Hk * (D + 4)
    bf_bytes = 2 * B * L * Hk * D * 2
    n = max(2, math.ceil(2 * LLC_BYTES / f8_bytes) + 1)  # rotating set > 2x the last-level cache, in fp8 bytes
    ns = ops.decode.default_num_splits(B, Hk, L)
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    slab = ops.KVCache(n, B, L, Hk, D, torch.bfloat16, dev)
    slab8 = ops.KVCache(n, B, L, Hk, D, torch.bfloat16, dev, kv_dtype=KV)
    for i in range(n):
        slab.k[i].normal_()
        slab.v[i].normal_()
        for src, codes, scales in ((slab.k[i], slab8.k[i], slab8.k_scale[i]), (slab.v[i], slab8.v[i], slab8.v_scale[i])):
            c, s = _quantise_layer(src)
            codes.copy_(c)
            scales.copy_(s)
    # the contract, before any timing: the bits of the bf16 kernel over the dequantised values
    twin = ops.KVCache(1, B, L, Hk, D, torch.bfloat16, dev)
    dk, dv = slab8.dequant(0)
    twin.k[0].copy_(dk)
    twin.v[0].copy_(dv)
    want = ops.decode_attention(q, twin, 0, num_splits=ns, kv_len=kv_len)
    got = ops.decode_attention(q, slab8, 0, num_splits=ns, kv_len=kv_len)
    if not torch.equal(got, want):
        raise SystemExit(f"fp8 and bf16-over-dequant outputs differ at {(B, Hq, Hk, D, L)}")
    del twin, dk, dv
    pg = ops.PagedKVCache(n, B, L, Hk, D, torch.bfloat16, dev, block_size=bs, zero_fill=False)
    pg8 = ops.PagedKVCache(n, B, L, Hk, D, torch.bfloat16, dev, block_size=bs, zero_fill=False, kv_dtype=KV)
    table = shuffled_table(B, pg.max_blocks, pg.num_blocks, seed=bs)
    pg.load_block_table(table)
    pg8.load_block_table(table)
    idx = torch.tensor(table, device=dev).reshape(-1)  # (b, j) -> block id
    nb = B * pg.max_blocks
    for i in range(n):
        pg.k[i][idx] = slab.k[i].reshape(nb, bs, Hk, D)
        pg.v[i][idx] = slab.v[i].reshape(nb, bs, Hk, D)
        for a, b_ in ((pg8.k, slab8.k), (pg8.v, slab8.v)):
            a[i].view(torch.uint8)[idx] = b_[i].view(torch.uint8).reshape(nb, bs, Hk, D)
        pg8.k_scale[i][idx] = slab8.k_scale[i].reshape(nb, bs, Hk)
        pg8.v_scale[i][idx] = slab8.v_scale[i].reshape(nb, bs, Hk)
    if not torch.equal(ops.decode_attention(q, pg8, 0, num_splits=ns, kv_len=kv_len), got):
        raise SystemExit(f"paged fp8 and contiguous fp8 outputs differ at {(B, Hq, Hk, D, L)}")
    caches = dict(bf16=slab, fp8=slab8, bf16_paged=pg, fp8_paged=pg8)
    variants = {name: Variant(name, [lambda i=i, c=c: ops.decode_attention(q, c, i, num_splits=ns, kv_len=kv_len)
                                     for i in range(n)]) for name, c in caches.items()}
    for v in variants.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants.values():
            v.measure()
    med = {k: statistics.median(v.us) for k, v in variants.items()}
    out = dict(B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, num_splits=ns, rotating_caches=n, repeats=repeats, block_size=bs,
               bit_equal=True, timing="graph replay")
    for tag, a, b_ in (("", "bf16", "fp8"), ("paged_", "bf16_paged", "fp8_paged")):
        sp = _spread(variants[a].us)
        out.update({
            f"{tag}bf16_us": round(med[a], 2), f"{tag}bf16_min_us": round(min(variants[a].us), 2),
            f"{tag}bf16_max_us": round(max(variants[a].us), 2), f"{tag}bf16_spread_pct": sp,
            f"{tag}bf16_TB_per_s": round(bf_bytes / (med[a] * 1e-6) / 1e12, 3),
            f"{tag}fp8_us": round(med[b_], 2), f"{tag}fp8_spread_pct": _spread(variants[b_].us),
            f"{tag}fp8_TB_per_s": round(f8_bytes / (med[b_] * 1e-6) / 1e12, 3),
            f"{tag}speedup": round(med[a] / med[b_], 3),
            f"{tag}goal_met": bool(med[b_] < med[a] * (1 - sp / 100)),
        })
    return out


@torch.no_grad()
def bench_append(B, Hq, Hk, D, repeats, window_ms, layers=32, S_max=4096, pos=2048, dev="cuda"):
    """``kv_append`` of one token per row (with rotary) into ``layers`` layers: one graph per dtype."""
    cos, sin = ops.rope_tables(S_max, D, device=dev)
    qkv = torch.randn(B, 1, (Hq + 2 * Hk) * D, device=dev, dtype=torch.bfloat16)
    variants = {}
    for name, kv in (("bf16", None), ("fp8", KV), ("bf16_paged", None), ("fp8_paged", KV)):
        if name.endswith("paged"):
            c = ops.PagedKVCache(layers, B, S_max, Hk, D, torch.bfloat16, dev, kv_dtype=kv)
            c.reserve([pos + 1] * B)
        else:
            c = ops.KVCache(layers, B, S_max, Hk, D, torch.bfloat16, dev, kv_dtype=kv)
        c.set_lens([pos] * B)
        variants[name] = Variant(name, [lambda i=i, c=c: ops.kv_append(qkv, c, i, Hq, Hk, cos, sin) for i in range(layers)])
    for v in variants.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants.values():
            v.measure()
    out = dict(op="kv_append", B=B, Hq=Hq, Hk=Hk, D=D, T=1, layers_per_graph=layers, timing="graph replay")
    for k, v in variants.items():
        out[f"{k}_us"] = round(statistics.median(v.us), 2)
    out["bf16_spread_pct"] = _spread(variants["bf16"].us)
    return out


def _llama7b(dev):
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig(**LLAMA_CONFIGS["llama-7b"], max_position_embeddings=8192), device=dev).eval()


def _random_fill(cache):
    """Finite random contents (timing only): normal values, or codes below NaN with scale 2^-6."""
    for i in range(cache.num_layers):
        if cache.quantized:
            for t, s in ((cache.k[i], cache.k_scale[i]), (cache.v[i], cache.v_scale[i])):
                t.view(torch.uint8).random_(0, 0x78)
                s.fill_(2.0 ** -6)
        else:
            cache.k[i].normal_()
            cache.v[i].normal_()


@torch.no_grad()
def bench_step(model, B, context, steps=20, rounds=3, dev="cuda"):
    """One llama-7b decode step at batch B over ``context`` cached tokens (random contents), with
    a bf16 and an fp8 contiguous cache, as a launch loop and as a graph replay.  The lengths
    are put back to ``context`` before every timed window."""
    total = 2 * (rounds + 1) * steps + 16
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = {}
    for name, kv in (("bf16", None), ("fp8", KV)):
        cache = model.init_cache(B, context + steps + 8, kv_dtype=kv)
        _random_fill(cache)
        cache.set_lens([context] * B)
        st = ops.SamplerState(B, total, dev)
        ops.sample_step(model.decode_step(torch.ones(B, dtype=torch.long, device=dev), cache), st)
        cache.set_lens([context] * B)
        graph = model.decode_graph(cache, st, steps=total)
        runs[name] = dict(cache=cache, st=st, graph=graph, loop=[], replay=[])

    def window(fn, cache):
        cache.set_lens([context] * B)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / steps

    for rnd in range(rounds + 1):  # the first round warms up
        for name, r in runs.items():
            loop = window(lambda: ops.sample_step(model.decode_step(r["st"].tok, r["cache"]), r["st"]), r["cache"])
            replay = window(r["graph"].step, r["cache"])
            if rnd:
                r["loop"].append(loop)
                r["replay"].append(replay)
    out = dict(model="llama-7b", B=B, context=context, steps=steps, rounds=rounds)
    for how in ("loop", "replay"):
        a, b_ = statistics.median(runs["bf16"][how]), statistics.median(runs["fp8"][how])
        out.update({f"bf16_{how}_ms": round(a, 3), f"fp8_{how}_ms": round(b_, 3), f"{how}_speedup": round(a / b_, 3),
                    f"bf16_{how}_spread_pct": _spread(runs["bf16"][how])})
    out["bf16_cache_GiB"] = round(runs["bf16"]["cache"].nbytes / 2 ** 30, 3)
    out["fp8_cache_GiB"] = round(runs["fp8"]["cache"].nbytes / 2 ** 30, 3)
    return out


@torch.no_grad()
def bench_prefill(model, B, prompt=512, rounds=3, dev="cuda"):
    ids = torch.randint(1, model.cfg.vocab_size, (B, prompt), device=dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {"bf16": [], "fp8": []}
    caches = {"bf16": model.init_cache(B, prompt + 8), "fp8": model.init_cache(B, prompt + 8, kv_dtype=KV)}
    for rnd in range(rounds + 1):
        for name, cache in caches.items():
            torch.cuda.synchronize()
            t0.record()
            model.prefill(ids, cache)
            t1.record()
            torch.cuda.synchronize()
            if rnd:
                ms[name].append(t0.elapsed_time(t1))
    a, b_ = statistics.median(ms["bf16"]), statistics.median(ms["fp8"])
    return dict(model="llama-7b", op="prefill", B=B, prompt=prompt, bf16_ms=round(a, 3), fp8_ms=round(b_, 3),
                ratio=round(b_ / a, 4), bf16_spread_pct=_spread(ms["bf16"]))


@torch.no_grad()
def agreement(new_tokens=32, dev="cuda"):
    """Greedy tokens with the fp8 cache against the bf16 cache on the tiny test models, and the
    largest logit difference over the steps up to the first token that differs."""
    from paddle_amd.models.gpt import GPTConfig, GPTForCausalLM
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    out = []
    for kind in ("llama", "llama-kv1", "gpt"):
        torch.manual_seed(0)
        if kind == "gpt":
            model = GPTForCausalLM(GPTConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2, num_attention_heads=2,
                                             max_position_embeddings=128, dtype="bfloat16"), device=dev).eval()
        else:
            model = LlamaForCausalLM(LlamaConfig(**LLAMA_CONFIGS["llama-tiny"], dtype="bfloat16",
                                                 num_key_value_heads=1 if kind == "llama-kv1" else None), device=dev).eval()
        g = torch.Generator().manual_seed(3)
        ids = torch.zeros(3, 7, dtype=torch.long)
        for b, n in enumerate((3, 7, 5)):
            ids[b, :n] = torch.randint(1, model.cfg.vocab_size, (n,), generator=g)
        ids = ids.to(dev)
        runs = {}
        for name, kv in (("bf16", None), ("fp8", KV)):
            seen, orig = [], model._lm_logits
            model._lm_logits = lambda y: seen.append(orig(y).float().clone()) or seen[-1]
            try:
                toks, _ = model.generate(ids, new_tokens, prompt_lens=[3, 7, 5], kv_dtype=kv)
            finally:
                del model._lm_logits
            runs[name] = (toks, seen)
        same = runs["bf16"][0] == runs["fp8"][0]
        first = [int((~same[b]).nonzero()[0]) if not bool(same[b].all()) else new_tokens for b in range(3)]
        diff = max(float((runs["bf16"][1][s][b] - runs["fp8"][1][s][b]).abs().max())
                   for b in range(3) for s in range(min(first[b] + 1, new_tokens)))
        out.append(dict(model=kind, new_tokens=new_tokens, rows=3, token_agreement=round(float(same.float().mean()), 4),
                        first_difference_per_row=first, max_logit_diff=round(diff, 4),
                        max_abs_logit=round(float(max(x.abs().max() for x in runs["bf16"][1])), 3)))
    return out


def write_md(path, rows, appends, steps, prefills, agree):
    with open(path, "w") as f:
        f.write("| B | Hq/Hk | cached len | layout | splits | bf16 us (min-max) | bf16 spread | bf16 TB/s | fp8 us | "
                "fp8 TB/s | speed-up | goal met |\n" + "|---" * 12 + "|\n")
        for r in rows:
            for tag, layout in (("", "contiguous"), ("paged_", f"paged {r['block_size']}")):
                f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['cached_len']} | {layout} | {r['num_splits']} | "
                        f"{r[tag + 'bf16_us']} ({r[tag + 'bf16_min_us']}-{r[tag + 'bf16_max_us']}) | "
                        f"{r[tag + 'bf16_spread_pct']} % | {r[tag + 'bf16_TB_per_s']} | {r[tag + 'fp8_us']} | "
                        f"{r[tag + 'fp8_TB_per_s']} | {r[tag + 'speedup']:.3f} | {'yes' if r[tag + 'goal_met'] else 'NO'} |\n")
        if appends:
            f.write("\n| kv_append T = 1 | B | Hq/Hk | bf16 us | fp8 us | bf16 paged us | fp8 paged us | bf16 spread |\n"
                    + "|---" * 8 + "|\n")
            for r in appends:
                f.write(f"| per layer | {r['B']} | {r['Hq']}/{r['Hk']} | {r['bf16_us']} | {r['fp8_us']} | "
                        f"{r['bf16_paged_us']} | {r['fp8_paged_us']} | {r['bf16_spread_pct']} % |\n")
        if steps:
            f.write("\n| model | B | context | bf16 loop ms | fp8 loop ms | speed-up | bf16 graph ms | fp8 graph ms | "
                    "speed-up | bf16 spread (loop / graph) | cache GiB bf16 / fp8 |\n" + "|---" * 11 + "|\n")
            for r in steps:
                f.write(f"| {r['model']} | {r['B']} | {r['context']} | {r['bf16_loop_ms']} | {r['fp8_loop_ms']} | "
                        f"{r['loop_speedup']:.3f} | {r['bf16_replay_ms']} | {r['fp8_replay_ms']} | "
                        f"{r['replay_speedup']:.3f} | {r['bf16_loop_spread_pct']} % / {r['bf16_replay_spread_pct']} % | "
                        f"{r['bf16_cache_GiB']} / {r['fp8_cache_GiB']} |\n")
        if prefills:
            f.write("\n| prefill | B | prompt | bf16 ms | fp8 ms | fp8 / bf16 | bf16 spread |\n" + "|---" * 7 + "|\n")
            for r in prefills:
                f.write(f"| {r['model']} | {r['B']} | {r['prompt']} | {r['bf16_ms']} | {r['fp8_ms']} | {r['ratio']:.3f} | "
                        f"{r['bf16_spread_pct']} % |\n")
        if agree:
            f.write("\n| test model | new tokens x rows | greedy tokens equal | first difference per row | "
                    "max logit difference up to it | max abs logit |\n" + "|---" * 6 + "|\n")
            for r in agree:
                f.write(f"| {r['model']} | {r['new_tokens']} x {r['rows']} | {100 * r['token_agreement']:.1f} % | "
                        f"{r['first_difference_per_row']} | {r['max_logit_diff']} | {r['max_abs_logit']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=150.0, help="least length of one timed window")
    ap.add_argument("--append", action="store_true", help="also time kv_append at T = 1")
    ap.add_argument("--step", action="store_true", help="also time llama-7b decode steps and a 512-token prefill")
    ap.add_argument("--agree", action="store_true", help="also report the greedy-token agreement on the test models")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="two shapes, 2 rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_fp8_bench needs a GPU: a CPU timing says nothing about the kernel")
    shapes = [(B, 32, Hk, 128, L) for B in (1, 8) for Hk in (32, 8) for L in (2048, 8192)]
    if args.quick:
        shapes, args.repeats = [shapes[0], shapes[-1]], 2
    print(json.dumps(dict(repeats=args.repeats, window_ms=args.window_ms, block_size=DEFAULT_BLOCK_SIZE)), flush=True)
    rows, appends, steps, prefills, agree = [], [], [], [], []
    for s in shapes:
        rows.append(bench_shape(*s, repeats=args.repeats, window_ms=args.window_ms))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.append:
        for B in (1, 8):
            for Hk in (32, 8):
                appends.append(bench_append(B, 32, Hk, 128, args.repeats, min(args.window_ms, 50.0)))
                print(json.dumps(appends[-1]), flush=True)
    if args.agree:
        agree = agreement()
        for r in agree:
            print(json.dumps(r), flush=True)
    if args.step:
        model = _llama7b("cuda")
        for B in (1, 8):
            for ctx in ((512,) if args.quick else (512, 4096)):
                steps.append(bench_step(model, B, ctx, rounds=2 if args.quick else 3))
                print(json.dumps(steps[-1]), flush=True)
                torch.cuda.empty_cache()
            prefills.append(bench_prefill(model, B))
            print(json.dumps(prefills[-1]), flush=True)
    if args.md:
        write_md(args.md, rows, appends, steps, prefills, agree)


if __name__ == "__main__":
    main()
