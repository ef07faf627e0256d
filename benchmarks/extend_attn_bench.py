"""What ``ops.extend_attention`` (csrc/kernels/attn_extend.hip) costs, in one process:

small T   ``extend_attention`` of T in {2, 4, 8, 16} tokens per row against T successive
          ``decode_attention`` calls (cached lengths L+1 .. L+T) -- all the code could do before --
          for B in {1, 8} x Hq/Hk in {32/32, 32/8} x D = 128 x L in {2048, 8192} cached tokens
          x {bf16, fp8} x {contiguous, paged 64}.  The byte ceiling is T x: the T calls read the
          cache T times, the extend kernel once.  Goal: faster than the T calls by more than
          their run-to-run spread at every 8192-token shape.
chunk T   T = 512 on top of 0 / 2048 / 8192 cached tokens against ``F._fa_fwd`` over a dense
          bf16 K / V of the same length (Sq = 512, Sk = base + 512, causal): the floor for the
          contiguous bf16 case.  Reported, no goal.
model     llama-7b: ``extend`` of 8 and 16 tokens at context 512 against as many
          ``decode_step``s, and a 4096-token prompt through ``prefill(chunk=512)`` against the
          one-shot call (time and peak device memory above the resident model and cache), with
          bf16 and with quantised weights (``--model``).

Method (that of paged_decode_bench.py / kv_fp8_bench.py): every variant rotates over a set of
caches larger than twice the 256 MiB last-level cache in fp8 bytes; the calls of one pass are
captured once into a HIP graph and the replay is timed with HIP events; every graph is warmed
up, then ``--repeats`` rounds each time every variant of a shape once (interleaved) over a window
of at least ``--window-ms``.  Reported: the median over the rounds, and next to every ratio the
baseline's spread (max - min) / median.  The chunk part uses the same rotation and rounds but
times launch loops on both sides (``F._fa_fwd`` does not capture into a graph).  The model
part times launch loops (``extend`` is not captured into a graph) with HIP events, median of
``--model-rounds`` rounds.

    python benchmarks/extend_attn_bench.py --md extend_attn_bench_table.md
    FLAGS_allocator_strategy=torch python benchmarks/extend_attn_bench.py --only-model --md extend_model_table.md

(the model part reads torch's peak-memory statistics, which the default buddy allocator behind
torch does not keep).
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
from paddle_amd.ops import fused as F  # noqa: E402
from paddle_amd.ops.paged import DEFAULT_BLOCK_SIZE  # noqa: E402
from benchmarks.paged_decode_bench import LLC_BYTES, Variant, shuffled_table  # noqa: E402
from benchmarks.kv_fp8_bench import KV, _llama7b, _random_fill, _spread  # noqa: E402

TS = (2, 4, 8, 16)


class LoopVariant(Variant):
    """``Variant`` as a launch loop: ``F._fa_fwd`` does not capture into a graph, so the chunk
    part times both sides this way (the calls are long against a launch)."""

    def __init__(self, name, fns):
        self.name, self.n, self.fns = name, len(fns), fns
        for f in fns:
            f()
        torch.cuda.synchronize()
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.reps = 1
        self.us = []

    def window(self, reps):
        self.t0.record()
        for _ in range(reps):
            for f in self.fns:
                f()
        self.t1.record()
        torch.cuda.synchronize()
        return self.t0.elapsed_time(self.t1)  # ms


def _caches(n, B, S, Hk, D, dev, bs=DEFAULT_BLOCK_SIZE):
    """bf16 / fp8 x contiguous / paged caches of n layers with finite random contents."""
    out = {}
    for name, kv, paged in (("bf16", None, False), ("fp8", KV, False), ("bf16_paged", None, True), ("fp8_paged", KV, True)):
        if paged:
            c = ops.PagedKVCache(n, B, S, Hk, D, torch.bfloat16, dev, block_size=bs, zero_fill=False, kv_dtype=kv)
            c.load_block_table(shuffled_table(B, c.max_blocks, c.num_blocks, seed=bs))
        else:
            c = ops.KVCache(n, B, S, Hk, D, torch.bfloat16, dev, kv_dtype=kv)
        _random_fill(c)
        out[name] = c
    return out


@torch.no_grad()
def bench_small(B, Hq, Hk, D, L, repeats, window_ms, dev="cuda"):
    S = L + max(TS)
    f8_bytes = 2 * B * L * Hk * (D + 4)
    n = max(2, math.ceil(2 * LLC_BYTES / f8_bytes) + 1)
    caches = _caches(n, B, S, Hk, D, dev)
    base = torch.full((B,), L, dtype=torch.int32, device=dev)
    variants = {}
    for T in TS:
        q = torch.randn(B, T, Hq, D, device=dev, dtype=torch.bfloat16)
        lens = [torch.full((B,), L + j + 1, dtype=torch.int32, device=dev) for j in range(T)]
        for name, c in caches.items():
            variants[("extend", name, T)] = Variant(f"extend {name} T{T}", [
                lambda i=i, c=c, q=q: ops.extend_attention(q, c, i, base_len=base) for i in range(n)])
            variants[("decode", name, T)] = Variant(f"decode {name} T{T}", [
                lambda i=i, c=c, q=q, j=j, lens=lens: ops.decode_attention(q[:, j:j + 1], c, i, kv_len=lens[j])
                for i in range(n) for j in range(T)])
            variants[("decode", name, T)].n = n  # per pass of T calls over one cache
    for v in variants.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants.values():
            v.measure()
    rows = []
    for T in TS:
        for name in caches:
            e, d = variants[("extend", name, T)].us, variants[("decode", name, T)].us
            em, dm = statistics.median(e), statistics.median(d)
            sp = _spread(d)
            rows.append(dict(part="small", B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, T=T, cache=name,
                             extend_splits=ops.default_extend_splits(B, Hk, T, S),
                             decode_splits=ops.decode.default_num_splits(B, Hk, S), rotating_caches=n,
                             extend_us=round(em, 2), extend_spread_pct=_spread(e), decode_T_calls_us=round(dm, 2),
                             decode_spread_pct=sp, speedup=round(dm / em, 3), byte_ceiling=T,
                             goal_met=bool(em < dm * (1 - sp / 100))))
    return rows


@torch.no_grad()
def bench_chunk(B, Hq, Hk, D, base, T, repeats, window_ms, dev="cuda"):
    S = base + T
    bytes_ = 2 * B * S * Hk * (D + 4)
    n = max(2, math.ceil(2 * LLC_BYTES / bytes_) + 1)
    caches = _caches(n, B, S, Hk, D, dev)
    q = torch.randn(B, T, Hq, D, device=dev, dtype=torch.bfloat16)
    bl = torch.full((B,), base, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    slab = caches["bf16"]
    variants = {"fa_fwd": LoopVariant("fa_fwd", [lambda i=i: F._fa_fwd(q, slab.k[i], slab.v[i], True, scale)
                                                 for i in range(n)])}
    for name, c in caches.items():
        variants[name] = LoopVariant(name, [lambda i=i, c=c: ops.extend_attention(q, c, i, base_len=bl)
                                            for i in range(n)])
    # the two compute the same thing
    want, _ = F._fa_fwd(q, slab.k[0], slab.v[0], True, scale)
    got = ops.extend_attention(q, slab, 0, base_len=bl)
    err = float((got.float() - want.float()).abs().max())
    for v in variants.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants.values():
            v.measure()
    fa = statistics.median(variants["fa_fwd"].us)
    flops = 4.0 * B * Hq * D * (T * base + T * (T + 1) / 2)
    out = dict(part="chunk", B=B, Hq=Hq, Hk=Hk, D=D, base=base, T=T, rotating_caches=n,
               extend_splits=ops.default_extend_splits(B, Hk, T, S), max_abs_diff_vs_fa_fwd=round(err, 5),
               fa_fwd_us=round(fa, 1), fa_fwd_spread_pct=_spread(variants["fa_fwd"].us),
               fa_fwd_TFLOPs=round(flops / (fa * 1e-6) / 1e12, 1))
    for name in caches:
        m = statistics.median(variants[name].us)
        out[f"{name}_us"] = round(m, 1)
        out[f"{name}_over_fa_fwd"] = round(m / fa, 2)
    out["bf16_TFLOPs"] = round(flops / (out["bf16_us"] * 1e-6) / 1e12, 1)
    return out


def _timed(fn, setup, rounds):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rnd in range(rounds + 1):  # the first round warms up
        setup()
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if rnd:
            ms.append(t0.elapsed_time(t1))
    return ms


@torch.no_grad()
def bench_model(model, weights, rounds, dev="cuda"):
    out = []
    B, ctx = 1, 512
    cache = model.init_cache(B, ctx + 64)
    _random_fill(cache)
    for T in (8, 16):
        ids = torch.randint(1, model.cfg.vocab_size, (B, T), device=dev)
        reset = lambda: cache.set_lens([ctx] * B)  # noqa: E731
        ext = _timed(lambda: model.extend(ids, cache), reset, rounds)

        def steps():
            for j in range(T):
                model.decode_step(ids[:, j], cache)

        dec = _timed(steps, reset, rounds)
        e, d = statistics.median(ext), statistics.median(dec)
        out.append(dict(part="model_extend", weights=weights, B=B, context=ctx, T=T, extend_ms=round(e, 3),
                        decode_steps_ms=round(d, 3), decode_spread_pct=_spread(dec), speedup=round(d / e, 2)))
    del cache
    torch.cuda.empty_cache()
    S = 4096
    ids = torch.randint(1, model.cfg.vocab_size, (1, S), device=dev)
    cache = model.init_cache(1, S + 8)
    res = {}
    for name, chunk in (("one_shot", None), ("chunk_512", 512)):
        peaks = []

        def run():
            model.prefill(ids, cache, chunk=chunk)

        def setup():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            peaks.append(torch.cuda.memory_allocated())

        ms = _timed(run, setup, rounds)
        res[name] = (statistics.median(ms), _spread(ms), (torch.cuda.max_memory_allocated() - peaks[-1]) / 2 ** 20)
    a, b_ = res["one_shot"], res["chunk_512"]
    out.append(dict(part="model_prefill", weights=weights, B=1, prompt=S, one_shot_ms=round(a[0], 2),
                    one_shot_spread_pct=a[1], chunk_512_ms=round(b_[0], 2), chunk_over_one_shot=round(b_[0] / a[0], 3),
                    one_shot_peak_MiB=round(a[2], 1), chunk_512_peak_MiB=round(b_[2], 1)))
    return out


def write_md(path, small, chunk, model):
    with open(path, "w") as f:
        if small:
            f.write("| B | Hq/Hk | cached | T | cache | splits ext / dec | extend us | T decode calls us | "
                    "decode spread | speed-up (ceiling T) | goal met |\n" + "|---" * 11 + "|\n")
        for r in small:
            f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['cached_len']} | {r['T']} | {r['cache']} | "
                    f"{r['extend_splits']} / {r['decode_splits']} | {r['extend_us']} | {r['decode_T_calls_us']} | "
                    f"{r['decode_spread_pct']} % | {r['speedup']:.2f} | {'yes' if r['goal_met'] else 'NO'} |\n")
        if chunk:
            f.write("\n| B | Hq/Hk | base | T | fa_fwd us (spread) | fa_fwd TFLOP/s | extend bf16 us | x fa_fwd | "
                    "fp8 x | paged x | fp8 paged x | bf16 TFLOP/s |\n" + "|---" * 12 + "|\n")
            for r in chunk:
                f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['base']} | {r['T']} | {r['fa_fwd_us']} "
                        f"({r['fa_fwd_spread_pct']} %) | {r['fa_fwd_TFLOPs']} | {r['bf16_us']} | {r['bf16_over_fa_fwd']} | "
                        f"{r['fp8_over_fa_fwd']} | {r['bf16_paged_over_fa_fwd']} | {r['fp8_paged_over_fa_fwd']} | "
                        f"{r['bf16_TFLOPs']} |\n")
        ext = [r for r in model if r["part"] == "model_extend"]
        pre = [r for r in model if r["part"] == "model_prefill"]
        if ext:
            f.write("\n| llama-7b weights | context | T | extend ms | T decode steps ms (spread) | speed-up |\n"
                    + "|---" * 6 + "|\n")
            for r in ext:
                f.write(f"| {r['weights']} | {r['context']} | {r['T']} | {r['extend_ms']} | {r['decode_steps_ms']} "
                        f"({r['decode_spread_pct']} %) | {r['speedup']:.2f} |\n")
        if pre:
            f.write("\n| llama-7b weights | prompt | one-shot ms (spread) | chunk 512 ms | ratio | one-shot peak MiB | "
                    "chunk 512 peak MiB |\n" + "|---" * 7 + "|\n")
            for r in pre:
                f.write(f"| {r['weights']} | {r['prompt']} | {r['one_shot_ms']} ({r['one_shot_spread_pct']} %) | "
                        f"{r['chunk_512_ms']} | {r['chunk_over_one_shot']:.3f} | {r['one_shot_peak_MiB']} | "
                        f"{r['chunk_512_peak_MiB']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least length of one timed window")
    ap.add_argument("--model", action="store_true", help="also time llama-7b extend and chunked prefill")
    ap.add_argument("--only-model", action="store_true", help="skip the attention parts")
    ap.add_argument("--model-rounds", type=int, default=5)
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="one shape per part, 2 rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extend_attn_bench needs a GPU: a CPU timing says nothing about the kernel")
    shapes = [(B, 32, Hk, 128, L) for B in (1, 8) for Hk in (32, 8) for L in (2048, 8192)]
    chunks = [(B, 32, Hk, 128, base, 512) for B in (1, 8) for Hk in (32, 8) for base in (0, 2048, 8192)]
    if args.quick:
        shapes, chunks, args.repeats, args.model_rounds = shapes[:1], chunks[1:2], 2, 2
    if args.only_model:
        shapes, chunks, args.model = [], [], True
    from paddle_amd import runtime

    if args.model and runtime.buddy_active():
        raise SystemExit("--model reads torch's peak-memory statistics, which the buddy allocator behind torch does not "
                         "keep: run the model part with FLAGS_allocator_strategy=torch")
    print(json.dumps(dict(repeats=args.repeats, window_ms=args.window_ms, block_size=DEFAULT_BLOCK_SIZE)), flush=True)
    small, chunk, model_rows = [], [], []
    for s in shapes:
        rows = bench_small(*s, repeats=args.repeats, window_ms=args.window_ms)
        small += rows
        for r in rows:
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    for s in chunks:
        chunk.append(bench_chunk(*s, repeats=args.repeats, window_ms=args.window_ms))
        print(json.dumps(chunk[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.md:
        write_md(args.md, small, chunk, model_rows)
    if args.model:
        model = _llama7b("cuda")
        model_rows += bench_model(model, "bf16", args.model_rounds)
        model.quantize_weights()
        torch.cuda.empty_cache()
        model_rows += bench_model(model, "fp8_e4m3", args.model_rounds)
        for r in model_rows:
            print(json.dumps(r), flush=True)
    if args.md:
        write_md(args.md, small, chunk, model_rows)


if __name__ == "__main__":
    main()
