"""Decode attention (split-KV, csrc/kernels/attn_decode.hip) against the only other way
to attend one new token to a cache: ``ops.flash_attention`` with a single query row.

For every shape of

    B in {1, 8}  x  Hq/Hk in {32/32, 32/8}  x  D = 128  x  cached length in {2048, 8192}

it prints one JSON line: microseconds per call for both paths and the KV bytes read per
second by the new kernel (bytes = 2 * B * len * Hk * D * 2, what the algorithm must
read), with its share of the 6.3 TB/s HBM streaming figure (a float4 copy on this chip).

Method: HIP events around a stream of calls that rotates over a set of caches larger
than the 256 MiB last-level cache, so every call reads its keys and values from HBM;
the calls are captured once into a HIP graph (one linear chain) and the replay is
timed, so the host's launch cost is not in the number.  ``--no-graph`` times the plain
launch loop instead.  Every shape is warmed up first.

``--step`` also times one full ``decode_step`` of llama-7b at B = 1 and B = 8 and the
share of it spent in the GEMMs at M = B (whichever path ``ops.linear`` takes).

``--sweep`` times every split count per shape (how the default was checked).

    python benchmarks/decode_attn_bench.py --md decode_attn_bench_table.md --step
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddle_amd import ops  # noqa: E402

HBM_STREAM_TBS = 6.3  # measured float4 copy on MI355X
LLC_BYTES = 256 << 20
MIN_WINDOW_MS = 250.0


def _time_calls(fns, reps, graph):
    """Mean microseconds per call of the callables ``fns`` run in order, ``reps`` times."""
    for f in fns:  # warm-up: every call once
        f()
    torch.cuda.synchronize()
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for f in fns:
                f()
        g.replay()  # warm the replay
        torch.cuda.synchronize()

        def run():
            g.replay()
    else:
        def run():
            for f in fns:
                f()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(r):
        t0.record()
        for _ in range(r):
            run()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)  # ms

    # a short window measures the clock and the scheduler: size the timed one to >= MIN_WINDOW_MS
    ms = timed(reps)
    reps = max(reps, math.ceil(reps * MIN_WINDOW_MS / max(ms, 1e-3)))
    return timed(reps) * 1e3 / (reps * len(fns))


@torch.no_grad()
def bench_shape(B, Hq, Hk, D, L, graph, dev="cuda"):
    kv_bytes = 2 * B * L * Hk * D * 2
    n = max(2, math.ceil(2 * LLC_BYTES / kv_bytes) + 1)  # rotating set > 2x the last-level cache
    cache = ops.KVCache(n, B, L, Hk, D, torch.bfloat16, dev)  # n "layers" = n independent caches
    for i in range(n):
        cache.k[i].normal_()
        cache.v[i].normal_()
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    ns = ops.decode.default_num_splits(B, Hk, L)
    new = [lambda i=i: ops.decode_attention(q, cache, i, kv_len=kv_len) for i in range(n)]
    old = [lambda i=i: ops.flash_attention(q, cache.k[i], cache.v[i], causal=True) for i in range(n)]
    err = (new[0]().float() - old[0]().float()).abs().max().item()
    reps = max(3, math.ceil(200 / n))
    us_new = _time_calls(new, reps, graph)
    us_old = _time_calls(old, max(2, reps // 4), graph)
    tbs = kv_bytes / (us_new * 1e-6) / 1e12
    return dict(B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, num_splits=ns, rotating_caches=n,
                decode_attention_us=round(us_new, 2), flash_attention_1row_us=round(us_old, 2),
                speedup=round(us_old / us_new, 2), kv_bytes=kv_bytes, kv_TB_per_s=round(tbs, 3),
                pct_of_hbm_stream=round(100 * tbs / HBM_STREAM_TBS, 1), max_abs_diff_vs_flash=err,
                timing="graph replay" if graph else "launch loop")


@torch.no_grad()
def sweep_splits(B, Hq, Hk, D, L, graph, dev="cuda"):
    """decode_attention microseconds per call for every split count, next to the default."""
    kv_bytes = 2 * B * L * Hk * D * 2
    n = max(2, math.ceil(2 * LLC_BYTES / kv_bytes) + 1)
    cache = ops.KVCache(n, B, L, Hk, D, torch.bfloat16, dev)
    for i in range(n):
        cache.k[i].normal_()
        cache.v[i].normal_()
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    us = {}
    for ns in (1, 2, 4, 8, 16, 32, 64):
        fns = [lambda i=i: ops.decode_attention(q, cache, i, num_splits=ns, kv_len=kv_len) for i in range(n)]
        us[ns] = round(_time_calls(fns, 3, graph), 2)
    return dict(B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, default_splits=ops.decode.default_num_splits(B, Hk, L),
                us_by_splits=us)


@torch.no_grad()
def bench_step(B, prompt=512, steps=40, dev="cuda"):
    """One llama-7b decode step at batch B, and the GEMMs of that step alone."""
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(**LLAMA_CONFIGS["llama-7b"])
    model = LlamaForCausalLM(cfg, device=dev).eval()
    ids = torch.randint(1, cfg.vocab_size, (B, prompt), device=dev)
    cache = model.init_cache(B, prompt + steps + 4)
    logits = model.prefill(ids, cache)
    tok = logits.argmax(-1)
    for _ in range(3):
        tok = model.decode_step(tok, cache).argmax(-1)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        tok = model.decode_step(tok, cache).argmax(-1)
    t1.record()
    torch.cuda.synchronize()
    step_ms = t0.elapsed_time(t1) / steps
    # the same GEMMs alone: every layer's weights once per pass, so they stream from HBM
    H = cfg.hidden_size
    y = torch.randn(B, 1, H, device=dev, dtype=torch.bfloat16)

    def gemms():
        for layer in model.layers:
            ops.linear(y, layer.qkv_proj)
            ops.linear(y, layer.o_proj)
            layer._mlp(y)
        ops.linear(y, model.lm_head)

    gemms()
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        gemms()
    t1.record()
    torch.cuda.synchronize()
    gemm_ms = t0.elapsed_time(t1) / steps
    wbytes = 2 * sum(p.numel() for n, p in model.named_parameters() if p.dim() == 2 and n != "embed_tokens")
    return dict(model="llama-7b", B=B, context=prompt, decode_step_ms=round(step_ms, 3),
                gemms_alone_ms=round(gemm_ms, 3), gemm_share_pct=round(100 * gemm_ms / step_ms, 1),
                weight_bytes=wbytes, weight_stream_floor_ms=round(wbytes / (HBM_STREAM_TBS * 1e12) * 1e3, 3),
                timing="launch loop")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--no-graph", action="store_true", help="time the plain launch loop, not a graph replay")
    ap.add_argument("--step", action="store_true", help="also time a llama-7b decode step at B = 1 and 8")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--sweep", action="store_true", help="time every split count per shape instead")
    ap.add_argument("--quick", action="store_true", help="first shape only (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_attn_bench needs a GPU: a CPU timing says nothing about the kernel")
    shapes = [(B, 32, Hk, 128, L) for B in (1, 8) for Hk in (32, 8) for L in (2048, 8192)]
    rows, steps = [], []
    for s in shapes[:1] if args.quick else shapes:
        if args.sweep:
            print(json.dumps(sweep_splits(*s, graph=not args.no_graph)), flush=True)
            continue
        r = bench_shape(*s, graph=not args.no_graph)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.step:
        for B in (1, 8):
            r = bench_step(B)
            steps.append(r)
            print(json.dumps(r), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| B | Hq/Hk | D | cached len | splits | decode_attention us | flash_attention (1 row) us | "
                    f"speed-up | KV TB/s | % of {HBM_STREAM_TBS} TB/s |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['D']} | {r['cached_len']} | {r['num_splits']} | "
                        f"{r['decode_attention_us']} | {r['flash_attention_1row_us']} | {r['speedup']}x | "
                        f"{r['kv_TB_per_s']} | {r['pct_of_hbm_stream']} |\n")
            if steps:
                f.write("\n| model | B | context | decode step ms | GEMMs alone ms | GEMM share | "
                        "weight-stream floor ms |\n|---|---|---|---|---|---|---|\n")
                for r in steps:
                    f.write(f"| {r['model']} | {r['B']} | {r['context']} | {r['decode_step_ms']} | "
                            f"{r['gemms_alone_ms']} | {r['gemm_share_pct']} % | {r['weight_stream_floor_ms']} |\n")


if __name__ == "__main__":
    main()
