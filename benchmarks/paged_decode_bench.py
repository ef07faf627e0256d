"""What the block-table indirection of the paged KV cache costs: ``ops.decode_attention``
over a ``PagedKVCache`` against the same call over a contiguous ``KVCache``, in one
process, for

    B in {1, 8}  x  Hq/Hk in {32/32, 32/8}  x  D = 128  x  cached length in {2048, 8192}
    x  block_size in {16, 32, 64, 128, 256}

with the same ``num_splits`` on both sides and a shuffled block assignment: the pool's
block ids in random order, dealt to the rows round-robin, so no row's blocks are monotone
or adjacent and neighbouring blocks belong to different rows.

Method (that of decode_attn_bench.py): every variant rotates over a set of caches larger
than twice the 256 MiB last-level cache, so keys and values come from HBM; the calls of one
pass are captured once into a HIP graph and the replay is timed with HIP events, so launch
cost is not in the number.  Every graph is warmed up, then ``--repeats`` rounds each time
every variant once (contiguous, then each block size: interleaved, so drift hits all alike)
over a window of at least ``--window-ms``.  Reported: the median over the rounds; the
contiguous kernel's run-to-run spread is (max - min) / median of its rounds.  Before any
timing the paged output is checked bit-equal to the contiguous one on the same tokens.

The default block size is the smallest one whose median is within that spread of the
contiguous median at every 8192-token shape (the fastest one if none is).

``--step`` also times one llama-7b ``decode_step`` at context 512 with each cache (the paged
one with the block size this run chose).

    python benchmarks/paged_decode_bench.py --step --md paged_decode_bench_table.md
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
from paddle_amd.ops.paged import BLOCK_SIZES, DEFAULT_BLOCK_SIZE  # noqa: E402

LLC_BYTES = 256 << 20


def shuffled_table(B, blocks_per_row, num_blocks, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(num_blocks, generator=g).tolist()
    table = [[-1] * blocks_per_row for _ in range(B)]
    for j in range(blocks_per_row):
        for b in range(B):
            table[b][j] = ids.pop()
    return table


class Variant:
    """One graph: a pass of decode_attention over the n rotating caches."""

    def __init__(self, name, fns):
        self.name, self.n = name, len(fns)
        for f in fns:
            f()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for f in fns:
                f()
        self.graph.replay()
        torch.cuda.synchronize()
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.reps = 1
        self.us = []

    def window(self, reps):
        self.t0.record()
        for _ in range(reps):
            self.graph.replay()
        self.t1.record()
        torch.cuda.synchronize()
        return self.t0.elapsed_time(self.t1)  # ms

    def calibrate(self, window_ms):
        ms = self.window(3) / 3
        self.reps = max(3, math.ceil(window_ms / max(ms, 1e-3)))

    def measure(self):
        self.us.append(self.window(self.reps) * 1e3 / (self.reps * self.n))


@torch.no_grad()
def bench_shape(B, Hq, Hk, D, L, block_sizes, repeats, window_ms, dev="cuda"):
    kv_bytes = 2 * B * L * Hk * D * 2
    n = max(2, math.ceil(2 * LLC_BYTES / kv_bytes) + 1)  # rotating set > 2x the last-level cache
    ns = ops.decode.default_num_splits(B, Hk, L)
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    slab = ops.KVCache(n, B, L, Hk, D, torch.bfloat16, dev)
    for i in range(n):
        slab.k[i].normal_()
        slab.v[i].normal_()
    want = ops.decode_attention(q, slab, 0, num_splits=ns, kv_len=kv_len)
    variants = [Variant("contiguous", [lambda i=i: ops.decode_attention(q, slab, i, num_splits=ns, kv_len=kv_len)
                                       for i in range(n)])]
    pools = []
    for bs in block_sizes:
        pg = ops.PagedKVCache(n, B, L, Hk, D, torch.bfloat16, dev, block_size=bs, zero_fill=False)
        table = shuffled_table(B, pg.max_blocks, pg.num_blocks, seed=bs)
        pg.load_block_table(table)
        idx = torch.tensor(table, device=dev).reshape(-1)  # (b, j) -> block id
        for i in range(n):
            # the slab's tokens, block by block, at their shuffled places
            pg.k[i][idx] = slab.k[i].reshape(B * pg.max_blocks, bs, Hk, D)
            pg.v[i][idx] = slab.v[i].reshape(B * pg.max_blocks, bs, Hk, D)
        got = ops.decode_attention(q, pg, 0, num_splits=ns, kv_len=kv_len)
        if not torch.equal(got, want):
            raise SystemExit(f"paged (block_size {bs}) and contiguous outputs differ at {(B, Hq, Hk, D, L)}")
        pools.append(pg)
        variants.append(Variant(f"paged{bs}", [lambda i=i, pg=pg: ops.decode_attention(q, pg, i, num_splits=ns,
                                                                                      kv_len=kv_len) for i in range(n)]))
    for v in variants:
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants:
            v.measure()
    base = variants[0]
    med = statistics.median(base.us)
    out = dict(B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, num_splits=ns, rotating_caches=n, repeats=repeats,
               contiguous_us=round(med, 2), contiguous_min_us=round(min(base.us), 2),
               contiguous_max_us=round(max(base.us), 2), contiguous_spread_pct=round(100 * (max(base.us) - min(base.us)) / med, 2),
               kv_TB_per_s=round(kv_bytes / (med * 1e-6) / 1e12, 3), bit_equal=True, timing="graph replay")
    for bs, v in zip(block_sizes, variants[1:]):
        m = statistics.median(v.us)
        out[f"paged{bs}_us"] = round(m, 2)
        out[f"paged{bs}_ratio"] = round(m / med, 4)
        out[f"paged{bs}_spread_pct"] = round(100 * (max(v.us) - min(v.us)) / m, 2)
    return out


def choose_default(rows, block_sizes):
    """The smallest block size within the contiguous spread at every 8192-token shape, else
    the one with the smallest worst-case ratio."""
    big = [r for r in rows if r["cached_len"] == 8192]
    if not big:
        return None
    within = [bs for bs in block_sizes
              if all(r[f"paged{bs}_ratio"] <= 1 + r["contiguous_spread_pct"] / 100 for r in big)]
    worst = {bs: max(r[f"paged{bs}_ratio"] for r in big) for bs in block_sizes}
    pick = min(within) if within else min(block_sizes, key=lambda bs: worst[bs])
    return dict(chosen_block_size=pick, within_spread=within, worst_ratio_at_8192={str(k): v for k, v in worst.items()},
                rule="smallest block size whose median is within the contiguous kernel's run-to-run spread at "
                     "every 8192-token shape; the smallest worst-case ratio if none is")


@torch.no_grad()
def bench_step(B, block_size=None, prompt=512, steps=40, rounds=3, dev="cuda"):
    """One llama-7b decode step at batch B with a contiguous and with a paged cache (blocks of
    ``block_size`` tokens; default: the library's)."""
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(**LLAMA_CONFIGS["llama-7b"])
    model = LlamaForCausalLM(cfg, device=dev).eval()
    ids = torch.randint(1, cfg.vocab_size, (B, prompt), device=dev)
    max_len = prompt + (rounds + 1) * steps + 8
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    caches = {"contiguous": model.init_cache(B, max_len), "paged": model.init_cache(B, max_len, paged=True, block_size=block_size)}
    toks, ms = {}, {k: [] for k in caches}
    for name, cache in caches.items():
        toks[name] = model.prefill(ids, cache).argmax(-1)
        for _ in range(3):
            toks[name] = model.decode_step(toks[name], cache).argmax(-1)
    same = torch.equal(toks["contiguous"], toks["paged"])
    for _ in range(rounds):
        for name, cache in caches.items():
            tok = toks[name]
            torch.cuda.synchronize()
            t0.record()
            for _ in range(steps):
                tok = model.decode_step(tok, cache).argmax(-1)
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / steps)
            toks[name] = tok
    c, p = statistics.median(ms["contiguous"]), statistics.median(ms["paged"])
    return dict(model="llama-7b", B=B, context=prompt, block_size=caches["paged"].block_size,
                contiguous_step_ms=round(c, 3), paged_step_ms=round(p, 3), ratio=round(p / c, 4),
                contiguous_spread_pct=round(100 * (max(ms["contiguous"]) - min(ms["contiguous"])) / c, 2),
                same_tokens=bool(same and torch.equal(toks["contiguous"], toks["paged"])), timing="launch loop")


def write_md(path, rows, steps, choice, block_sizes):
    with open(path, "w") as f:
        f.write("| B | Hq/Hk | cached len | splits | contiguous us (min-max) | spread | "
                + " | ".join(f"bs {bs} us (ratio)" for bs in block_sizes) + " |\n")
        f.write("|---" * (6 + len(block_sizes)) + "|\n")
        for r in rows:
            f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['cached_len']} | {r['num_splits']} | "
                    f"{r['contiguous_us']} ({r['contiguous_min_us']}-{r['contiguous_max_us']}) | "
                    f"{r['contiguous_spread_pct']} % | "
                    + " | ".join(f"{r[f'paged{bs}_us']} ({r[f'paged{bs}_ratio']:.3f})" for bs in block_sizes) + " |\n")
        if choice:
            f.write(f"\nChosen block size: {choice['chosen_block_size']} (within the spread at every 8192-token "
                    f"shape: {choice['within_spread'] or 'none'}; worst paged / contiguous ratio at 8192 tokens per "
                    f"block size: {choice['worst_ratio_at_8192']}).\n")
        if steps:
            f.write("\n| model | B | context | block size | contiguous step ms | paged step ms | ratio | "
                    "contiguous spread | same tokens |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in steps:
                f.write(f"| {r['model']} | {r['B']} | {r['context']} | {r['block_size']} | {r['contiguous_step_ms']} | "
                        f"{r['paged_step_ms']} | {r['ratio']:.3f} | {r['contiguous_spread_pct']} % | "
                        f"{r['same_tokens']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=150.0, help="least length of one timed window")
    ap.add_argument("--step", action="store_true", help="also time a llama-7b decode step at B = 1 and 8")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="first shape, two block sizes, 2 rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paged_decode_bench needs a GPU: a CPU timing says nothing about the kernel")
    shapes = [(B, 32, Hk, 128, L) for B in (1, 8) for Hk in (32, 8) for L in (2048, 8192)]
    block_sizes = list(BLOCK_SIZES)
    if args.quick:
        shapes, block_sizes, args.repeats = shapes[:1], block_sizes[:2], 2
    print(json.dumps(dict(default_block_size_in_tree=DEFAULT_BLOCK_SIZE, repeats=args.repeats,
                          window_ms=args.window_ms)), flush=True)
    rows, steps = [], []
    for s in shapes:
        r = bench_shape(*s, block_sizes=block_sizes, repeats=args.repeats, window_ms=args.window_ms)
        rows.append(r)
        print(json.dumps(r), flush=True)
    choice = choose_default(rows, block_sizes)
    if choice:
        print(json.dumps(choice), flush=True)
    if args.step:
        for B in (1, 8):
            r = bench_step(B, choice['chosen_block_size'] if choice else None)
            steps.append(r)
            print(json.dumps(r), flush=True)
    if args.md:
        write_md(args.md, rows, steps, choice, block_sizes)


if __name__ == "__main__":
    main()
