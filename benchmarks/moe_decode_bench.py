"""``ops.moe_decode_ffn`` (csrc/kernels/moe_decode.hip) against ``MoELayer.forward`` on grouped
experts, on the same rows, in one process, at the ernie-moe-21b-a3b block shape

    H 2560, I 1536, E 64, top-k 6  x  M in {1, 2, 4, 8, 16} rows.

Method (that of paged_decode_bench.py): every variant rotates over ``--layers`` MoE layers with
their own router and 1.5 GB of expert weights each, so the experts a pass selects (M = 1: 6 x
23.6 MB per layer) exceed the 256 MiB last-level cache over a rotation and come from HBM; the
calls of one pass are captured once into a HIP graph and the replay is timed with HIP events, so
launch cost is in neither number.  Every graph is warmed up, then ``--repeats`` rounds each time
both variants once (interleaved, so drift hits both alike) over a window of at least
``--window-ms``.  Reported: the median over the rounds, the baseline's (max - min) / median
spread next to the ratio, and the bytes of the selected experts (distinct experts per layer x
23.6 MB, read from the routing before any timing) per second against the 6.3 TB/s a streaming
read reaches on an MI355X.  Before any timing the two outputs are compared.

``--step`` also times one ``decode_step`` of an ernie-moe-a3b-8l variant with 20 / 5 heads (four
query heads per KV head, which the decode attention kernel takes) at context 512.

    python benchmarks/moe_decode_bench.py --step --md moe_decode_bench_table.md
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
from paddle_amd.distributed.fleet.moe import MoELayer, TopKGate  # noqa: E402
from paddle_amd.models.ernie_moe import (ERNIE_MOE_CONFIGS, ErnieMoEConfig, ErnieMoEForCausalLM,  # noqa: E402
                                         GroupedSwiGLUExperts)

H, I, E, K = 2560, 1536, 64, 6
EXPERT_BYTES = 3 * H * I * 2
STREAM_TBS = 6.3
ROWS = (1, 2, 4, 8, 16)


class Variant:
    """One graph: a pass over the rotating layers (timed as a launch loop, and reported so, if
    the pass cannot be captured)."""

    def __init__(self, name, fns):
        self.name, self.n, self.fns = name, len(fns), fns
        for f in fns:
            f()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph):
                for f in fns:
                    f()
            self.graph.replay()
        except RuntimeError as e:
            print(json.dumps(dict(variant=name, capture_failed=str(e)[:200])), flush=True)
            self.graph = None
        torch.cuda.synchronize()
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.reps = 1
        self.us = []

    def window(self, reps):
        self.t0.record()
        for _ in range(reps):
            if self.graph is not None:
                self.graph.replay()
            else:
                for f in self.fns:
                    f()
        self.t1.record()
        torch.cuda.synchronize()
        return self.t0.elapsed_time(self.t1)  # ms

    def calibrate(self, window_ms):
        ms = self.window(3) / 3
        self.reps = max(3, math.ceil(window_ms / max(ms, 1e-3)))

    def measure(self):
        self.us.append(self.window(self.reps) * 1e3 / (self.reps * self.n))


def make_layers(n, dev):
    layers = []
    for i in range(n):
        experts = GroupedSwiGLUExperts(H, I, range(E), dev, torch.bfloat16, 0.02, lambda e, i=i: 7919 * (i + 1) + e)
        gate = TopKGate(H, E, K, "gshard")
        gate.to(device=dev)
        with torch.no_grad():
            gate.weight.normal_(0.0, 0.05)
        layers.append(MoELayer(H, experts, gate=gate).eval())
    return layers


@torch.no_grad()
def bench_rows(layers, M, repeats, window_ms, dev="cuda"):
    g = torch.Generator(device=dev).manual_seed(M)
    xs = [torch.randn(M, H, device=dev, generator=g).to(torch.bfloat16) for _ in layers]
    args = [(moe.gate.weight, *moe.stacked_experts()) for moe in layers]
    kernel = ops.moe_decode.moe_decode_kernel  # the kernels whatever the routing policy says
    distinct, err = 0, 0.0
    for x, moe, a in zip(xs, layers, args):
        idx, _ = ops.moe_decode_route(x, a[0], K)
        distinct += len(set(idx.reshape(-1).tolist()))
        err = max(err, float((kernel(x, *a, K).float() - moe(x).float()).abs().max()))
    base = Variant("MoELayer.forward", [lambda x=x, moe=moe: moe(x) for x, moe in zip(xs, layers)])
    ours = Variant("moe_decode_ffn", [lambda x=x, a=a: kernel(x, *a, K) for x, a in zip(xs, args)])
    for v in (base, ours):
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in (base, ours):
            v.measure()
    b, o = statistics.median(base.us), statistics.median(ours.us)
    sel = distinct / len(layers) * EXPERT_BYTES
    spread = (max(base.us) - min(base.us)) / b
    return dict(M=M, layers=len(layers), repeats=repeats, distinct_experts_per_layer=round(distinct / len(layers), 2),
                selected_MB=round(sel / 1e6, 1), baseline_us=round(b, 2), baseline_min_us=round(min(base.us), 2),
                baseline_max_us=round(max(base.us), 2), baseline_spread_pct=round(100 * spread, 2),
                moe_decode_us=round(o, 2), moe_decode_spread_pct=round(100 * (max(ours.us) - min(ours.us)) / o, 2),
                ratio=round(o / b, 4), faster_by_more_than_the_spread=bool(o < b * (1 - spread)),
                selected_TB_per_s=round(sel / (o * 1e-6) / 1e12, 3),
                fraction_of_streaming=round(sel / (o * 1e-6) / 1e12 / STREAM_TBS, 3),
                baseline_selected_TB_per_s=round(sel / (b * 1e-6) / 1e12, 3), max_abs_diff=round(err, 5),
                splits=list(ops.moe_decode_default_splits(H, I)),
                timing="graph replay" if base.graph is not None and ours.graph is not None else "launch loop")


@torch.no_grad()
def bench_step(B, prompt=512, steps=32, rounds=3, dev="cuda"):
    """One decode step of ernie-moe-a3b-8l with 20 / 5 heads and grouped experts: the launch loop
    and the replayed graph."""
    torch.manual_seed(0)
    cfg = ErnieMoEConfig(**ERNIE_MOE_CONFIGS["ernie-moe-a3b-8l"], num_key_value_heads=5, grouped_experts=True)
    model = ErnieMoEForCausalLM(cfg, device=dev).eval()
    ids = torch.randint(1, cfg.vocab_size, (B, prompt), device=dev)
    total = (2 * rounds + 2) * steps + 8
    cache = model.init_cache(B, prompt + total)
    st = ops.SamplerState(B, total, dev, None, 0)
    how = (0, False, 1.0, 0, 1.0)
    ops.sample_step(model.prefill(ids, cache), st, *how)
    for _ in range(3):
        ops.sample_step(model.decode_step(st.tok, cache), st, *how)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    loop, replay = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0.record()
        for _ in range(steps):
            ops.sample_step(model.decode_step(st.tok, cache), st, *how)
        t1.record()
        torch.cuda.synchronize()
        loop.append(t0.elapsed_time(t1) / steps)
    graph = model.decode_graph(cache, st, rounds * steps + 4, *how)
    graph.step()
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0.record()
        for _ in range(steps):
            graph.step()
        t1.record()
        torch.cuda.synchronize()
        replay.append(t0.elapsed_time(t1) / steps)
    lo, rp = statistics.median(loop), statistics.median(replay)
    return dict(model="ernie-moe-a3b-8l, 20/5 heads, grouped experts", B=B, context=prompt,
                launch_loop_step_ms=round(lo, 3), launch_loop_spread_pct=round(100 * (max(loop) - min(loop)) / lo, 2),
                graph_step_ms=round(rp, 3), graph_spread_pct=round(100 * (max(replay) - min(replay)) / rp, 2))


def write_md(path, rows, steps):
    with open(path, "w") as f:
        f.write("| M | distinct experts / layer | selected MB | MoELayer.forward us (min-max) | spread | "
                "moe_decode_ffn us | ratio | faster by more than the spread | selected TB/s (of 6.3) | max abs diff |\n")
        f.write("|---" * 10 + "|\n")
        for r in rows:
            f.write(f"| {r['M']} | {r['distinct_experts_per_layer']} | {r['selected_MB']} | {r['baseline_us']} "
                    f"({r['baseline_min_us']}-{r['baseline_max_us']}) | {r['baseline_spread_pct']} % | "
                    f"{r['moe_decode_us']} | {r['ratio']:.3f} | {r['faster_by_more_than_the_spread']} | "
                    f"{r['selected_TB_per_s']} ({r['fraction_of_streaming']:.2f}) | {r['max_abs_diff']} |\n")
        if steps:
            f.write("\n| model | B | context | launch loop step ms | spread | graph step ms | spread |\n"
                    "|---|---|---|---|---|---|---|\n")
            for r in steps:
                f.write(f"| {r['model']} | {r['B']} | {r['context']} | {r['launch_loop_step_ms']} | "
                        f"{r['launch_loop_spread_pct']} % | {r['graph_step_ms']} | {r['graph_spread_pct']} % |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=100.0, help="least length of one timed window")
    ap.add_argument("--layers", type=int, default=4, help="rotating MoE layers (1.5 GB of experts each)")
    ap.add_argument("--step", action="store_true", help="also time an ernie-moe-a3b-8l decode step at B = 1 and 8")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_decode_bench needs a GPU: a CPU timing says nothing about the kernels")
    print(json.dumps(dict(H=H, I=I, E=E, top_k=K, layers=args.layers, repeats=args.repeats, window_ms=args.window_ms,
                          routed_rows_in_tree=ops.moe_decode.ROUTED_ROWS)), flush=True)
    layers = make_layers(args.layers, "cuda")
    rows, steps = [], []
    for M in ROWS:
        r = bench_rows(layers, M, args.repeats, args.window_ms)
        rows.append(r)
        print(json.dumps(r), flush=True)
    del layers
    torch.cuda.empty_cache()
    if args.step:
        for B in (1, 8):
            r = bench_step(B)
            steps.append(r)
            print(json.dumps(r), flush=True)
    if args.md:
        write_md(args.md, rows, steps)


if __name__ == "__main__":
    main()
