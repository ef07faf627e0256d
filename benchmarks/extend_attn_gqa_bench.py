"""What ``ops.extend_attention`` costs at 5 and 16 query heads per KV head, where it runs the
run-time-ratio kernel of csrc/kernels/attn_extend_gqa.hip, in one process:

kernel    ``extend_attention`` of T in {2, 5, 16} tokens per row for heads 20 / 4 (the
          ernie-moe-21b-a3b preset) and 32 / 2, D = 128, B in {1, 8}, 2048 / 8192 cached tokens,
          {bf16, fp8} x {contiguous, paged 64}, against the two things these shapes could do before:
          (a) T successive ``decode_attention`` calls on the MFMA decode kernel (cached lengths
              L+1 .. L+T), which read the cache T times where the extend kernel reads it once.
              Goal: faster by more than that baseline's run-to-run spread at every 8192-token shape.
          (b) the plain-torch reference ``extend_attention`` ran for these ratios: the dequantised
              copy of the layer for an fp8 or paged cache, a host read of ``base_len``, one row at a
              time.  Reported, no goal.
end to end  one eager ``ops.extend_attention`` call of 5 tokens on the preset's attention shape
          (20 / 4 heads of 128, B = 1, 2048 cached tokens, bf16 contiguous) before (the reference)
          and after (the kernel), launch overhead included.

Method (that of extend_attn_bench.py): every variant rotates over a set of caches larger than twice
the 256 MiB last-level cache in fp8 bytes; the calls of one pass are captured once into a HIP graph
and the replay is timed with HIP events; every graph is warmed up, then ``--repeats`` rounds each
time every variant of a shape once (interleaved) over a window of at least ``--window-ms``.
Reported: the median over the rounds, and next to every ratio the baseline's spread (max - min) /
median.  The reference reads the lengths on the host and cannot be captured: it is timed as a launch
loop, one pass per round over at most ``REF_CACHES`` of the rotating caches (small shapes then stay
in the last-level cache, which favours the baseline).

    FLAGS_allocator_strategy=torch python benchmarks/extend_attn_gqa_bench.py --md extend_attn_gqa_table.md

(torch's own allocator: at B 8, 32 / 2 heads and 8192 tokens one graph holds 17 split workspaces of
68 MB, and the default buddy allocator behind torch cannot take memory from the driver during a
capture).
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
from paddle_amd.ops import decode as DEC  # noqa: E402
from benchmarks.paged_decode_bench import LLC_BYTES, Variant  # noqa: E402
from benchmarks.kv_fp8_bench import _spread  # noqa: E402
from benchmarks.extend_attn_bench import LoopVariant, _caches  # noqa: E402

TS = (2, 5, 16)
REF_CACHES = 8


def reference(q, cache, layer, base):
    """What ``extend_attention`` ran for a ratio its kernel refused."""
    k, v = cache.dequant(layer)
    return DEC._extend_attention_ref(q, k, v, base, 1.0 / math.sqrt(q.shape[-1]))


@torch.no_grad()
def bench_shape(B, Hq, Hk, D, L, repeats, window_ms, dev="cuda"):
    S = L + max(TS)
    f8_bytes = 2 * B * L * Hk * (D + 4)
    n = max(2, math.ceil(2 * LLC_BYTES / f8_bytes) + 1)
    caches = _caches(n, B, S, Hk, D, dev)
    base = torch.full((B,), L, dtype=torch.int32, device=dev)
    graphs, loops = {}, {}
    for T in TS:
        q = torch.randn(B, T, Hq, D, device=dev, dtype=torch.bfloat16)
        lens = [torch.full((B,), L + j + 1, dtype=torch.int32, device=dev) for j in range(T)]
        for name, c in caches.items():
            # the three compute the same thing
            got, want = ops.extend_attention(q, c, 0, base_len=base).float(), reference(q, c, 0, base).float()
            steps = torch.cat([ops.decode_attention(q[:, j:j + 1], c, 0, kv_len=lens[j]) for j in range(T)], 1).float()
            tol = 3e-2 * float(want.abs().max())
            assert float((got - want).abs().max()) < tol and float((steps - want).abs().max()) < tol, (T, name)
            graphs[("extend", name, T)] = Variant(f"extend {name} T{T}", [
                lambda i=i, c=c, q=q: ops.extend_attention(q, c, i, base_len=base) for i in range(n)])
            graphs[("decode", name, T)] = Variant(f"decode {name} T{T}", [
                lambda i=i, c=c, q=q, j=j, lens=lens: ops.decode_attention(q[:, j:j + 1], c, i, kv_len=lens[j])
                for i in range(n) for j in range(T)])
            graphs[("decode", name, T)].n = n  # per pass of T calls over one cache
            loops[(name, T)] = LoopVariant(f"reference {name} T{T}", [
                lambda i=i, c=c, q=q: reference(q, c, i, base) for i in range(min(n, REF_CACHES))])
    for v in graphs.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in list(graphs.values()) + list(loops.values()):
            v.measure()
    rows = []
    for T in TS:
        for name in caches:
            e, d, r = graphs[("extend", name, T)].us, graphs[("decode", name, T)].us, loops[(name, T)].us
            em, dm, rm = statistics.median(e), statistics.median(d), statistics.median(r)
            sp = _spread(d)
            rows.append(dict(B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, T=T, cache=name, rotating_caches=n,
                             extend_splits=ops.default_extend_splits(B, Hk, T, S),
                             decode_splits=DEC.default_num_splits(B, Hk, S),
                             extend_us=round(em, 2), extend_spread_pct=_spread(e), decode_T_calls_us=round(dm, 2),
                             decode_spread_pct=sp, speedup=round(dm / em, 3), byte_ceiling=T,
                             goal_met=bool(em < dm * (1 - sp / 100)), reference_eager_us=round(rm, 1),
                             reference_spread_pct=_spread(r), over_reference=round(rm / em, 1)))
    return rows


@torch.no_grad()
def bench_end_to_end(repeats, dev="cuda"):
    """One eager call on the preset's attention shape: the reference before, the kernel after."""
    B, Hq, Hk, D, L, T = 1, 20, 4, 128, 2048, 5
    n = max(2, math.ceil(2 * LLC_BYTES / (2 * B * L * Hk * D * 2)) + 1)
    c = ops.KVCache(n, B, L + T, Hk, D, torch.bfloat16, dev)
    for i in range(n):
        c.k[i].normal_()
        c.v[i].normal_()
    q = torch.randn(B, T, Hq, D, device=dev, dtype=torch.bfloat16)
    base = torch.full((B,), L, dtype=torch.int32, device=dev)
    before = LoopVariant("reference", [lambda i=i: reference(q, c, i, base) for i in range(n)])
    after = LoopVariant("kernel", [lambda i=i: ops.extend_attention(q, c, i, base_len=base) for i in range(n)])
    for _ in range(repeats):
        before.measure()
        after.measure()
    b, a = statistics.median(before.us), statistics.median(after.us)
    return dict(part="end_to_end", B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, T=T, rotating_caches=n,
                before_reference_us=round(b, 1), before_spread_pct=_spread(before.us), after_kernel_us=round(a, 1),
                after_spread_pct=_spread(after.us), speedup=round(b / a, 1))


def write_md(path, rows, e2e):
    with open(path, "w") as f:
        f.write("| B | Hq/Hk | cached | T | cache | splits ext / dec | extend us | T decode calls us | decode spread | "
                "speed-up (ceiling T) | goal met | reference eager us (spread) | x reference |\n" + "|---" * 13 + "|\n")
        for r in rows:
            f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['cached_len']} | {r['T']} | {r['cache']} | "
                    f"{r['extend_splits']} / {r['decode_splits']} | {r['extend_us']} | {r['decode_T_calls_us']} | "
                    f"{r['decode_spread_pct']} % | {r['speedup']:.2f} | {'yes' if r['goal_met'] else 'NO'} | "
                    f"{r['reference_eager_us']} ({r['reference_spread_pct']} %) | {r['over_reference']} |\n")
        missed = [r for r in rows if r["cached_len"] == 8192 and not r["goal_met"]]
        f.write(f"\nMissed at 8192 cached tokens: {len(missed)} of {sum(r['cached_len'] == 8192 for r in rows)}.\n")
        for r in missed:
            f.write(f"- B {r['B']} {r['Hq']}/{r['Hk']} T {r['T']} {r['cache']}: {r['speedup']:.2f}x, "
                    f"decode spread {r['decode_spread_pct']} %\n")
        if e2e:
            f.write(f"\nEnd to end, one eager `ops.extend_attention` call, {e2e['Hq']}/{e2e['Hk']} heads of {e2e['D']}, "
                    f"B {e2e['B']}, {e2e['cached_len']} cached tokens, T {e2e['T']}, bf16 contiguous: before (plain-torch "
                    f"reference) {e2e['before_reference_us']} us (spread {e2e['before_spread_pct']} %), after (kernel) "
                    f"{e2e['after_kernel_us']} us (spread {e2e['after_spread_pct']} %): {e2e['speedup']}x.\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least length of one timed window")
    ap.add_argument("--md", default=None, help="write the results as a markdown table to this file")
    ap.add_argument("--quick", action="store_true", help="one shape, 2 rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extend_attn_gqa_bench needs a GPU: a CPU timing says nothing about the kernel")
    shapes = [(B, Hq, Hk, 128, L) for Hq, Hk in ((20, 4), (32, 2)) for B in (1, 8) for L in (2048, 8192)]
    if args.quick:
        shapes, args.repeats = shapes[2:3], 2
    print(json.dumps(dict(repeats=args.repeats, window_ms=args.window_ms, reference_caches=REF_CACHES)), flush=True)
    rows = []
    for s in shapes:
        got = bench_shape(*s, repeats=args.repeats, window_ms=args.window_ms)
        rows += got
        for r in got:
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
        if args.md:
            write_md(args.md, rows, None)
    e2e = bench_end_to_end(args.repeats)
    print(json.dumps(e2e), flush=True)
    if args.md:
        write_md(args.md, rows, e2e)


if __name__ == "__main__":
    main()
