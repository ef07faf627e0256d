"""The MFMA decode attention kernel (csrc/kernels/attn_decode_gqa.hip), two tables.

(a) The new ground: heads 20 / 4 and 28 / 4, D 128, B in {1, 8}, 2048 and 8192 cached tokens,
    bf16 and e4m3, contiguous and paged 64.  ``ops.decode_attention`` (the kernel) against what
    these shapes ran before: the plain-torch reference, called directly.  The reference reads
    the lengths on the host, so it cannot be captured: it is timed as an eager call between
    HIP events (median of ``--ref-rounds`` calls), the kernel as a graph replay.  Reported:
    microseconds, and the K / V bytes per second as a share of the 6.3 TB/s streaming figure.
(b) The decision for later: heads 32 / 8 and 32 / 4.  ``_decode_mfma_kernel`` against today's
    ``ops.decode_attention`` (the VALU kernel) with the same ``num_splits``, both as graph
    replays.  The routing of these ratios does not depend on this table.

Method (that of kv_fp8_bench.py): every variant rotates over a set of caches larger than twice
the 256 MiB last-level cache in e4m3 bytes, one pass is captured into a HIP graph, every graph
is warmed up, then ``--repeats`` rounds time every variant of a shape once each (interleaved)
over a window of at least ``--window-ms``.  Reported: the median; the baseline's spread is
(max - min) / median of its rounds.  The cache contents are random and finite (timing only).

    python benchmarks/decode_attn_gqa_bench.py --md decode_attn_gqa_table.md
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
from benchmarks.kv_fp8_bench import KV, _random_fill, _spread  # noqa: E402
from benchmarks.paged_decode_bench import LLC_BYTES, Variant, shuffled_table  # noqa: E402

STREAM_TBS = 6.3
BS = 64
LAYOUTS = ("bf16", "fp8", "bf16_paged", "fp8_paged")


def make_caches(B, Hk, D, L, dev):
    f8_bytes = 2 * B * L * Hk * (D + 4)
    n = max(2, math.ceil(2 * LLC_BYTES / f8_bytes) + 1)
    out = {}
    for name in LAYOUTS:
        kv = KV if name.startswith("fp8") else None
        if name.endswith("paged"):
            c = ops.PagedKVCache(n, B, L, Hk, D, torch.bfloat16, dev, block_size=BS, zero_fill=False, kv_dtype=kv)
            c.load_block_table(shuffled_table(B, c.max_blocks, c.num_blocks, seed=BS))
        else:
            c = ops.KVCache(n, B, L, Hk, D, torch.bfloat16, dev, kv_dtype=kv)
        _random_fill(c)
        out[name] = c
    return n, out


def kv_bytes(name, B, Hk, D, L):
    return 2 * B * L * Hk * ((D + 4) if name.startswith("fp8") else 2 * D)


def timed(variants, repeats, window_ms):
    for v in variants.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants.values():
            v.measure()
    return {k: statistics.median(v.us) for k, v in variants.items()}


def reference_us(q, c, n, kv_len, scale, rounds):
    """The plain-torch path of a refused shape, eagerly (it reads kv_len on the host)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for r in range(rounds + 1):  # the first call warms up
        i = r % n
        torch.cuda.synchronize()
        t0.record()
        k, v = c.gather(i) if getattr(c, "paged", False) else c.dequant(i)
        DEC._decode_attention_ref(q, k, v, kv_len, scale)
        t1.record()
        torch.cuda.synchronize()
        if r:
            us.append(t0.elapsed_time(t1) * 1e3)
    return us


@torch.no_grad()
def bench_new_ground(B, Hq, Hk, D, L, args, dev="cuda"):
    n, caches = make_caches(B, Hk, D, L, dev)
    ns = DEC.default_num_splits(B, Hk, L)
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    variants = {k: Variant(k, [lambda i=i, c=c: ops.decode_attention(q, c, i, num_splits=ns, kv_len=kv_len)
                               for i in range(n)]) for k, c in caches.items()}
    med = timed(variants, args.repeats, args.window_ms)
    out = dict(table="a", B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, num_splits=ns, rotating_caches=n)
    for k, c in caches.items():
        ref = reference_us(q, c, n, kv_len, scale, args.ref_rounds)
        tbs = kv_bytes(k, B, Hk, D, L) / (med[k] * 1e-6) / 1e12
        out.update({f"{k}_us": round(med[k], 2), f"{k}_spread_pct": _spread(variants[k].us),
                    f"{k}_TB_per_s": round(tbs, 3), f"{k}_share_pct": round(100 * tbs / STREAM_TBS, 1),
                    f"{k}_ref_us": round(statistics.median(ref), 1), f"{k}_ref_spread_pct": _spread(ref),
                    f"{k}_speedup": round(statistics.median(ref) / med[k], 1)})
    return out


@torch.no_grad()
def bench_decision(B, Hq, Hk, D, L, args, dev="cuda"):
    n, caches = make_caches(B, Hk, D, L, dev)
    ns = DEC.default_num_splits(B, Hk, L)
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    q = torch.randn(B, 1, Hq, D, device=dev, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    variants = {}
    for k, c in caches.items():
        variants[k + "_valu"] = Variant(k + "_valu", [lambda i=i, c=c: ops.decode_attention(
            q, c, i, num_splits=ns, kv_len=kv_len) for i in range(n)])
        variants[k + "_mfma"] = Variant(k + "_mfma", [lambda i=i, c=c: DEC._decode_mfma_kernel(
            q, c, i, scale, ns, kv_len) for i in range(n)])
    med = timed(variants, args.repeats, args.window_ms)
    out = dict(table="b", B=B, Hq=Hq, Hk=Hk, D=D, cached_len=L, num_splits=ns, rotating_caches=n)
    for k in caches:
        a, b_ = med[k + "_valu"], med[k + "_mfma"]
        sp = _spread(variants[k + "_valu"].us)
        tbs = kv_bytes(k, B, Hk, D, L) / (b_ * 1e-6) / 1e12
        out.update({f"{k}_valu_us": round(a, 2), f"{k}_valu_spread_pct": sp, f"{k}_mfma_us": round(b_, 2),
                    f"{k}_mfma_share_pct": round(100 * tbs / STREAM_TBS, 1), f"{k}_speedup": round(a / b_, 3),
                    f"{k}_faster": bool(b_ < a * (1 - sp / 100))})
    return out


def write_md(path, rows):
    with open(path, "w") as f:
        f.write("(a) kernel against the plain-torch reference\n\n| B | Hq/Hk | cached | splits | storage, layout | "
                "kernel us | spread | TB/s | share of 6.3 TB/s | reference us (eager) | speed-up |\n" + "|---" * 11 + "|\n")
        for r in (r for r in rows if r["table"] == "a"):
            for k in LAYOUTS:
                f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['cached_len']} | {r['num_splits']} | {k} | {r[k + '_us']} | "
                        f"{r[k + '_spread_pct']} % | {r[k + '_TB_per_s']} | {r[k + '_share_pct']} % | {r[k + '_ref_us']} | "
                        f"{r[k + '_speedup']} |\n")
        f.write("\n(b) MFMA kernel against the VALU kernel, same num_splits\n\n| B | Hq/Hk | cached | splits | storage, "
                "layout | VALU us | spread | MFMA us | MFMA share of 6.3 TB/s | VALU / MFMA | beyond the spread |\n"
                + "|---" * 11 + "|\n")
        for r in (r for r in rows if r["table"] == "b"):
            for k in LAYOUTS:
                f.write(f"| {r['B']} | {r['Hq']}/{r['Hk']} | {r['cached_len']} | {r['num_splits']} | {k} | "
                        f"{r[k + '_valu_us']} | {r[k + '_valu_spread_pct']} % | {r[k + '_mfma_us']} | "
                        f"{r[k + '_mfma_share_pct']} % | {r[k + '_speedup']:.3f} | {'yes' if r[k + '_faster'] else 'no'} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=100.0, help="least length of one timed window")
    ap.add_argument("--ref-rounds", type=int, default=5, help="timed eager calls of the reference")
    ap.add_argument("--md", default=None, help="write the two tables as markdown to this file")
    ap.add_argument("--quick", action="store_true", help="one shape per table, 2 rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_attn_gqa_bench needs a GPU: a CPU timing says nothing about the kernel")
    grid = [(B, L) for B in (1, 8) for L in (2048, 8192)]
    new = [(B, Hq, 4, 128, L) for Hq in (20, 28) for B, L in grid]
    old = [(B, 32, Hk, 128, L) for Hk in (8, 4) for B, L in grid]
    if args.quick:
        new, old, args.repeats = new[:1], old[:1], 2
    print(json.dumps(dict(repeats=args.repeats, window_ms=args.window_ms, ref_rounds=args.ref_rounds, block_size=BS)),
          flush=True)
    rows = []
    for fn, shapes in ((bench_new_ground, new), (bench_decision, old)):
        for s in shapes:
            rows.append(fn(*s, args))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.md:
        write_md(args.md, rows)


if __name__ == "__main__":
    main()
