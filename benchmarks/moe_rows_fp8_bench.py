"""The quantised MoE expert MLP above 16 rows: ``ops.grouped_fp8w_kernel`` (csrc/kernels/
moe_rows_f8.hip, the e4m3 codes as stored) against the only other way a quantised model can
compute it, in one process:

    rows     ops.grouped_fp8w_kernel(x_sorted, gate_up, down, counts)
    dequant  gate_up.dequant(), down.dequant() + ops.grouped.grouped_swiglu_mlp: two bf16 images
             of the whole layer written, then read by the bf16 ragged grouped GEMM

at the ernie-moe-a3b shapes (H 2560, I 1536, E 64, k 6) and 17, 32, 64, 128, 256, 1024 and 4096
tokens.  The routing is the real gate's (``TopKGate`` with its initial weight) on N(0, 1)
activations, sorted by ``ops.moe_route``; ``counts`` stays on the device for both paths.

Method: HIP events around a launch loop of each path (the model runs these calls eagerly above
16 rows), windows of at least 60 ms, the two paths in interleaved rounds; the figure is the
median of 7 rounds and ``spread`` is (max - min) / median over the rounds of a path.  One layer's
codes are 0.75 GB, and every call reads at least the experts that have rows: more than twice the
256 MiB last-level cache at every token count, so no rotation over copies is needed.  A cell is
won when ``dequant / rows > 1 + rows spread + dequant spread``.  ``TB/s`` is the bytes of the
codes of the experts that had rows (both stacks) over the time of the call, and ``share`` that
over 6.3 TB/s.  Before any timing the two outputs are compared.

``--model`` times, eagerly, one ``decode_step`` at B 32 (context 512) and one ``prefill`` of a
1024-token prompt of ernie-moe-a3b-8l (20 / 5 heads, grouped experts) after ``quantize_weights()``
with ``FLAGS_moe_rows_fp8`` on and off; off takes exactly the calls of the commit before the
kernel.

    python benchmarks/moe_rows_fp8_bench.py --model --md moe_rows_fp8_table.md
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
from paddle_amd.distributed.fleet.moe import TopKGate  # noqa: E402
from paddle_amd.ops import grouped as _grouped  # noqa: E402
from paddle_amd.ops import moe_route as _route  # noqa: E402
from paddle_amd.utils import flags  # noqa: E402

H, I, E, K_TOP = 2560, 1536, 64, 6
TOKENS = (17, 32, 64, 128, 256, 1024, 4096)
ROUNDS = 7
WINDOW_MS = 60.0
PEAK_TBS = 6.3


def _window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def interleaved(paths):
    """{name: fn} -> {name: (median us, spread)} over ROUNDS interleaved rounds."""
    reps = {}
    for k, fn in paths.items():
        fn()
        torch.cuda.synchronize()
        reps[k] = max(3, math.ceil(3 * WINDOW_MS / max(_window_ms(fn, 3), 1e-3)))
    got = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            got[k].append(_window_ms(fn, reps[k]) * 1e3 / reps[k])
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in got.items()}


def _baseline(x, gu8, dn8, counts):
    return _grouped.grouped_swiglu_mlp(x, gu8.dequant(), dn8.dequant(), counts)


@torch.no_grad()
def bench_layer(dev="cuda"):
    torch.manual_seed(0)
    gate = TopKGate(H, E, K_TOP, "gshard", None).to(dev)
    gu8 = ops.quantize_experts_fp8(torch.empty(E, H, 2 * I, dtype=torch.bfloat16, device=dev).normal_(std=H ** -0.5))
    dn8 = ops.quantize_experts_fp8(torch.empty(E, I, H, dtype=torch.bfloat16, device=dev).normal_(std=I ** -0.5))
    torch.cuda.empty_cache()
    per_expert = (gu8.q[0].numel() + dn8.q[0].numel())
    rows = []
    for T in TOKENS:
        xt = torch.randn(T, H, device=dev, dtype=torch.bfloat16)
        _, idx, _ = gate(xt)
        src, pos, _, counts = _route.route(idx.reshape(-1), T, K_TOP, E, None)
        x = _route.dispatch(xt, src, pos, K_TOP)
        live = int((counts > 0).sum())
        new, old = ops.grouped_fp8w_kernel(x, gu8, dn8, counts).float(), _baseline(x, gu8, dn8, counts).float()
        diff = float((new - old).abs().max() / old.abs().max())
        t = interleaved({"rows": lambda: ops.grouped_fp8w_kernel(x, gu8, dn8, counts),
                         "dequant": lambda: _baseline(x, gu8, dn8, counts)})
        (us, sp), (base, bsp) = t["rows"], t["dequant"]
        tbs = live * per_expert / (us * 1e-6) / 1e12
        r = dict(tokens=T, sorted_rows=int(x.shape[0]), experts_with_rows=live, max_rows_per_expert=int(counts.max()),
                 rows_us=round(us, 1), rows_spread=round(sp, 3), dequant_us=round(base, 1), dequant_spread=round(bsp, 3),
                 dequant_over_rows=round(base / us, 3), won=bool(base / us > 1 + sp + bsp),
                 code_TB_per_s=round(tbs, 3), share_of_peak=round(tbs / PEAK_TBS, 3), max_rel_diff=round(diff, 5))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def routed_sorted_rows(rows):
    """The largest sorted-row count of the list up to which every count is won; None (no limit)
    when none is lost, 0 when the first is."""
    best = 0
    for r in rows:
        if not r["won"]:
            return best
        best = r["sorted_rows"]
    return None


@torch.no_grad()
def bench_model(dev="cuda"):
    from paddle_amd.models.ernie_moe import ERNIE_MOE_CONFIGS, ErnieMoEConfig, ErnieMoEForCausalLM

    torch.manual_seed(0)
    cfg = ErnieMoEConfig(**ERNIE_MOE_CONFIGS["ernie-moe-a3b-8l"], num_key_value_heads=5, grouped_experts=True)
    model = ErnieMoEForCausalLM(cfg, device=dev).eval()
    model.quantize_weights()
    torch.cuda.empty_cache()
    ids = torch.randint(1, cfg.vocab_size, (32, 512), device=dev)
    long_ids = torch.randint(1, cfg.vocab_size, (1, 1024), device=dev)
    cache = model.init_cache(32, 512 + 80)  # the context grows from 512 over the timed steps
    pcache = model.init_cache(1, 1024)
    model.prefill(ids, cache)
    got = {}
    for name, fn, reps in (("decode_step_B32_ctx512_ms", lambda: model.decode_step(ids[:, 0], cache), 5),
                           ("prefill_1024_ms", lambda: model.prefill(long_ids, pcache), 2)):
        times = {True: [], False: []}
        for rnd in range(6):  # the first round warms up
            for on in (True, False):
                flags.set("moe_rows_fp8", on)
                torch.cuda.synchronize()
                t = _window_ms(fn, reps) / reps
                if rnd:
                    times[on].append(t)
        flags.set("moe_rows_fp8", True)
        got[name] = {}
        for on, tag in ((True, "kernel"), (False, "parent")):
            v = times[on]
            got[name][tag] = round(statistics.median(v), 3)
            got[name][tag + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
    r = dict(model="ernie-moe-a3b-8l, 20/5 heads, grouped experts, quantize_weights()",
             timing="launch loop, median of 5 interleaved rounds", **got)
    print(json.dumps(r), flush=True)
    return r


def write_md(path, rows, model):
    with open(path, "w") as f:
        if rows:
            f.write("| tokens | sorted rows | experts with rows | rows us (spread) | dequant + grouped us (spread) | "
                    "dequant / rows | cell | code TB/s | share of 6.3 TB/s |\n" + "|---" * 9 + "|\n")
            for r in rows:
                f.write(f"| {r['tokens']} | {r['sorted_rows']} | {r['experts_with_rows']} | {r['rows_us']} "
                        f"({100 * r['rows_spread']:.1f} %) | {r['dequant_us']} ({100 * r['dequant_spread']:.1f} %) | "
                        f"{r['dequant_over_rows']}x | {'won' if r['won'] else 'LOST'} | {r['code_TB_per_s']} | "
                        f"{100 * r['share_of_peak']:.1f} % |\n")
            f.write(f"\nROUTED_SORTED_ROWS from this table: {routed_sorted_rows(rows)}\n")
        if model:
            f.write("\n| quantised ernie-moe-a3b-8l, launch loop | kernel ms (spread) | parent ms (spread) |\n|---|---|---|\n")
            for k in ("decode_step_B32_ctx512_ms", "prefill_1024_ms"):
                m = model[k]
                f.write(f"| {k} | {m['kernel']} ({100 * m['kernel_spread']:.1f} %) | {m['parent']} "
                        f"({100 * m['parent_spread']:.1f} %) |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", action="store_true", help="also time decode_step at B 32 and a 1024-token prefill")
    ap.add_argument("--no-layer", action="store_true", help="skip the per-layer table")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_rows_fp8_bench needs a GPU: a CPU timing says nothing about the kernel")
    rows, model = [], None
    if not args.no_layer:
        rows = bench_layer()
        print(json.dumps(dict(routed_sorted_rows=routed_sorted_rows(rows))), flush=True)
    if args.model:
        model = bench_model()
    if args.md:
        write_md(args.md, rows, model)


if __name__ == "__main__":
    main()
