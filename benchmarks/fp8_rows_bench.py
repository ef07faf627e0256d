"""Weight-only e4m3 GEMMs at 17..256 rows (csrc/kernels/gemm_rows_f8.hip) against the only other
way a quantised model can compute them, in one session:

    rows     ops.rows_fp8.rows_kernel on an ops.Fp8Weight   (the codes as stored, K * N bytes)
    dequant  w.dequant() + ops.linear (+ ops.swiglu): the bf16 image written, then read by the GEMM

Products: llama-7b's four layer products, qkv [4096, 12288], o_proj [4096, 4096], gate|up +
SwiGLU [4096, 22016] and down_proj [11008, 4096], each at M = 17, 32, 64, 128, 192, 256.

Method (benchmarks/skinny_mxfp4_bench.py, whose timer this uses): HIP events around a HIP-graph
replay of a chain of calls that rotates over copies of the weight totalling more than twice the
256 MiB last-level cache; the two paths are timed in interleaved rounds; the figure is the
median of 7 rounds and ``spread`` the (max - min) / median over the rounds of that path.  A cell
is won when ``dequant / rows > 1 + dequant spread``.  ``ROUTED_ROWS`` is the largest M of the
list up to which all four products are won at every M.

``--model`` times, eagerly (events around the calls, median of 5 interleaved rounds), one
llama-7b ``decode_step`` at B 32 and context 512 and ``prefill(chunk=64)`` of a 1024-token
prompt with ``FLAGS_fp8_rows`` on and off; off takes exactly the calls of the commit before the
kernel.  ``--capture`` tries once whether a decode step at B 32 captures into a graph.

    python benchmarks/fp8_rows_bench.py --model --capture --md fp8_rows_bench_table.md
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddle_amd import ops  # noqa: E402
from paddle_amd.ops import rows_fp8  # noqa: E402
from paddle_amd.utils import flags  # noqa: E402
from mxfp4_rows_bench import _eager_ms  # noqa: E402
from skinny_mxfp4_bench import LLC_BYTES, PRODUCTS, Timed, interleaved  # noqa: E402

MS = (17, 32, 64, 128, 192, 256)


def _baseline(x, w8, act):
    y = ops.linear(x, w8.dequant())
    return ops.swiglu(y) if act else y


@torch.no_grad()
def bench_product(name, K, Nn, act, dev="cuda"):
    w = torch.empty(K, Nn, dtype=torch.bfloat16, device=dev).normal_(std=K ** -0.5)
    w8 = ops.quantize_weight_fp8(w)
    del w
    n8 = max(2, math.ceil(2 * LLC_BYTES / w8.nbytes) + 1)
    w8s = [w8] + [ops.Fp8Weight(w8.q.clone(), w8.scale.clone()) for _ in range(n8 - 1)]
    rows = []
    for M in MS:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        paths = {
            "rows": Timed([lambda w=w: rows_fp8.rows_kernel(x, w, act=act) for w in w8s]),
            "dequant": Timed([lambda w=w: _baseline(x, w, act) for w in w8s]),
        }
        t = interleaved(paths)
        us, base, spread = t["rows"][0], t["dequant"][0], t["dequant"][1]
        r = dict(product=name, K=K, N=Nn, act=act, M=M, splits=ops.rows_fp8_default_splits(Nn, K),
                 rows_us=round(us, 2), rows_spread=round(t["rows"][1], 3), dequant_linear_us=round(base, 2),
                 dequant_spread=round(spread, 3), dequant_over_rows=round(base / us, 3),
                 won=bool(base / us > 1 + spread), weight_TB_per_s=round(w8.nbytes / (us * 1e-6) / 1e12, 3),
                 mfma_TFLOPs=round(2.0 * M * K * Nn / (us * 1e-6) / 1e12, 1))
        rows.append(r)
        print(json.dumps(r), flush=True)
        del paths
    del w8s
    torch.cuda.empty_cache()
    return rows


def routed_rows(rows):
    """The largest M of MS up to which every product is won at every M (0: none)."""
    best = 0
    for M in MS:
        if not all(r["won"] for r in rows if r["M"] == M):
            break
        best = M
    return best


def _llama7b(dev):
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(**LLAMA_CONFIGS["llama-7b"]), device=dev).eval()
    model.quantize_weights()
    torch.cuda.empty_cache()
    return model


@torch.no_grad()
def bench_model(model, dev="cuda"):
    ids = torch.randint(1, model.cfg.vocab_size, (32, 512), device=dev)
    long_ids = torch.randint(1, model.cfg.vocab_size, (1, 1024), device=dev)
    cache = model.init_cache(32, 512 + 128)  # the context grows from 512 to 632 over the 120 timed steps
    pcache = model.init_cache(1, 1024)
    model.prefill(ids, cache)
    got = {"decode_step_B32_ctx512_ms": {}, "prefill_chunk64_1024_ms": {}}
    for name, fn, reps in (("decode_step_B32_ctx512_ms", lambda: model.decode_step(ids[:, 0], cache), 10),
                           ("prefill_chunk64_1024_ms", lambda: model.prefill(long_ids, pcache, chunk=64), 2)):
        times = {True: [], False: []}
        for rnd in range(6):  # the first round warms up
            for on in (True, False):
                flags.set("fp8_rows", on)
                t = _eager_ms(fn, reps)
                if rnd:
                    times[on].append(t)
        flags.set("fp8_rows", True)
        for on, tag in ((True, "kernel"), (False, "parent")):
            v = times[on]
            got[name][tag] = round(statistics.median(v), 3)
            got[name][tag + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
    r = dict(model="llama-7b fp8_e4m3", timing="eager, median of 5 interleaved rounds", **got)
    print(json.dumps(r), flush=True)
    return r


@torch.no_grad()
def try_capture(model, dev="cuda", B=32):
    """One attempt to capture and replay a decode step at B rows (not a promise: reported only)."""
    r = dict(capture_B=B)
    try:
        ids = torch.randint(1, model.cfg.vocab_size, (B, 16), device=dev)
        cache = model.init_cache(B, 64)
        st = ops.SamplerState(B, 32, dev, None, 0)
        ops.sample_step(model.prefill(ids, cache), st, 0, False, 1.0, 0, 1.0)
        g = model.decode_graph(cache, st, 8)
        for _ in range(3):
            g.step()
        torch.cuda.synchronize()
        r.update(captured=True, finite=bool(torch.isfinite(g.logits.float()).all()))
    except Exception as e:  # reported, not raised: capture above 16 rows is not part of the contract
        r.update(captured=False, error=f"{type(e).__name__}: {str(e)[:300]}")
    print(json.dumps(r), flush=True)
    return r


def write_md(path, rows, model, capture):
    with open(path, "w") as f:
        if rows:
            f.write("| product | K x N | M | splits | rows us (spread) | dequant + linear us (spread) | dequant / rows | "
                    "cell | weight TB/s | MFMA TFLOP/s |\n" + "|---" * 10 + "|\n")
            for r in rows:
                f.write(f"| {r['product']} | {r['K']} x {r['N']} | {r['M']} | {r['splits']} | {r['rows_us']} "
                        f"({100 * r['rows_spread']:.1f} %) | {r['dequant_linear_us']} ({100 * r['dequant_spread']:.1f} %) | "
                        f"{r['dequant_over_rows']}x | {'won' if r['won'] else 'LOST'} | {r['weight_TB_per_s']} | "
                        f"{r['mfma_TFLOPs']} |\n")
            f.write(f"\nROUTED_ROWS from this table: {routed_rows(rows)}\n")
        if model:
            f.write("\n| llama-7b fp8_e4m3, eager | kernel ms (spread) | parent ms (spread) |\n|---|---|---|\n")
            for k in ("decode_step_B32_ctx512_ms", "prefill_chunk64_1024_ms"):
                m = model[k]
                f.write(f"| {k} | {m['kernel']} ({100 * m['kernel_spread']:.1f} %) | {m['parent']} "
                        f"({100 * m['parent_spread']:.1f} %) |\n")
        if capture:
            f.write(f"\ngraph capture of a decode step: {json.dumps(capture)}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", action="store_true", help="also time llama-7b decode_step at B 32 and chunked prefill")
    ap.add_argument("--capture", action="store_true", help="also try once to capture a decode step at B 32")
    ap.add_argument("--no-products", action="store_true", help="skip the per-product table")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8_rows_bench needs a GPU: a CPU timing says nothing about the kernel")
    rows, model, capture = [], None, None
    if not args.no_products:
        for prod in PRODUCTS:
            rows += bench_product(*prod)
        print(json.dumps(dict(routed_rows=routed_rows(rows))), flush=True)
    if args.model or args.capture:
        m = _llama7b("cuda")
        if args.model:
            model = bench_model(m)
        if args.capture:
            capture = try_capture(m)
    if args.md:
        write_md(args.md, rows, model, capture)


if __name__ == "__main__":
    main()
