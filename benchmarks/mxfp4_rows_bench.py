"""MXFP4 weight GEMMs at 17..256 rows (csrc/kernels/gemm_rows_mxfp4.hip) against the only other
way a quantised model can compute them, in one session:

    rows     ops.rows_mxfp4.rows_kernel on an ops.Mxfp4Weight   (the packed image, K * N * 17 / 32 bytes)
    dequant  w.dequant() + ops.linear (+ ops.swiglu): the bf16 image written, then read by the GEMM

Products: llama-7b's four layer products, qkv [4096, 12288], o_proj [4096, 4096], gate|up +
SwiGLU [4096, 22016] and down_proj [11008, 4096], each at M = 17, 24, 32, 48, 64, 96, 128, 192, 256.

Method (benchmarks/skinny_mxfp4_bench.py, whose timer this uses): HIP events around a HIP-graph
replay of a chain of calls that rotates over copies of the weight totalling more than twice the
256 MiB last-level cache; the two paths are timed in interleaved rounds; the figure is the
median of 7 rounds and ``spread`` the (max - min) / median over the rounds of that path.  A cell
is won when ``dequant / rows > 1 + dequant spread``.  ``ROUTED_ROWS`` is the largest M of the
list up to which all four products are won at every M.

``--model`` times, eagerly (events around the calls, median of 5 interleaved rounds), one
llama-7b ``decode_step`` at B 32 and context 512 and ``prefill(chunk=64)`` of a 1024-token
prompt with ``FLAGS_mxfp4_rows`` on and off; off takes exactly the calls of the commit before
the kernel.  ``--greedy`` reports where the greedy tokens of the tests' tiny models first differ
between the two settings, and the logit gap there.

    python benchmarks/mxfp4_rows_bench.py --model --greedy --md mxfp4_rows_bench_table.md
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
from paddle_amd.ops import rows_mxfp4  # noqa: E402
from paddle_amd.utils import flags  # noqa: E402
from skinny_mxfp4_bench import LLC_BYTES, PRODUCTS, Timed, interleaved  # noqa: E402

MS = (17, 24, 32, 48, 64, 96, 128, 192, 256)


def _baseline(x, w4, act):
    y = ops.linear(x, w4.dequant())
    return ops.swiglu(y) if act else y


@torch.no_grad()
def bench_product(name, K, Nn, act, dev="cuda"):
    w = torch.empty(K, Nn, dtype=torch.bfloat16, device=dev).normal_(std=K ** -0.5)
    w4 = ops.quantize_weight_mxfp4(w)
    del w
    n4 = max(2, math.ceil(2 * LLC_BYTES / w4.nbytes) + 1)
    w4s = [w4] + [ops.Mxfp4Weight(w4.packed.clone(), w4.scale_e8m0.clone()) for _ in range(n4 - 1)]
    rows = []
    for M in MS:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        paths = {
            "rows": Timed([lambda w=w: rows_mxfp4.rows_kernel(x, w, act=act) for w in w4s]),
            "dequant": Timed([lambda w=w: _baseline(x, w, act) for w in w4s]),
        }
        t = interleaved(paths)
        us, base, spread = t["rows"][0], t["dequant"][0], t["dequant"][1]
        r = dict(product=name, K=K, N=Nn, act=act, M=M, splits=ops.rows_mxfp4_default_splits(Nn, K),
                 rows_us=round(us, 2), rows_spread=round(t["rows"][1], 3), dequant_linear_us=round(base, 2),
                 dequant_spread=round(spread, 3), dequant_over_rows=round(base / us, 3),
                 won=bool(base / us > 1 + spread), weight_TB_per_s=round(w4.nbytes / (us * 1e-6) / 1e12, 3),
                 mfma_TFLOPs=round(2.0 * M * K * Nn / (us * 1e-6) / 1e12, 1))
        rows.append(r)
        print(json.dumps(r), flush=True)
        del paths
    del w4s
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


def _eager_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


@torch.no_grad()
def bench_model(dev="cuda"):
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(**LLAMA_CONFIGS["llama-7b"]), device=dev).eval()
    model.quantize_weights("mxfp4")
    torch.cuda.empty_cache()
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
                flags.set("mxfp4_rows", on)
                t = _eager_ms(fn, reps)
                if rnd:
                    times[on].append(t)
        flags.set("mxfp4_rows", True)
        for on, tag in ((True, "kernel"), (False, "parent")):
            v = times[on]
            got[name][tag] = round(statistics.median(v), 3)
            got[name][tag + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
    r = dict(model="llama-7b mxfp4", timing="eager, median of 5 interleaved rounds", **got)
    print(json.dumps(r), flush=True)
    return r


@torch.no_grad()
def greedy_gap(dev="cuda"):
    """Tiny llama and GPT of the tests, quantised: the first step at which greedy tokens at B 20
    differ between FLAGS_mxfp4_rows on and off, and the gap between the two candidates' logits."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_mxfp4_weight_cpu import tiny

    out = []
    for kind in ("llama", "gpt"):
        model = tiny(kind, dev, "bfloat16")
        model.quantize_weights("mxfp4")
        torch.manual_seed(3)
        ids = torch.randint(1, model.cfg.vocab_size, (20, 12), device=dev)[:, :6]
        caches = {on: model.init_cache(20, 16) for on in (True, False)}
        tok, r = None, dict(model=kind, first_differing_step=None)
        for stp in range(8):
            lg = {}
            for on in (True, False):
                flags.set("mxfp4_rows", on)
                lg[on] = (model.prefill(ids, caches[on]) if stp == 0 else model.decode_step(tok, caches[on])).float()
            flags.set("mxfp4_rows", True)
            a, b = lg[True].argmax(-1), lg[False].argmax(-1)
            if not torch.equal(a, b):
                row = int((a != b).nonzero()[0])
                off = lg[False][row]
                r = dict(model=kind, first_differing_step=stp, row=row, token_on=int(a[row]), token_off=int(b[row]),
                         logit_gap_off=float(off[b[row]] - off[a[row]]), logit_gap_on=float(lg[True][row][a[row]] - lg[True][row][b[row]]),
                         logit_abs_max=float(off.abs().max()), max_logit_diff_on_off=float((lg[True] - lg[False]).abs().max()))
                break
            tok = b  # both runs follow the same tokens up to the first difference
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def write_md(path, rows, model, greedy):
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
            f.write("\n| llama-7b mxfp4, eager | kernel ms (spread) | parent ms (spread) |\n|---|---|---|\n")
            for k in ("decode_step_B32_ctx512_ms", "prefill_chunk64_1024_ms"):
                m = model[k]
                f.write(f"| {k} | {m['kernel']} ({100 * m['kernel_spread']:.1f} %) | {m['parent']} "
                        f"({100 * m['parent_spread']:.1f} %) |\n")
        for g in greedy or []:
            f.write(f"\ngreedy tokens, tiny {g['model']}: {json.dumps(g)}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", action="store_true", help="also time llama-7b decode_step at B 32 and chunked prefill")
    ap.add_argument("--greedy", action="store_true", help="also report the first differing greedy step of the tiny models")
    ap.add_argument("--no-products", action="store_true", help="skip the per-product table")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_rows_bench needs a GPU: a CPU timing says nothing about the kernel")
    rows, model, greedy = [], None, None
    if not args.no_products:
        for prod in PRODUCTS:
            rows += bench_product(*prod)
        print(json.dumps(dict(routed_rows=routed_rows(rows))), flush=True)
    if args.greedy:
        greedy = greedy_gap()
    if args.model:
        model = bench_model()
    if args.md:
        write_md(args.md, rows, model, greedy)


if __name__ == "__main__":
    main()
