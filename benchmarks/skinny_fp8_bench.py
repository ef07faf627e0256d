"""Decode-step GEMMs on e4m3 weights (csrc/kernels/gemm_skinny_f8.hip) against the two paths
a user can compare them with, in one session:

    fp8      ops.skinny_fp8.skinny_kernel on an ops.Fp8Weight   (K * N bytes streamed)
    bf16     ops.skinny.skinny_kernel on the bf16 weight        (2 * K * N bytes; what an
             unquantised model runs, built from the same tree)
    dequant  pa_fp8w_dequant + ops.linear / the unfused SwiGLU expression: the only other
             way a quantised model can compute the product (both flags off)

Products: llama-7b's qkv [4096, 12288], o_proj [4096, 4096], gate|up + SwiGLU [4096, 22016],
down_proj [11008, 4096] and lm_head [4096, 32000], each at M = 1, 4, 8, 16.

Method (benchmarks/skinny_gemm_bench.py): HIP events around a HIP-graph replay of a chain of
calls that rotates over copies of the weight totalling more than twice the 256 MiB last-level
cache, so every call streams its weight from HBM; warm-up first.  The three paths are timed
in interleaved rounds (fp8, bf16, dequant, fp8, ...); the figure is the median round and
``spread`` the (max - min) / median over the rounds of that path.

``--sweep`` adds forced split counts (M = 1 and 8) for each ``--tiles`` geometry (the kernel's
column tile, 256 or 128; the split rule follows it); ``--step`` times a llama-7b ``decode_step``
at B = 1 and 8, context 512, and one 512-token prefill, before and after
``quantize_weights()``, with the weight bytes.

    python benchmarks/skinny_fp8_bench.py --sweep --step --md skinny_fp8_bench_table.md
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
from paddle_amd.ops import _native as N  # noqa: E402
from paddle_amd.ops import skinny, skinny_fp8  # noqa: E402
from paddle_amd.utils import flags  # noqa: E402

HBM_STREAM_TBS = 6.3  # measured float4 copy on MI355X
LLC_BYTES = 256 << 20
ROUNDS = 3
WINDOW_MS = 100.0  # per round and path

# name, K, N, act
PRODUCTS = [
    ("qkv", 4096, 12288, None),
    ("o_proj", 4096, 4096, None),
    ("gate_up+swiglu", 4096, 22016, "swiglu_interleaved"),
    ("down_proj", 11008, 4096, None),
    ("lm_head", 4096, 32000, None),
]
LAYER_PRODUCTS = ("qkv", "o_proj", "gate_up+swiglu", "down_proj")
MS = (1, 4, 8, 16)

_STREAM = []


class Timed:
    """A chain of calls captured once as a HIP graph (after a warm-up on the capture stream);
    ``us()`` replays it for at least WINDOW_MS and returns microseconds per call."""

    def __init__(self, fns):
        if not _STREAM:
            _STREAM.append(torch.cuda.Stream())
        st = _STREAM[0]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for f in fns:
                f()
        torch.cuda.synchronize()
        self.g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g, stream=st):
            for f in fns:
                f()
        self.g.replay()
        torch.cuda.synchronize()
        self.n = len(fns)
        self.reps = None

    def _run(self, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            self.g.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def us(self):
        if self.reps is None:
            self.reps = max(3, math.ceil(3 * WINDOW_MS / max(self._run(3), 1e-3)))
        return self._run(self.reps) * 1e3 / (self.reps * self.n)


def interleaved(paths):
    """{name: Timed} -> {name: (median us, spread)} over ROUNDS interleaved rounds."""
    got = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, t in paths.items():
            got[k].append(t.us())
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in got.items()}


def _weights(K, Nn, dev):
    """Rotating copies of one weight, bf16 and e4m3, each set larger than twice the cache."""
    w = torch.empty(K, Nn, dtype=torch.bfloat16, device=dev).normal_(std=K ** -0.5)
    w8 = ops.quantize_weight_fp8(w)
    n8 = max(2, math.ceil(2 * LLC_BYTES / (K * Nn)) + 1)
    n16 = max(2, math.ceil(2 * LLC_BYTES / (2 * K * Nn)) + 1)
    w8s = [w8] + [ops.Fp8Weight(w8.q.clone(), w8.scale.clone()) for _ in range(n8 - 1)]
    w16s = [w] + [w.clone() for _ in range(n16 - 1)]
    return w16s, w8s


def _dequant_path(x, w8, act):
    prev = flags.get("skinny_fp8"), flags.get("skinny_gemm")
    flags.set("skinny_fp8", False)
    flags.set("skinny_gemm", False)
    try:
        return ops.skinny_linear(x, w8, act=act)
    finally:
        flags.set("skinny_fp8", prev[0])
        flags.set("skinny_gemm", prev[1])


@torch.no_grad()
def bench_product(name, K, Nn, act, sweep, tiles, dev="cuda"):
    w16s, w8s = _weights(K, Nn, dev)
    rows, sweeps = [], []
    default = ops.skinny_fp8_default_splits(Nn, K)
    for M in MS:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        new = skinny_fp8.skinny_kernel(x, w8s[0], act=act).float()
        alt = _dequant_path(x, w8s[0], act).float()
        paths = {
            "fp8": Timed([lambda w=w: skinny_fp8.skinny_kernel(x, w, act=act) for w in w8s]),
            "bf16": Timed([lambda w=w: skinny.skinny_kernel(x, w, act=act) for w in w16s]),
            "dequant": Timed([lambda w=w: _dequant_path(x, w, act) for w in w8s]),
        }
        t = interleaved(paths)
        us8 = t["fp8"][0]
        tbs = K * Nn / (us8 * 1e-6) / 1e12
        r = dict(product=name, K=K, N=Nn, act=act, M=M, routed_to_fp8=bool(ops.skinny_fp8_ok(x, w8s[0], act=act)),
                 default_splits=default, fp8_us=round(us8, 2), fp8_spread=round(t["fp8"][1], 3),
                 bf16_skinny_us=round(t["bf16"][0], 2), bf16_spread=round(t["bf16"][1], 3),
                 dequant_linear_us=round(t["dequant"][0], 2), dequant_spread=round(t["dequant"][1], 3),
                 speedup_vs_bf16=round(t["bf16"][0] / us8, 2), e4m3_bytes=K * Nn, e4m3_TB_per_s=round(tbs, 3),
                 pct_of_hbm_stream=round(100 * tbs / HBM_STREAM_TBS, 1),
                 floor_us=round(K * Nn / (HBM_STREAM_TBS * 1e12) * 1e6, 2),
                 rel_diff_vs_dequant_path=((new - alt).norm() / alt.norm()).item())
        rows.append(r)
        print(json.dumps(r), flush=True)
        del paths
    if sweep:
        for tile in tiles:
            N.lib().pa_gemm_skinny_f8_set_tile(tile)
            dflt = ops.skinny_fp8_default_splits(Nn, K)
            cand = sorted({1, 2, 4, 8, 16, 32, 64, dflt})
            for M in (1, 8):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                us = {}
                for s in cand:
                    if s > 1 and K // s < 64:
                        continue
                    t = Timed([lambda w=w: skinny_fp8.skinny_kernel(x, w, act=act, num_splits=s) for w in w8s])
                    us[s] = round(statistics.median(t.us() for _ in range(ROUNDS)), 2)
                r = dict(product=name, K=K, N=Nn, M=M, tile=tile, default_splits=dflt, us_by_splits=us)
                sweeps.append(r)
                print(json.dumps(r), flush=True)
        N.lib().pa_gemm_skinny_f8_set_tile(256)
    del w16s, w8s
    torch.cuda.empty_cache()
    return rows, sweeps


def _step_ms(model, B, prompt, steps, dev):
    ids = torch.randint(1, model.cfg.vocab_size, (B, prompt), device=dev)
    cache = model.init_cache(B, prompt + steps + 4)
    tok = model.prefill(ids, cache).argmax(-1)
    for _ in range(3):
        tok = model.decode_step(tok, cache).argmax(-1)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        tok = model.decode_step(tok, cache).argmax(-1)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def _prefill_ms(model, prompt, dev, reps=3):
    ids = torch.randint(1, model.cfg.vocab_size, (1, prompt), device=dev)
    cache = model.init_cache(1, prompt + 4)
    model.prefill(ids, cache)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        model.prefill(ids, cache)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def _bytes(model):
    ts = list(model.parameters()) + list(model.buffers())
    total = sum(t.numel() * t.element_size() for t in ts)
    emb = model.embed_tokens.numel() * model.embed_tokens.element_size()
    return total, total - emb  # all, and what a decode step streams (everything but the embedding rows)


@torch.no_grad()
def bench_steps(prompt=512, steps=40, dev="cuda"):
    """llama-7b decode_step at B = 1 and 8 and one prefill, on one model before and after
    quantize_weights()."""
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(**LLAMA_CONFIGS["llama-7b"])
    model = LlamaForCausalLM(cfg, device=dev).eval()
    res = {}
    for tag in ("bf16", "fp8"):
        if tag == "fp8":
            model.quantize_weights()
            torch.cuda.empty_cache()
        total, streamed = _bytes(model)
        res[tag] = dict(model_bytes=total, streamed_bytes=streamed,
                        floor_ms=round(streamed / (HBM_STREAM_TBS * 1e12) * 1e3, 3),
                        prefill_ms=round(_prefill_ms(model, prompt, dev), 2),
                        decode_step_ms={B: round(_step_ms(model, B, prompt, steps, dev), 3) for B in (1, 8)})
    r = dict(model="llama-7b", context=prompt, timing="launch loop", **{k: v for k, v in res.items()})
    print(json.dumps(r), flush=True)
    return r


def write_md(path, rows, sweeps, step):
    with open(path, "w") as f:
        f.write(f"| product | K x N | M | splits | fp8 us (spread) | e4m3 TB/s | % of {HBM_STREAM_TBS} TB/s | "
                "bf16 skinny us (spread) | fp8 vs bf16 | dequant + linear us | routed |\n" + "|---" * 11 + "|\n")
        for r in rows:
            f.write(f"| {r['product']} | {r['K']} x {r['N']} | {r['M']} | {r['default_splits']} | {r['fp8_us']} "
                    f"({100 * r['fp8_spread']:.1f} %) | {r['e4m3_TB_per_s']} | {r['pct_of_hbm_stream']} | "
                    f"{r['bf16_skinny_us']} ({100 * r['bf16_spread']:.1f} %) | {r['speedup_vs_bf16']}x | "
                    f"{r['dequant_linear_us']} | {'yes' if r['routed_to_fp8'] else 'no'} |\n")
        if sweeps:
            f.write("\n| product | M | tile | rule's splits | us by forced split count |\n|---|---|---|---|---|\n")
            for r in sweeps:
                cells = ", ".join(f"{k}: {v}" for k, v in r["us_by_splits"].items())
                f.write(f"| {r['product']} | {r['M']} | {r['tile']} | {r['default_splits']} | {cells} |\n")
        if step:
            f.write("\n| llama-7b, context 512 | model bytes | streamed per step | floor ms | decode ms B 1 | "
                    "decode ms B 8 | 512-token prefill ms |\n|---|---|---|---|---|---|---|\n")
            for tag in ("bf16", "fp8"):
                s = step[tag]
                f.write(f"| {tag} | {s['model_bytes']} | {s['streamed_bytes']} | {s['floor_ms']} | "
                        f"{s['decode_step_ms'][1]} | {s['decode_step_ms'][8]} | {s['prefill_ms']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sweep", action="store_true", help="also time forced split counts per tile geometry")
    ap.add_argument("--tiles", default="256,128", help="column tiles the sweep covers")
    ap.add_argument("--step", action="store_true", help="also time llama-7b decode steps and a prefill")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="o_proj only (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skinny_fp8_bench needs a GPU: a CPU timing says nothing about the kernel")
    tiles = [int(t) for t in args.tiles.split(",")]
    rows, sweeps, step = [], [], None
    for prod in PRODUCTS[1:2] if args.quick else PRODUCTS:
        r, s = bench_product(*prod, sweep=args.sweep, tiles=tiles)
        rows += r
        sweeps += s
    if args.step:
        step = bench_steps()
    if args.md:
        write_md(args.md, rows, sweeps, step)


if __name__ == "__main__":
    main()
