"""Decode-step GEMMs on MXFP4 weights (csrc/kernels/gemm_skinny_mxfp4.hip) against the two paths
a user can compare them with, in one session:

    mxfp4    ops.skinny_mxfp4.skinny_kernel on an ops.Mxfp4Weight   (K * N * 17 / 32 bytes streamed)
    fp8      ops.skinny_fp8.skinny_kernel on an ops.Fp8Weight of the same matrix   (K * N bytes)
    dequant  pa_mxfp4w_dequant + ops.linear / the unfused SwiGLU expression: the only other way
             a quantised model can compute the product (all skinny flags off)

Products: llama-7b's four layer products, qkv [4096, 12288], o_proj [4096, 4096], gate|up +
SwiGLU [4096, 22016] and down_proj [11008, 4096], each at M = 1, 2, 4, 8, 16.

Method (benchmarks/skinny_fp8_bench.py): HIP events around a HIP-graph replay of a chain of
calls that rotates over copies of the weight totalling more than twice the 256 MiB last-level
cache, so every call streams its weight from HBM; warm-up first.  The three paths are timed in
interleaved rounds (mxfp4, fp8, dequant, mxfp4, ...); the figure is the median of 7 rounds and
``spread`` the (max - min) / median over the rounds of that path.  The goal of a cell is
``fp8 / mxfp4 > 1 + fp8 spread``.

``--step`` times one llama-7b ``decode_step`` + sampler as a replayed HIP graph
(``model.decode_graph``) at context 512, B = 1 and 8, with bf16, fp8 and mxfp4 layer weights,
and reports the model's bytes.

    python benchmarks/skinny_mxfp4_bench.py --step --md skinny_mxfp4_bench_table.md
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
from paddle_amd.ops import skinny_fp8, skinny_mxfp4  # noqa: E402
from paddle_amd.utils import flags  # noqa: E402

HBM_STREAM_TBS = 6.3  # measured float4 copy on MI355X
LLC_BYTES = 256 << 20
ROUNDS = 7
WINDOW_MS = 60.0  # per round and path

# name, K, N, act
PRODUCTS = [
    ("qkv", 4096, 12288, None),
    ("o_proj", 4096, 4096, None),
    ("gate_up+swiglu", 4096, 22016, "swiglu_interleaved"),
    ("down_proj", 11008, 4096, None),
]
MS = (1, 2, 4, 8, 16)
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
    """Rotating copies of one weight, mxfp4 and e4m3, each set larger than twice the cache."""
    w = torch.empty(K, Nn, dtype=torch.bfloat16, device=dev).normal_(std=K ** -0.5)
    w4, w8 = ops.quantize_weight_mxfp4(w), ops.quantize_weight_fp8(w)
    n4 = max(2, math.ceil(2 * LLC_BYTES / w4.nbytes) + 1)
    n8 = max(2, math.ceil(2 * LLC_BYTES / w8.nbytes) + 1)
    w4s = [w4] + [ops.Mxfp4Weight(w4.packed.clone(), w4.scale_e8m0.clone()) for _ in range(n4 - 1)]
    w8s = [w8] + [ops.Fp8Weight(w8.q.clone(), w8.scale.clone()) for _ in range(n8 - 1)]
    return w4s, w8s


def _dequant_path(x, w4, act):
    names = ("skinny_mxfp4", "skinny_gemm")
    prev = [flags.get(n) for n in names]
    for n in names:
        flags.set(n, False)
    try:
        return ops.skinny_linear(x, w4, act=act)
    finally:
        for n, v in zip(names, prev):
            flags.set(n, v)


@torch.no_grad()
def bench_product(name, K, Nn, act, dev="cuda"):
    w4s, w8s = _weights(K, Nn, dev)
    rows = []
    nbytes = w4s[0].nbytes
    for M in MS:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        new = skinny_mxfp4.skinny_kernel(x, w4s[0], act=act).float()
        alt = _dequant_path(x, w4s[0], act).float()
        paths = {
            "mxfp4": Timed([lambda w=w: skinny_mxfp4.skinny_kernel(x, w, act=act) for w in w4s]),
            "fp8": Timed([lambda w=w: skinny_fp8.skinny_kernel(x, w, act=act) for w in w8s]),
            "dequant": Timed([lambda w=w: _dequant_path(x, w, act) for w in w4s[:4]]),
        }
        t = interleaved(paths)
        us4, us8 = t["mxfp4"][0], t["fp8"][0]
        tbs = nbytes / (us4 * 1e-6) / 1e12
        ratio = us8 / us4
        r = dict(product=name, K=K, N=Nn, act=act, M=M, splits=ops.skinny_mxfp4_default_splits(Nn, K),
                 mxfp4_us=round(us4, 2), mxfp4_spread=round(t["mxfp4"][1], 3), fp8_us=round(us8, 2),
                 fp8_spread=round(t["fp8"][1], 3), fp8_over_mxfp4=round(ratio, 3),
                 goal_met=bool(ratio > 1 + t["fp8"][1]), dequant_linear_us=round(t["dequant"][0], 2),
                 dequant_spread=round(t["dequant"][1], 3), beats_dequant=bool(us4 < t["dequant"][0]),
                 mxfp4_bytes=nbytes, mxfp4_TB_per_s=round(tbs, 3), pct_of_hbm_stream=round(100 * tbs / HBM_STREAM_TBS, 1),
                 floor_us=round(nbytes / (HBM_STREAM_TBS * 1e12) * 1e6, 2),
                 rel_diff_vs_dequant_path=((new - alt).norm() / alt.norm()).item())
        rows.append(r)
        print(json.dumps(r), flush=True)
        del paths
    del w4s, w8s
    torch.cuda.empty_cache()
    return rows


def _bytes(model):
    ts = list(model.parameters()) + list(model.buffers())
    total = sum(t.numel() * t.element_size() for t in ts)
    emb = model.embed_tokens.numel() * model.embed_tokens.element_size()
    return total, total - emb  # all, and what a decode step streams (everything but the embedding rows)


def _graph_step_ms(model, B, prompt, steps, dev):
    ids = torch.randint(1, model.cfg.vocab_size, (B, prompt), device=dev)
    cache = model.init_cache(B, prompt + 2 * steps + 8)
    st = ops.SamplerState(B, 2 * steps + 8, dev, None, 0)
    ops.sample_step(model.prefill(ids, cache), st, 0, False, 1.0, 0, 1.0)
    g = model.decode_graph(cache, st, 2 * steps + 4)
    for _ in range(3):
        g.step()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        g.step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


@torch.no_grad()
def bench_steps(prompt=512, steps=40, dev="cuda"):
    """llama-7b: one replayed decode step at B = 1 and 8 with bf16, fp8 and mxfp4 layer weights
    (the same random model, built once per format)."""
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    res = {}
    for tag, fmt in (("bf16", None), ("fp8", "fp8_e4m3"), ("mxfp4", "mxfp4")):
        torch.manual_seed(0)
        model = LlamaForCausalLM(LlamaConfig(**LLAMA_CONFIGS["llama-7b"]), device=dev).eval()
        if fmt:
            model.quantize_weights(fmt)
            torch.cuda.empty_cache()
        total, streamed = _bytes(model)
        res[tag] = dict(model_bytes=total, streamed_bytes=streamed,
                        floor_ms=round(streamed / (HBM_STREAM_TBS * 1e12) * 1e3, 3),
                        decode_step_ms={B: round(_graph_step_ms(model, B, prompt, steps, dev), 3) for B in (1, 8)})
        del model
        torch.cuda.empty_cache()
    r = dict(model="llama-7b", context=prompt, timing="graph replay", **res)
    print(json.dumps(r), flush=True)
    return r


def write_md(path, rows, step):
    with open(path, "w") as f:
        if rows:
            f.write(f"| product | K x N | M | splits | mxfp4 us (spread) | TB/s | % of {HBM_STREAM_TBS} TB/s | fp8 us (spread) | "
                    "fp8 / mxfp4 | goal | dequant + linear us |\n" + "|---" * 11 + "|\n")
        for r in rows:
            f.write(f"| {r['product']} | {r['K']} x {r['N']} | {r['M']} | {r['splits']} | {r['mxfp4_us']} "
                    f"({100 * r['mxfp4_spread']:.1f} %) | {r['mxfp4_TB_per_s']} | {r['pct_of_hbm_stream']} | "
                    f"{r['fp8_us']} ({100 * r['fp8_spread']:.1f} %) | {r['fp8_over_mxfp4']}x | "
                    f"{'met' if r['goal_met'] else 'MISSED'} | {r['dequant_linear_us']} |\n")
        if step:
            f.write("\n| llama-7b, context 512, graph replay | model bytes | streamed per step | floor ms | decode ms B 1 | "
                    "decode ms B 8 |\n|---|---|---|---|---|---|\n")
            for tag in ("bf16", "fp8", "mxfp4"):
                s = step[tag]
                f.write(f"| {tag} | {s['model_bytes']} | {s['streamed_bytes']} | {s['floor_ms']} | "
                        f"{s['decode_step_ms'][1]} | {s['decode_step_ms'][8]} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", action="store_true", help="also time llama-7b decode steps as replayed graphs")
    ap.add_argument("--no-products", action="store_true", help="skip the per-product table")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="o_proj only (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skinny_mxfp4_bench needs a GPU: a CPU timing says nothing about the kernel")
    rows, step = [], None
    if not args.no_products:
        for prod in PRODUCTS[1:2] if args.quick else PRODUCTS:
            rows += bench_product(*prod)
    if args.step:
        step = bench_steps()
    if args.md:
        write_md(args.md, rows, step)


if __name__ == "__main__":
    main()
