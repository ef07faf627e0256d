"""Decode-step GEMMs (M = 1..16) on the skinny-M kernels (csrc/kernels/gemm_skinny.hip)
against the path they replace, in one session.

Products: llama-7b's five decode GEMMs and GPT's tied head,

    qkv      [4096, 12288]            o      [4096, 4096]
    gate|up  [4096, 22016] + SwiGLU   down   [11008, 4096]
    lm_head  [4096, 32000]            tied   [50257, 4096] (K-major)

each at M = 1, 4, 8, 16.  "skinny" is the kernel (``ops.skinny.skinny_kernel``, also where the
default routing of ``ops.skinny_linear`` / ``ops.skinny_linear_t`` leaves a shape to the
parent: ``routed_to_skinny``), "parent" the public op with ``FLAGS_skinny_gemm`` off
(``ops.linear``, the unfused SwiGLU expression, ``ops.linear_t``): both process the same M
rows and the same weights.  One JSON line per (product, M): microseconds for both, weight
bytes per second of the kernel and its share of the 6.3 TB/s HBM streaming figure, the
speed-up, and what the default routing therefore costs (``default_routing_us``).

Method (as decode_attn_bench.py): HIP events around a HIP-graph replay of a chain of calls
that rotates over copies of the weight totalling more than twice the 256 MiB last-level
cache, so every call streams its weight from HBM; warm-up first; the timed window is at
least 250 ms.

``--sweep`` times forced split counts around the default per product (M = 1 and 8);
``--step`` times a llama-7b ``decode_step`` at B = 1 and 8, context 512, flag on and off.

    python benchmarks/skinny_gemm_bench.py --sweep --step --md skinny_gemm_bench_table.md
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
from paddle_amd.ops import skinny  # noqa: E402
from paddle_amd.utils import flags  # noqa: E402

HBM_STREAM_TBS = 6.3  # measured float4 copy on MI355X
LLC_BYTES = 256 << 20
MIN_WINDOW_MS = 250.0

# name, K, N, b_kmaj, act
PRODUCTS = [
    ("qkv", 4096, 12288, False, None),
    ("o_proj", 4096, 4096, False, None),
    ("gate_up+swiglu", 4096, 22016, False, "swiglu_interleaved"),
    ("down_proj", 11008, 4096, False, None),
    ("lm_head", 4096, 32000, False, None),
    ("tied_head", 4096, 50257, True, None),
]
MS = (1, 4, 8, 16)


_STREAM = []


def _time_calls(fns, reps):
    """Mean microseconds per call of ``fns`` run in order, as one replayed HIP graph.  The
    warm-up runs on the stream the graph is captured on, so whatever a path allocates once
    per stream (the vendor BLAS workspace of the parent path) exists before the capture."""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    st = _STREAM[0]
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for f in fns:
            f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(r):
        t0.record()
        for _ in range(r):
            g.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    ms = timed(reps)
    reps = max(reps, math.ceil(reps * MIN_WINDOW_MS / max(ms, 1e-3)))
    return timed(reps) * 1e3 / (reps * len(fns))


def _weights(K, Nn, kmaj, dev):
    wbytes = K * Nn * 2
    n = max(2, math.ceil(2 * LLC_BYTES / wbytes) + 1)
    shape = (Nn, K) if kmaj else (K, Nn)
    ws = []
    for _ in range(n):
        w = torch.empty(shape, dtype=torch.bfloat16, device=dev)
        w.normal_(std=K ** -0.5)
        ws.append(w)
    return ws, wbytes


def _call(x, w, kmaj, act):
    """The public op: the kernel where the default routing sends it, else the parent path."""
    if kmaj:
        return ops.skinny_linear_t(x, w)
    return ops.skinny_linear(x, w, act=act)


def _kernel(x, w, kmaj, act, splits=None):
    """The kernel itself, also for the (shape, M) the default routing leaves to the parent."""
    return skinny.skinny_kernel(x, w, b_kmaj=kmaj, act=act, num_splits=splits)


@torch.no_grad()
def bench_product(name, K, Nn, kmaj, act, sweep, dev="cuda"):
    ws, wbytes = _weights(K, Nn, kmaj, dev)
    rows = []
    default = ops.skinny_default_splits(kmaj, Nn, K)
    for M in MS:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        flags.set("skinny_gemm", True)
        routed = ops.skinny_ok(x, ws[0], b_kmaj=kmaj, act=act)
        new = _kernel(x, ws[0], kmaj, act).float()
        us_new = _time_calls([lambda w=w: _kernel(x, w, kmaj, act) for w in ws], 5)
        flags.set("skinny_gemm", False)
        old = _call(x, ws[0], kmaj, act).float()
        us_old = _time_calls([lambda w=w: _call(x, w, kmaj, act) for w in ws], 5)
        flags.set("skinny_gemm", True)
        tbs = wbytes / (us_new * 1e-6) / 1e12
        r = dict(product=name, K=K, N=Nn, b_kmaj=kmaj, act=act, M=M, routed_to_skinny=bool(routed),
                 default_splits=default, rotating_weights=len(ws), skinny_us=round(us_new, 2),
                 parent_us=round(us_old, 2), speedup=round(us_old / us_new, 2),
                 default_routing_us=round(us_new if routed else us_old, 2), weight_bytes=wbytes,
                 weight_TB_per_s=round(tbs, 3), pct_of_hbm_stream=round(100 * tbs / HBM_STREAM_TBS, 1),
                 floor_us=round(wbytes / (HBM_STREAM_TBS * 1e12) * 1e6, 2),
                 rel_diff_vs_parent=((new - old).norm() / old.norm()).item())
        rows.append(r)
        print(json.dumps(r), flush=True)
    sweeps = []
    if sweep:
        cand = sorted({1, 2, 4, 8, 16, 32, max(1, default // 2), default, min(64, default * 2)})
        for M in (1, 8):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            us = {}
            for s in cand:
                if s > 1 and K // s < 64:
                    continue
                us[s] = round(_time_calls([lambda w=w: _kernel(x, w, kmaj, act, s) for w in ws], 3), 2)
            r = dict(product=name, K=K, N=Nn, b_kmaj=kmaj, M=M, default_splits=default, us_by_splits=us)
            sweeps.append(r)
            print(json.dumps(r), flush=True)
    del ws
    torch.cuda.empty_cache()
    return rows, sweeps


@torch.no_grad()
def bench_steps(prompt=512, steps=40, dev="cuda"):
    """llama-7b decode_step at B = 1 and 8, with the flag on and off, on one model."""
    from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(**LLAMA_CONFIGS["llama-7b"])
    model = LlamaForCausalLM(cfg, device=dev).eval()
    wbytes = 2 * sum(p.numel() for n, p in model.named_parameters() if p.dim() == 2 and n != "embed_tokens")
    out = []
    for B in (1, 8):
        ids = torch.randint(1, cfg.vocab_size, (B, prompt), device=dev)
        res = {}
        for on in (True, False):
            flags.set("skinny_gemm", on)
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
            res[on] = t0.elapsed_time(t1) / steps
            del cache
        flags.set("skinny_gemm", True)
        r = dict(model="llama-7b", B=B, context=prompt, decode_step_ms_skinny=round(res[True], 3),
                 decode_step_ms_parent=round(res[False], 3), speedup=round(res[False] / res[True], 2),
                 weight_bytes=wbytes, weight_stream_floor_ms=round(wbytes / (HBM_STREAM_TBS * 1e12) * 1e3, 3),
                 timing="launch loop")
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def write_md(path, rows, sweeps, steps):
    with open(path, "w") as f:
        f.write(f"| product | K x N | M | splits | skinny us | weight TB/s | % of {HBM_STREAM_TBS} TB/s | parent us | "
                "speed-up | routed | default routing us |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['product']} | {r['K']} x {r['N']}{' (K-major)' if r['b_kmaj'] else ''} | {r['M']} | "
                    f"{r['default_splits']} | {r['skinny_us']} | {r['weight_TB_per_s']} | {r['pct_of_hbm_stream']} | "
                    f"{r['parent_us']} | {r['speedup']}x | {'yes' if r['routed_to_skinny'] else 'no'} | "
                    f"{r['default_routing_us']} |\n")
        if sweeps:
            f.write("\n| product | M | default splits | us by forced split count |\n|---|---|---|---|\n")
            for r in sweeps:
                cells = ", ".join(f"{k}: {v}" for k, v in r["us_by_splits"].items())
                f.write(f"| {r['product']} | {r['M']} | {r['default_splits']} | {cells} |\n")
        if steps:
            f.write("\n| model | B | context | decode step ms (skinny) | decode step ms (parent) | speed-up | "
                    "weight-stream floor ms |\n|---|---|---|---|---|---|---|\n")
            for r in steps:
                f.write(f"| {r['model']} | {r['B']} | {r['context']} | {r['decode_step_ms_skinny']} | "
                        f"{r['decode_step_ms_parent']} | {r['speedup']}x | {r['weight_stream_floor_ms']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sweep", action="store_true", help="also time forced split counts around the default")
    ap.add_argument("--step", action="store_true", help="also time a llama-7b decode step at B = 1 and 8")
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="first product only (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skinny_gemm_bench needs a GPU: a CPU timing says nothing about the kernel")
    rows, sweeps, steps = [], [], []
    for prod in PRODUCTS[:1] if args.quick else PRODUCTS:
        r, s = bench_product(*prod, sweep=args.sweep)
        rows += r
        sweeps += s
    if args.step:
        steps = bench_steps()
    if args.md:
        write_md(args.md, rows, sweeps, steps)


if __name__ == "__main__":
    main()
