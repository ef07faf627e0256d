"""What speculative decoding costs (ops/speculative.py, models/speculative.py), in one process:

verify   ``ops.spec_judge`` + ``ops.spec_commit`` (csrc/kernels/spec_verify.hip) over target and
         draft logits [B, G+1, V] / [B, G, V] against ``G + 1`` launches of the sampling kernel
         over the same target logits -- all the code could do before -- for B in {1, 8} x G in
         {4, 8} x V in {32000, 50257} x {greedy, sampled (temperature 0.8, top-k 50, top-p 0.9)},
         bf16.  Goal: faster than the ``G + 1`` launches by more than their run-to-run spread at
         every shape.
round    llama-7b (random weights), context 512, B in {1, 8}, G in {2, 4, 8}, greedy, with two
         drafts: an 8-layer model of the target's configuration, and a copy of the target after
         ``quantize_weights()``.  One round split into draft (``G + 1`` decode steps and ``G``
         token selections), ``extend``, verify and the host read of ``kept``, next to one plain
         ``decode_step`` + ``sample_step`` as a launch loop and as ``DecodeGraph`` replay, and the
         break-even tokens per round ``t_round / t_step`` against either.  For the fp8 draft also
         ``generate(draft=...)`` end to end: the acceptance measured and tokens/s against plain
         ``generate()`` (launch loop and ``graph=True``).

Method (that of extend_attn_bench.py): the verify part captures one pass over ``--buffers``
sets of logits into a HIP graph per variant and times replays with HIP events over windows of
at least ``--window-ms``; every variant of a shape is timed once per round, interleaved;
reported are the median over ``--repeats`` rounds and, next to every ratio, the baseline's spread
(max - min) / median.  The logits are not rotated out of the last-level cache: in generation
they have just been written by the LM head.  The round part times launch loops with HIP events
(``extend`` and the host read do not capture), median of ``--model-rounds`` rounds.

    python benchmarks/spec_decode_bench.py --model --md spec_decode_table.md
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddle_amd import ops  # noqa: E402
from paddle_amd.ops import sampling as S  # noqa: E402
from benchmarks.paged_decode_bench import Variant  # noqa: E402
from benchmarks.kv_fp8_bench import _llama7b, _random_fill, _spread  # noqa: E402
from benchmarks.extend_attn_bench import _timed  # noqa: E402

SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.9)
SEED = 1234


@torch.no_grad()
def bench_verify(B, G, V, do_sample, buffers, repeats, window_ms, dev="cuda"):
    how = (do_sample, SAMPLED["temperature"], SAMPLED["top_k"], SAMPLED["top_p"]) if do_sample else (False, 1.0, 0, 1.0)
    g = torch.Generator(device=dev).manual_seed(V + G)
    tl = [(torch.randn(B, G + 1, V, device=dev, generator=g) * 3).bfloat16() for _ in range(buffers)]
    dl = [(t[:, :G].float() + torch.randn(B, G, V, device=dev, generator=g)).bfloat16() for t in tl]
    cand = [ops.sample_tokens(d.reshape(B * G, V), SEED, 1, *how).view(B, G) for d in dl]
    st = ops.SpecState(B, buffers * (G + 1) + 1, G, dev)
    outs = (torch.empty(B, G, dtype=torch.bool, device=dev), torch.empty(B, G + 1, dtype=torch.long, device=dev))
    tok = torch.empty(B, dtype=torch.long, device=dev)

    def verify(i):
        if i == 0:  # the state starts over once per pass: two fills, counted against this side
            st.pos.zero_()
            st.done.zero_()
        a, l_ = ops.spec_judge(tl[i], cand[i], dl[i] if do_sample else None, SEED, i, *how, out=outs)
        ops.spec_commit(a, l_, cand[i], st)

    def samples(i):
        for j in range(G + 1):
            S._launch(tl[i][:, j], SEED, None, j, *how, tok, None)

    assert ops.spec_kernel_ok(tl[0], dl[0], do_sample)
    variants = {"verify": Variant("verify", [lambda i=i: verify(i) for i in range(buffers)]),
                "samples": Variant("samples", [lambda i=i: samples(i) for i in range(buffers)])}
    for v in variants.values():
        v.calibrate(window_ms)
    for _ in range(repeats):
        for v in variants.values():
            v.measure()
    a, b_ = variants["verify"].us, variants["samples"].us
    am, bm, sp = statistics.median(a), statistics.median(b_), _spread(b_)
    return dict(part="verify", B=B, G=G, V=V, mode="sampled" if do_sample else "greedy", verify_us=round(am, 2),
                verify_spread_pct=_spread(a), samples_us=round(bm, 2), samples_spread_pct=sp,
                speedup=round(bm / am, 3), goal_met=bool(am < bm * (1 - sp / 100)))


def _median_ms(fn, setup, rounds):
    ms = _timed(fn, setup, rounds)
    return statistics.median(ms), _spread(ms)


@torch.no_grad()
def bench_round(target, draft, draft_name, B, G, rounds, ctx=512, dev="cuda"):
    V = target.cfg.vocab_size
    tcache, dcache = target.init_cache(B, ctx + G + 24), draft.init_cache(B, ctx + G + 24)
    _random_fill(tcache)
    _random_fill(dcache)
    st = ops.SpecState(B, 4 * (G + 1), G, dev)
    x0 = torch.randint(1, V, (B,), device=dev)
    cand = torch.randint(1, V, (B, G), device=dev)
    feed = torch.cat([x0[:, None], cand], 1)
    box = {}

    def reset():
        tcache.set_lens([ctx] * B)
        dcache.set_lens([ctx] * B)
        st.pos.fill_(1)
        st.done.zero_()

    def draft_part():
        x = x0
        for j in range(G):
            x = ops.sample_tokens(draft.decode_step(x, dcache), SEED, 1 + j)
            cand[:, j] = x
        draft.decode_step(x, dcache)

    def extend_part():
        box["tl"] = target.extend(feed, tcache, all_logits=True)

    def verify_part():
        ops.spec_verify(box["tl"], cand, None, st, SEED, 0)

    def read_part():
        box["kept"] = st.kept.tolist()

    def whole():
        draft_part()
        feed[:, 1:] = cand
        extend_part()
        verify_part()
        read_part()
        back = [G + 1 - k for k in box["kept"]]
        tcache.rewind_each(back, bound=ctx + G + 1)
        dcache.rewind_each(back, bound=ctx + G + 1)

    reset()
    extend_part()
    out = dict(part="round", draft=draft_name, B=B, G=G, context=ctx)
    for name, fn in (("draft", draft_part), ("extend", extend_part), ("verify", verify_part), ("read", read_part),
                     ("round", whole)):
        m, sp = _median_ms(fn, reset, rounds)
        out[f"{name}_ms"] = round(m, 3)
        out[f"{name}_spread_pct"] = sp
    # one plain step: the launch loop and the graph replay of the parent's generate()
    pst = ops.SamplerState(B, 64, dev)
    steps = 16

    def loop():
        for _ in range(steps):
            ops.sample_step(target.decode_step(pst.tok, tcache), pst)

    m, sp = _median_ms(loop, reset, rounds)
    out["step_loop_ms"], out["step_loop_spread_pct"] = round(m / steps, 3), sp
    reset()
    graph = target.decode_graph(tcache, pst, steps=(rounds + 2) * steps)

    def replay():
        for _ in range(steps):
            graph.step()

    m, sp = _median_ms(replay, reset, rounds)
    out["step_graph_ms"], out["step_graph_spread_pct"] = round(m / steps, 3), sp
    out["break_even_vs_loop"] = round(out["round_ms"] / out["step_loop_ms"], 2)
    out["break_even_vs_graph"] = round(out["round_ms"] / out["step_graph_ms"], 2)
    return out


@torch.no_grad()
def bench_generate(target, draft, draft_name, B, G, new, rounds, ctx=512, dev="cuda"):
    ids = torch.randint(1, target.cfg.vocab_size, (B, ctx), device=dev)

    def wall(**kw):
        ts = []
        for rnd in range(rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            target.generate(ids, new, sampler="philox", seed=SEED, **kw)
            torch.cuda.synchronize()
            if rnd:
                ts.append(time.perf_counter() - t)
        return statistics.median(ts), _spread(ts)

    loop, loop_sp = wall()
    graph, graph_sp = wall(graph=True)
    spec, spec_sp = wall(draft=draft, num_draft=G)
    s = target.last_speculation
    return dict(part="generate", draft=draft_name, B=B, G=G, context=ctx, new_tokens=new, rounds=s.rounds,
                proposed=s.proposed, accepted=s.accepted, acceptance=round(s.accepted / max(s.proposed, 1), 3),
                tokens_per_round=round((s.emitted - B) / max(s.rounds, 1) / B, 2),
                loop_tok_s=round(B * new / loop, 1), loop_spread_pct=loop_sp, graph_tok_s=round(B * new / graph, 1),
                graph_spread_pct=graph_sp, spec_tok_s=round(B * new / spec, 1), spec_spread_pct=spec_sp,
                spec_over_loop=round(loop / spec, 3), spec_over_graph=round(graph / spec, 3))


def write_md(path, verify, rounds_, gens):
    with open(path, "w") as f:
        if verify:
            f.write("| B | G | V | mode | judge + commit us | G+1 sample launches us (spread) | speed-up | goal met |\n"
                    + "|---" * 8 + "|\n")
        for r in verify:
            f.write(f"| {r['B']} | {r['G']} | {r['V']} | {r['mode']} | {r['verify_us']} | {r['samples_us']} "
                    f"({r['samples_spread_pct']} %) | {r['speedup']:.2f} | {'yes' if r['goal_met'] else 'NO'} |\n")
        if rounds_:
            f.write("\n| draft | B | G | draft ms | extend ms | verify ms | read ms | round ms (spread) | "
                    "step loop ms (spread) | step graph ms (spread) | break-even vs loop | vs graph |\n"
                    + "|---" * 12 + "|\n")
        for r in rounds_:
            f.write(f"| {r['draft']} | {r['B']} | {r['G']} | {r['draft_ms']} | {r['extend_ms']} | {r['verify_ms']} | "
                    f"{r['read_ms']} | {r['round_ms']} ({r['round_spread_pct']} %) | {r['step_loop_ms']} "
                    f"({r['step_loop_spread_pct']} %) | {r['step_graph_ms']} ({r['step_graph_spread_pct']} %) | "
                    f"{r['break_even_vs_loop']} | {r['break_even_vs_graph']} |\n")
        if gens:
            f.write("\n| draft | B | G | new | rounds | accepted / proposed | tokens per round and row | "
                    "loop tok/s (spread) | graph tok/s (spread) | speculative tok/s (spread) | x loop | x graph |\n"
                    + "|---" * 12 + "|\n")
        for r in gens:
            f.write(f"| {r['draft']} | {r['B']} | {r['G']} | {r['new_tokens']} | {r['rounds']} | {r['accepted']} / "
                    f"{r['proposed']} ({r['acceptance']}) | {r['tokens_per_round']} | {r['loop_tok_s']} "
                    f"({r['loop_spread_pct']} %) | {r['graph_tok_s']} ({r['graph_spread_pct']} %) | {r['spec_tok_s']} "
                    f"({r['spec_spread_pct']} %) | {r['spec_over_loop']} | {r['spec_over_graph']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7, help="timed rounds per variant (the median is reported)")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least length of one timed window")
    ap.add_argument("--buffers", type=int, default=4, help="sets of logits one captured pass walks over")
    ap.add_argument("--model", action="store_true", help="also time llama-7b rounds and generate(draft=...)")
    ap.add_argument("--only-model", action="store_true", help="skip the verify part")
    ap.add_argument("--model-rounds", type=int, default=7)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--md", default=None, help="write the results as markdown tables to this file")
    ap.add_argument("--quick", action="store_true", help="one shape per part, 2 rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_decode_bench needs a GPU: a CPU timing says nothing about the kernel")
    shapes = [(B, G, V, m) for B in (1, 8) for G in (4, 8) for V in (32000, 50257) for m in (False, True)]
    model_shapes = [(B, G) for B in (1, 8) for G in (2, 4, 8)]
    if args.quick:
        shapes, model_shapes, args.repeats, args.model_rounds, args.new_tokens = shapes[:2], model_shapes[:1], 2, 2, 16
    if args.only_model:
        shapes, args.model = [], True
    print(json.dumps(dict(repeats=args.repeats, window_ms=args.window_ms, buffers=args.buffers,
                          model_rounds=args.model_rounds)), flush=True)
    verify, rounds_, gens = [], [], []
    for s in shapes:
        verify.append(bench_verify(*s, buffers=args.buffers, repeats=args.repeats, window_ms=args.window_ms))
        print(json.dumps(verify[-1]), flush=True)
    if args.md:
        write_md(args.md, verify, rounds_, gens)
    if args.model:
        from paddle_amd.models.llama import LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM

        target = _llama7b("cuda")
        torch.manual_seed(1)
        cfg8 = dict(LLAMA_CONFIGS["llama-7b"], num_hidden_layers=8)
        small = LlamaForCausalLM(LlamaConfig(**cfg8, max_position_embeddings=8192), device="cuda").eval()
        for B, G in model_shapes:
            rounds_.append(bench_round(target, small, "8 layers", B, G, args.model_rounds))
            print(json.dumps(rounds_[-1]), flush=True)
        del small
        torch.cuda.empty_cache()
        fp8 = copy.deepcopy(target).quantize_weights()
        torch.cuda.empty_cache()
        for B, G in model_shapes:
            rounds_.append(bench_round(target, fp8, "fp8 copy", B, G, args.model_rounds))
            print(json.dumps(rounds_[-1]), flush=True)
            gens.append(bench_generate(target, fp8, "fp8 copy", B, G, args.new_tokens, min(args.model_rounds, 3)))
            print(json.dumps(gens[-1]), flush=True)
            if args.md:
                write_md(args.md, verify, rounds_, gens)
    if args.md:
        write_md(args.md, verify, rounds_, gens)


if __name__ == "__main__":
    main()
