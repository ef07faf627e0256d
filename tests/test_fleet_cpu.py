"""Fleet hybrid parallelism on CPU (gloo, multi-process): every axis is checked
against a single-process reference run of the same model on the same data."""
import pytest
import torch

from paddle_amd import ops

from dist_util import assert_adam_close, run_dist
from paddle_amd.distributed.topology import CommunicateTopology
from paddle_amd.models.llama import (LLAMA_CONFIGS, LlamaConfig, LlamaForCausalLM, LlamaPretrainingCriterion,
                                     llama_pipeline_descs, shard_llama_state_dict)


def _cfg(**kw):
    c = dict(LLAMA_CONFIGS["llama-tiny"])
    c.update(kw)
    return LlamaConfig(**c, dtype="float32")


def _batch(B=4, S=17, V=512, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (B, S), generator=g)


def test_topology_axes():
    t = CommunicateTopology(dict(dp=2, pp=2, mp=2))
    assert t.world_size == 8
    assert t.coord(5) == dict(dp=1, pp=0, sharding=0, sep=0, mp=1)
    assert t.axis_groups("mp")[0] == [0, 1]
    assert t.axis_groups("pp")[0] == [0, 2]
    assert t.axis_groups("dp")[0] == [0, 4]


# ----------------------------------------------------------------- tensor parallel
def _tp_worker(rank, world):
    from paddle_amd.distributed.fleet import TPGroup

    cfg = _cfg()
    torch.manual_seed(0)
    full = LlamaForCausalLM(cfg, "cpu")
    b = _batch()
    loss_ref = full(b[:, :-1], b[:, 1:])
    loss_ref.backward()
    # gradients in the canonical (state-dict) layout: gate_up de-interleaved like weights
    grads_ref = {n: (torch.cat(ops.deinterleave_gate_up(p.grad), -1)
                     if n.endswith("gate_up_proj") and full.layers[0].mlp_interleaved else p.grad)
                 for n, p in full.named_parameters()}
    tp = TPGroup(None)
    m = LlamaForCausalLM(cfg, "cpu", tp=tp)
    sd = shard_llama_state_dict({k: v.detach() for k, v in full.state_dict().items()}, cfg, rank, world)
    m.load_state_dict(sd)
    loss = m(b[:, :-1], b[:, 1:])
    loss.backward()
    gshard = shard_llama_state_dict(grads_ref, cfg, rank, world)
    errs = {n: (p.grad - gshard[n]).abs().max().item() for n, p in m.named_parameters()}
    return loss.item(), loss_ref.item(), max(errs.values())


def test_tensor_parallel_llama_matches_single():
    res = run_dist(_tp_worker, 2)
    for loss, ref, gerr in res:
        assert abs(loss - ref) < 1e-5
        assert gerr < 1e-5


# --------------------------------------------------------------- pipeline parallel
def _pp_ref(M, steps):
    from paddle_amd.distributed.fleet.pipeline import PipelineLayer

    cfg = _cfg(num_hidden_layers=4)
    crit = LlamaPretrainingCriterion()
    model = PipelineLayer(llama_pipeline_descs(cfg, "cpu"), num_stages=1, loss_fn=crit, seed=11)
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    losses = []
    for s in range(steps):
        b = _batch(B=8, seed=s)
        tot = 0.0
        for mb in b.chunk(M):
            loss = crit(model(mb[:, :-1]), mb[:, 1:]) / M
            loss.backward()
            tot += loss.item()
        opt.step()
        opt.zero_grad()
        losses.append(tot)
    return losses, model


def _pp_worker(rank, world, M, steps):
    from paddle_amd.distributed.fleet import DistributedStrategy, fleet
    from paddle_amd.distributed.fleet.pipeline import PipelineLayer

    st = DistributedStrategy()
    st.hybrid_configs = {"dp_degree": 1, "pp_degree": world}
    st.pipeline_configs = {"accumulate_steps": M}
    fleet.init(is_collective=True, strategy=st)
    hcg = fleet.get_hybrid_communicate_group()
    cfg = _cfg(num_hidden_layers=4)
    layer = PipelineLayer(llama_pipeline_descs(cfg, "cpu"), hcg=hcg, loss_fn=LlamaPretrainingCriterion(), seed=11)
    model = fleet.distributed_model(layer)
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    losses = []
    rounds = []
    for s in range(steps):
        b = _batch(B=8, seed=s)
        losses.append(model.train_batch((b[:, :-1], b[:, 1:]), opt).item())
        p2p = model._p2p_train
        rounds.append((p2p.meta_rounds, p2p.host_syncs))
    lo = layer.bounds[hcg.get_stage_id()]
    params = {f"run_function.{lo + int(n.split('.')[1])}.{'.'.join(n.split('.')[2:])}": p.detach().clone()
              for n, p in layer.named_parameters()}
    return losses, params, rounds


@pytest.mark.parametrize("world,M", [(2, 4), (4, 8)])
def test_pipeline_1f1b_llama_matches_single(world, M):
    steps = 2
    ref_losses, ref_model = _pp_ref(M, steps)
    ref = dict(ref_model.named_parameters())
    res = run_dist(_pp_worker, world, M, steps)
    for losses, params, rounds in res:
        # metadata travels only in the first step; steady state: one batched round per
        # exchange and no device->host reads
        assert rounds[-1][0] == rounds[0][0] and rounds[0][0] <= 4, rounds
        assert rounds[-1][1] == 0, rounds
        for a, b in zip(losses, ref_losses):
            assert abs(a - b) < 1e-5, (losses, ref_losses)
        for n, p in params.items():
            assert torch.allclose(p, ref[n].detach(), atol=1e-5), n


# ------------------------------------------------------------------ expert parallel
def _experts(n, d, seed):
    out = []
    for e in range(n):
        torch.manual_seed(seed + e)
        out.append(torch.nn.Sequential(torch.nn.Linear(d, 2 * d), torch.nn.GELU(), torch.nn.Linear(2 * d, d)))
    return out


def _moe_worker(rank, world, cap, sync_free=True):
    from paddle_amd.distributed.fleet import MoELayer, TopKGate

    d, E, T = 16, 4, 24
    torch.manual_seed(100)
    gate_w = torch.randn(d, E) * 0.5
    xs = [torch.randn(T, d, generator=torch.Generator().manual_seed(50 + r)) for r in range(world)]
    # reference: all experts, all tokens, one process
    ref_gate = TopKGate(d, E, top_k=2, capacity_factor=cap)
    ref_gate.weight.data.copy_(gate_w)
    ref = MoELayer(d, _experts(E, d, 7), gate=ref_gate, group=None, capacity_factor=cap)
    if cap is None:
        xr = torch.cat(xs).requires_grad_()
        yr = ref(xr)
        yr.pow(2).sum().backward()
        y_ref, g_ref = yr.detach()[rank * T:(rank + 1) * T], xr.grad[rank * T:(rank + 1) * T]
    else:  # capacity is per source rank: reference runs each rank's tokens separately
        xr = xs[rank].clone().requires_grad_()
        y_ref, g_ref = None, None
    n_local = E // world
    gate = TopKGate(d, E, top_k=2, capacity_factor=cap)
    gate.weight.data.copy_(gate_w)
    allex = _experts(E, d, 7)
    moe = MoELayer(d, allex[rank * n_local:(rank + 1) * n_local], gate=gate, group=None if world == 1 else
                   torch.distributed.group.WORLD, capacity_factor=cap, sync_free=sync_free)
    x = xs[rank].clone().requires_grad_()
    y = moe(x)
    y.pow(2).sum().backward()
    if y_ref is None:
        return y.detach(), x.grad.detach(), [p.grad.detach().clone() for p in moe.parameters()]
    return (y.detach() - y_ref).abs().max().item(), (x.grad - g_ref).abs().max().item()


def test_moe_expert_parallel_matches_single():
    for yerr, gerr in run_dist(_moe_worker, 2, None):
        assert yerr < 1e-5 and gerr < 1e-5


def _moe_cap_pair(rank, world, cap):
    a = _moe_worker(rank, world, cap, sync_free=True)
    b = _moe_worker(rank, world, cap, sync_free=False)
    return ((a[0] - b[0]).abs().max().item(), (a[1] - b[1]).abs().max().item(),
            max((ga - gb).abs().max().item() for ga, gb in zip(a[2], b[2])), int((a[0] == 0).all(1).sum()))


def test_moe_capacity_drop_runs():
    run_dist(_moe_worker, 2, 0.5)


def test_moe_capacity_sync_free_matches_exact_split():
    """The fixed-capacity, equal-split exchange (no host sync) drops the same slots
    and gives the same outputs and input / expert / gate gradients as the exact-split
    exchange with the same capacity (reference seed: GShard capacity semantics)."""
    for cap in (0.5, 1.0):
        for yerr, xerr, perr, _ in run_dist(_moe_cap_pair, 2, cap):
            assert yerr < 1e-5 and xerr < 1e-5 and perr < 1e-5, (cap, yerr, xerr, perr)


# -------------------------------------------------------------- sharding stage 3
def _stage3_run(rank, world, steps):
    from paddle_amd.distributed import group_sharded_parallel

    cfg = _cfg()
    torch.manual_seed(0)
    m = LlamaForCausalLM(cfg, "cpu")
    m, opt = group_sharded_parallel(m, level="p_g_os", lr=1e-2, weight_decay=0.1, grad_clip=1.0)
    losses = []
    for s in range(steps):
        b = _batch(B=4, seed=s)
        part = b.chunk(world)[rank]
        loss = m(part[:, :-1], part[:, 1:])
        loss.backward()
        opt.step()
        opt.zero_grad()
        t = torch.tensor([loss.item()])
        if world > 1:
            torch.distributed.all_reduce(t)
        losses.append(t.item() / world)
    sd = opt.full_state_dict()
    return losses, {k: v for k, v in sd.items() if not k.startswith("rope")}


def test_sharding_stage3_matches_single():
    ref_losses, ref_sd = _stage3_run(0, 1, 3)
    res = run_dist(_stage3_run, 2, 3)
    for losses, sd in res:
        for a, b in zip(losses, ref_losses):
            assert abs(a - b) < 1e-4, (losses, ref_losses)
        for k in ref_sd:
            # (Adam normalises near-zero gradients: fp32 summation order shows at ~1e-4 of lr)
            assert_adam_close(sd[k], ref_sd[k], atol=3e-4, rtol=1e-3, lr=1e-2, steps=3, name=k)


# ---------------------------------------------------------------- context parallel
def _cp_worker(rank, world, kind):
    from paddle_amd.distributed.fleet import allgather_kv_attention, ulysses_attention
    from paddle_amd.ops.fused import _attn_ref

    B, S, H, D = 2, 16, 4, 8
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, S, H, D, generator=g) for _ in range(3))
    qf, kf, vf = (t.clone().requires_grad_() for t in (q, k, v))
    o = _attn_ref(qf, kf, vf, True, 0.3)
    o.pow(2).sum().backward()
    s = S // world
    sl = slice(rank * s, (rank + 1) * s)
    ql, kl, vl = (t[:, sl].clone().requires_grad_() for t in (q, k, v))
    fn = ulysses_attention if kind == "ulysses" else allgather_kv_attention
    ol = fn(ql, kl, vl, torch.distributed.group.WORLD, causal=True, scale=0.3)
    ol.pow(2).sum().backward()
    errs = [(ol.detach() - o.detach()[:, sl]).abs().max().item()]
    for a, b in ((ql, qf), (kl, kf), (vl, vf)):
        errs.append((a.grad - b.grad[:, sl]).abs().max().item())
    return max(errs)


@pytest.mark.parametrize("kind", ["ulysses", "allgather_kv"])
def test_context_parallel_attention_matches_full(kind):
    for err in run_dist(_cp_worker, 2, kind):
        assert err < 1e-5


def _ring_worker(rank, world, hk):
    from paddle_amd.distributed.fleet import ring_attention, zigzag_split
    from paddle_amd.ops.fused import _attn_ref

    B, S, H, D = 2, 8 * world, 4, 8
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, S, H, D, generator=g)
    k, v = (torch.randn(B, S, hk, D, generator=g) for _ in range(2))
    qf, kf, vf = (t.clone().requires_grad_() for t in (q, k, v))
    o = _attn_ref(qf, kf, vf, True, 0.35)
    w = torch.randn(o.shape, generator=g)
    (o * w).sum().backward()
    ql, kl, vl = (zigzag_split(t, rank, world).clone().requires_grad_() for t in (q, k, v))
    ol = ring_attention(ql, kl, vl, torch.distributed.group.WORLD, causal=True, scale=0.35)
    (ol * zigzag_split(w, rank, world)).sum().backward()
    errs = [(ol.detach() - zigzag_split(o.detach(), rank, world)).abs().max().item()]
    for a, b in ((ql, qf), (kl, kf), (vl, vf)):
        errs.append((a.grad - zigzag_split(b.grad, rank, world)).abs().max().item())
    return max(errs)


@pytest.mark.parametrize("world,hk", [(2, 4), (4, 4), (4, 2)])
def test_ring_attention_zigzag_matches_full(world, hk):
    """Zigzag ring attention (P2P K/V ring, LSE merge, global-LSE backward with dK/dV
    riding the ring home) equals full causal attention, incl. GQA."""
    for err in run_dist(_ring_worker, world, hk):
        assert err < 1e-5


def test_zigzag_split_merge_roundtrip():
    from paddle_amd.distributed.fleet import zigzag_merge, zigzag_split

    x = torch.arange(2 * 24).reshape(2, 24)
    for P in (1, 2, 3, 4):
        shards = [zigzag_split(x, r, P) for r in range(P)]
        assert torch.equal(zigzag_merge(shards), x)
        # balanced causal work: chunk pairs (r, 2P-1-r) sum to the same index
        assert len({(r + 2 * P - 1 - r) for r in range(P)}) == 1


# ------------------------------------------------------- DataParallel + fleet dp x mp
def _dp_mp_worker(rank, world, steps):
    from paddle_amd.distributed.fleet import DistributedStrategy, TPGroup, fleet

    st = DistributedStrategy()
    st.hybrid_configs = {"dp_degree": 2, "mp_degree": 2}
    fleet.init(is_collective=True, strategy=st)
    hcg = fleet.get_hybrid_communicate_group()
    cfg = _cfg()
    torch.manual_seed(0)
    full = LlamaForCausalLM(cfg, "cpu")
    sd_full = {k: v.detach() for k, v in full.state_dict().items()}
    tp = TPGroup(hcg.get_model_parallel_group())
    m = LlamaForCausalLM(cfg, "cpu", tp=tp)
    m.load_state_dict(shard_llama_state_dict(sd_full, cfg, hcg.get_model_parallel_rank(), 2))
    model = fleet.distributed_model(m)
    inner = torch.optim.SGD(m.parameters(), lr=0.5)
    inner.grad_clip = 1.0
    opt = fleet.distributed_optimizer(inner)
    for s in range(steps):
        b = _batch(B=4, seed=s).chunk(2)[hcg.get_data_parallel_rank()]
        loss = model(b[:, :-1], b[:, 1:])
        loss.backward()
        opt.step()
        opt.clear_grad()
    # the dp all-reduce buckets were issued from grad-ready hooks during backward
    assert opt._bucket_sync is not None and opt._bucket_sync.launch_count > 0
    return hcg.get_model_parallel_rank(), {k: v.detach().clone() for k, v in m.state_dict().items()}


def _dp_mp_ref(steps):
    cfg = _cfg()
    torch.manual_seed(0)
    full = LlamaForCausalLM(cfg, "cpu")
    opt = torch.optim.SGD(full.parameters(), lr=0.5)
    for s in range(steps):
        b = _batch(B=4, seed=s)
        loss = full(b[:, :-1], b[:, 1:])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(full.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
    return cfg, {k: v.detach() for k, v in full.state_dict().items()}


def test_fleet_dp2_mp2_llama_matches_single():
    steps = 2
    cfg, ref = _dp_mp_ref(steps)
    for mp_rank, sd in run_dist(_dp_mp_worker, 4, steps):
        want = shard_llama_state_dict(ref, cfg, mp_rank, 2)
        for k in want:
            assert torch.allclose(sd[k], want[k], atol=2e-5, rtol=1e-4), k


def _ddp_worker(rank, world):
    from paddle_amd.distributed import DataParallel

    torch.manual_seed(rank)  # different init: DataParallel must broadcast rank 0's
    net = torch.nn.Sequential(torch.nn.Linear(8, 32), torch.nn.Tanh(), torch.nn.Linear(32, 4))
    dp = DataParallel(net, bucket_mb=0.0005)
    assert len(dp.buckets) > 1
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))
    for _ in range(3):
        dp(x.chunk(world)[rank]).pow(2).mean().backward()
        opt.step()
        opt.zero_grad()
    return [p.detach().clone() for p in net.parameters()]


def test_data_parallel_buckets_match_single():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(8, 32), torch.nn.Tanh(), torch.nn.Linear(32, 4))
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))
    for _ in range(3):
        # mean over ranks of per-rank means == full-batch mean for equal chunks
        net(x).pow(2).mean().backward()
        opt.step()
        opt.zero_grad()
    res = run_dist(_ddp_worker, 2)
    for ps in res:
        for a, b in zip(ps, net.parameters()):
            assert torch.allclose(a, b.detach(), atol=1e-6)


def test_launcher_runs_two_ranks(tmp_path):
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "w.py"
    script.write_text(
        "import os, torch, torch.distributed as dist\n"
        "dist.init_process_group('gloo')\n"
        "t = torch.tensor([dist.get_rank() + 1.0]); dist.all_reduce(t)\n"
        "open(os.path.join(os.path.dirname(__file__), 'out%s' % os.environ['PADDLE_TRAINER_ID']), 'w')"
        ".write(str(t.item()))\n")
    from dist_util import _free_port

    rc = subprocess.call([sys.executable, "-m", "paddle_amd.distributed.launch", "--nproc_per_node", "2",
                          "--master_port", str(_free_port()), str(script)],
                         cwd=root, timeout=120)
    assert rc == 0
    assert (tmp_path / "out0").read_text() == "3.0" and (tmp_path / "out1").read_text() == "3.0"


# ------------------------------------------------------- dp2 x pp2 (1F1B) with hook-fired dp buckets
def _dp_pp_worker(rank, world, M, steps):
    from paddle_amd.distributed.fleet import DistributedStrategy, fleet
    from paddle_amd.distributed.fleet.pipeline import PipelineLayer

    st = DistributedStrategy()
    st.hybrid_configs = {"dp_degree": 2, "pp_degree": 2}
    st.pipeline_configs = {"accumulate_steps": M}
    fleet.init(is_collective=True, strategy=st)
    hcg = fleet.get_hybrid_communicate_group()
    cfg = _cfg(num_hidden_layers=4)
    layer = PipelineLayer(llama_pipeline_descs(cfg, "cpu"), hcg=hcg, loss_fn=LlamaPretrainingCriterion(), seed=11)
    model = fleet.distributed_model(layer)
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    losses = []
    for s in range(steps):
        b = _batch(B=8, seed=s).chunk(2)[hcg.get_data_parallel_rank()]
        losses.append(model.train_batch((b[:, :-1], b[:, 1:]), opt).item())
    gs = model._grad_sync
    lo = layer.bounds[hcg.get_stage_id()]
    params = {f"run_function.{lo + int(n.split('.')[1])}.{'.'.join(n.split('.')[2:])}": p.detach().clone()
              for n, p in layer.named_parameters()}
    return losses, params, gs.launch_count


def test_pipeline_dp2_pp2_matches_single():
    M, steps = 2, 2
    _, ref_model = _pp_ref(M * 2, steps)
    ref = dict(ref_model.named_parameters())
    for losses, params, launched in run_dist(_dp_pp_worker, 4, M, steps):
        assert launched > 0  # buckets issued during the last micro-batch's reverse pass
        for n, p in params.items():
            assert torch.allclose(p, ref[n].detach(), atol=2e-5), n


# ------------------------------------------------------- dp x mp bucket sync: accumulation and AMP
def _dp_mp_sync_worker(rank, world, steps, mode):
    import paddle_amd
    from paddle_amd.distributed.fleet import DistributedStrategy, TPGroup, fleet

    st = DistributedStrategy()
    st.hybrid_configs = {"dp_degree": 2, "mp_degree": 2}
    fleet.init(is_collective=True, strategy=st)
    hcg = fleet.get_hybrid_communicate_group()
    cfg = _cfg()
    torch.manual_seed(0)
    full = LlamaForCausalLM(cfg, "cpu")
    sd_full = {k: v.detach() for k, v in full.state_dict().items()}
    tp = TPGroup(hcg.get_model_parallel_group())
    m = LlamaForCausalLM(cfg, "cpu", tp=tp)
    m.load_state_dict(shard_llama_state_dict(sd_full, cfg, hcg.get_model_parallel_rank(), 2))
    model = fleet.distributed_model(m)
    opt = fleet.distributed_optimizer(paddle_amd.optimizer.SGD(learning_rate=0.5, parameters=m.parameters()))
    scaler = paddle_amd.amp.GradScaler(init_loss_scaling=1024.0) if mode == "amp" else None
    dpr = hcg.get_data_parallel_rank()
    for s in range(steps):
        b = _batch(B=4, seed=s).chunk(2)[dpr]
        if mode == "accum":
            # two reverse passes before one step: the buckets launched by the first
            # must not be written back over the accumulated gradients
            for half in b.chunk(2):
                (model(half[:, :-1], half[:, 1:]) / 2).backward()
            opt.step()
        else:
            loss = model(b[:, :-1], b[:, 1:])
            if s == 0 and dpr == 0:
                loss = loss * float("inf")  # overflow on ONE data-parallel replica only
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        opt.clear_grad()
    gs = opt._bucket_sync
    return hcg.get_model_parallel_rank(), {k: v.detach().clone() for k, v in m.state_dict().items()}, \
        gs.launch_count, gs.redo_count


def _dp_mp_sync_ref(steps, skip_first):
    cfg = _cfg()
    torch.manual_seed(0)
    full = LlamaForCausalLM(cfg, "cpu")
    opt = torch.optim.SGD(full.parameters(), lr=0.5)
    for s in range(steps):
        if skip_first and s == 0:
            continue
        b = _batch(B=4, seed=s)
        full(b[:, :-1], b[:, 1:]).backward()
        opt.step()
        opt.zero_grad()
    return cfg, {k: v.detach() for k, v in full.state_dict().items()}


@pytest.mark.parametrize("mode", ["accum", "amp"])
def test_fleet_dp_bucket_sync_accumulation_and_amp(mode):
    steps = 2
    cfg, ref = _dp_mp_sync_ref(steps, skip_first=(mode == "amp"))
    for mp_rank, sd, launched, redo in run_dist(_dp_mp_sync_worker, 4, steps, mode):
        assert launched > 0
        want = shard_llama_state_dict(ref, cfg, mp_rank, 2)
        for k in want:
            assert torch.allclose(sd[k], want[k], atol=2e-5, rtol=1e-4), (mode, k)
