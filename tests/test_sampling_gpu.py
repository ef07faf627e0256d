"""The sampling kernel (csrc/kernels/sample.hip) against the float64 reference of
ops/sampling.py: the Philox bits, greedy ties, every draw of 64 steps x B rows inside the
reference's survivor set and running-sum interval, run-to-run bits, row independence,
degenerate rows and the ``sample_step`` bookkeeping.

Tolerance of the interval check: the kernel sums at most 2^17 fp32 masses in a tree, which
errs by about 17 * 2^-24 ~ 1e-6 of the total; ``TOL`` is ten times that.  The inputs are
chosen (and asserted below, on the CPU side) so that the top-p decision of every row is more
than 1e-4 of the mass away from flipping and at most 1 % of the draws fall within ``TOL`` of
an interval end; those draws are checked like the others, with the widened interval."""
import itertools

import pytest
import torch

from paddle_amd import ops
from paddle_amd.ops import sampling as S

pytestmark = pytest.mark.gpu

dev = "cuda"
TOL = 1e-5
SEED = 0x1234567855B6
STEPS = 64
ROWS = 16
VOCABS = [1, 7, 1003, 50257, 131072]
BATCHES = [1, 3, 16]
DTYPES = [torch.bfloat16, torch.float32]
# every sampling configuration of the interval check; the temperature of the unfiltered one
# sharpens the distribution so that few draws land within TOL of one of up to 2^17 interval ends
CONFIGS = [dict(temperature=0.5, top_k=0, top_p=1.0), dict(temperature=0.8, top_k=50, top_p=0.9),
           dict(temperature=0.5, top_k=0, top_p=0.7), dict(temperature=1.0, top_k=4, top_p=1.0)]
PAD = 3  # extra row stride: rows start at every 16-byte misalignment
MARGIN = 1e-4  # least distance of a row's top-p decision from flipping, as a fraction of the mass


def _margin_ok(row):
    return all(S.reference_top_p_margin(row, **cfg) > 2 * MARGIN for cfg in CONFIGS if cfg["top_p"] < 1.0)


def make_logits(V, dtype):
    """[ROWS, V] fp32 values: seeded randn * 3 rounded to bf16 (ties occur naturally at large V;
    for fp32 the rows from 8 on keep their fp32 bits); a candidate row whose top-p decision is
    within 2 * MARGIN of flipping is drawn again.  Rows 0-2 carry planted ties (V >= 7): row 0
    at the maximum, row 1 at the 4th largest value (top_k = 4), row 2 two equal logits that
    straddle top_p = 0.7 in sorted order over a far background."""
    g = torch.Generator().manual_seed(1000 + V)
    a, b, c = V // 3, V // 2, V - 1
    rows = []
    while len(rows) < ROWS:
        i = len(rows)
        x = torch.randn(V, generator=g) * 3
        r = x if (dtype == torch.float32 and i >= 8) else x.bfloat16().float()
        if V >= 7 and i == 0:
            r[b] = r[c] = 16.0
        if V >= 7 and i == 1:
            r[[a, b, c]] = r.topk(4).values[-1]
        if V >= 7 and i == 2:
            r.fill_(-20.0)
            r[a] = 4.0
            r[b] = r[c] = 3.5
        if _margin_ok(r):
            rows.append(r)
    return torch.stack(rows)


_ref = {}


def reference(V, dtype):
    """(logits, per configuration the reference distribution of every row), cached for the
    vocabulary in use (the cases run ordered by V)."""
    key = (V, dtype)
    if key not in _ref:
        for k in [k for k in _ref if k[0] != V]:
            del _ref[k]
        x = make_logits(V, dtype)
        dists = []
        for cfg in CONFIGS:
            per_row = [S.reference_distribution(x[b], **cfg) for b in range(ROWS)]
            assert all(d is not None for d in per_row)
            if cfg["top_p"] < 1.0:
                worst = min(S.reference_top_p_margin(x[b], **cfg) for b in range(ROWS))
                assert worst > MARGIN, f"V={V} {cfg}: top-p margin {worst:.2e}: choose another seed"
            dists.append(per_row)
        _ref[key] = (x, dists)
    return _ref[key]


def uniforms(B):
    return torch.tensor([[S.philox_u(SEED, s, b) for b in range(B)] for s in range(STEPS)], dtype=torch.float64)


def near_boundary_fraction(dists, B):
    """Fraction of the STEPS x B draws that lie within TOL of an end of some token's interval."""
    u = uniforms(B)
    near = 0
    for b in range(B):
        c = dists[b][1]
        ends = torch.cat([torch.zeros(1, dtype=c.dtype), c])
        i = torch.searchsorted(ends, u[:, b]).clamp(1, ends.numel() - 1)
        d = torch.minimum((u[:, b] - ends[i - 1]).abs(), (ends[i] - u[:, b]).abs())
        near += int((d <= TOL).sum())
    return near / (STEPS * B)


def on_device(x, dtype, pad=PAD):
    """x [B, V] as device logits of ``dtype`` with a row stride of V + pad."""
    B, V = x.shape
    buf = torch.full((B, V + pad), float("nan"), dtype=dtype, device=dev)
    buf[:, :V] = x.to(dev, dtype)
    return buf[:, :V]


class count_launches:
    def __enter__(self):
        self.n = 0
        self._orig = S._launch

        def wrapped(*a, **k):
            self.n += 1
            return self._orig(*a, **k)

        S._launch = wrapped
        return self

    def __exit__(self, *exc):
        S._launch = self._orig


def test_philox_bits_equal_the_cpu():
    for seed, step, B in [(0, 0, 1), (SEED, 5, 16), (2 ** 63 + 11, 2 ** 31 - 1, 300), (2 ** 32, 1, 3)]:
        want = ops.philox_uniform(seed, step, B, "cpu")
        assert torch.equal(ops.philox_uniform(seed, step, B, dev).cpu(), want)
        st = torch.tensor([step], dtype=torch.int32, device=dev)
        assert torch.equal(ops.philox_uniform(seed, st, B, dev).cpu(), want)


CASES = [(V, dt, B) for V, dt, B in itertools.product(VOCABS, DTYPES, BATCHES)]


@pytest.mark.parametrize("V,dtype,B", CASES, ids=[f"V{V}-{str(dt)[6:]}-B{B}" for V, dt, B in CASES])
def test_tokens_against_the_reference(V, dtype, B):
    x, dists = reference(V, dtype)
    logits = on_device(x[:B], dtype)
    assert logits.stride(0) == V + PAD and S.sample_kernel_ok(logits)
    with count_launches() as c:
        greedy = ops.sample_tokens(logits)
        runs = [[torch.stack([ops.sample_tokens(logits, seed=SEED, step=s, do_sample=True, **cfg)
                              for s in range(STEPS)]) for cfg in CONFIGS] for _ in range(2)]
    assert c.n == 1 + 2 * STEPS * len(CONFIGS)  # the kernel ran, every time
    assert greedy.dtype == torch.int64
    assert greedy.tolist() == [S.reference_greedy(x[b]) for b in range(B)]
    u = uniforms(B)
    for ci, cfg in enumerate(CONFIGS):
        assert torch.equal(runs[0][ci], runs[1][ci]), f"{cfg}: two runs differ"
        frac = near_boundary_fraction(dists[ci], B)
        assert frac <= 0.01, f"{cfg}: {frac:.3f} of the draws are within TOL of an interval end"
        toks = runs[0][ci].cpu()  # [STEPS, B]
        assert ((toks >= 0) & (toks < V)).all()
        for b in range(B):
            keep, c_ = dists[ci][b]
            t = toks[:, b]
            assert keep[t].all(), f"{cfg} row {b}: a token outside the survivor set"
            lo = torch.where(t > 0, c_[(t - 1).clamp(min=0)], torch.zeros_like(u[:, b]))
            bad = ~((lo - TOL <= u[:, b]) & (u[:, b] < c_[t] + TOL))
            assert not bad.any(), (f"{cfg} row {b}: steps {bad.nonzero().flatten().tolist()} drew tokens "
                                   f"{t[bad].tolist()} for u {u[bad, b].tolist()}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_contiguous_rows_and_a_broadcast_row(dtype):
    x, dists = reference(1003, dtype)
    cfg = CONFIGS[1]
    padded = ops.sample_tokens(on_device(x[:3], dtype), seed=SEED, step=7, do_sample=True, **cfg)
    assert torch.equal(ops.sample_tokens(on_device(x[:3], dtype, 0), seed=SEED, step=7, do_sample=True, **cfg), padded)
    # one row seen three times (row stride 0): rows differ only by their random number
    same = x[:1].to(dev, dtype).expand(3, -1)
    toks = ops.sample_tokens(same, seed=SEED, step=7, do_sample=True, **cfg).tolist()
    for b, t in enumerate(toks):
        keep, c = dists[1][0]
        ub = S.philox_u(SEED, 7, b)
        assert keep[t] and (c[t - 1] if t else 0.0) - TOL <= ub < c[t] + TOL


def test_row_independence():
    x, _ = reference(1003, torch.bfloat16)
    a = on_device(x, torch.bfloat16)
    other = x.flip(0).clone()
    other[5] = x[5]
    b = on_device(other, torch.bfloat16)
    for cfg in CONFIGS:
        for step in range(8):
            ta = ops.sample_tokens(a, seed=SEED, step=step, do_sample=True, **cfg)
            tb = ops.sample_tokens(b, seed=SEED, step=step, do_sample=True, **cfg)
            assert ta[5] == tb[5]


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_rows_stay_in_range(dtype):
    V = 1003
    ninf, nan, inf = float("-inf"), float("nan"), float("inf")
    rows = torch.zeros(7, V)
    rows[0].fill_(ninf)
    rows[1].fill_(nan)
    rows[2] = torch.arange(V).float() / 64
    rows[2, 1002] = nan  # a NaN counts as -inf
    rows[3].fill_(ninf)
    rows[3, 777] = 1.0
    rows[4, 11] = inf
    rows[5, ::2] = nan
    rows[5, 1::4] = ninf
    rows[6].fill_(-3.0e38)  # exp underflows for all but the maximum
    rows[6, 500] = 3.0e38
    x = on_device(rows, dtype)
    for kw in (dict(), dict(do_sample=True), dict(do_sample=True, top_k=4, top_p=0.5, temperature=1e-9),
               dict(do_sample=True, top_p=0.0), dict(do_sample=True, temperature=1e9)):
        for step in range(4):
            t = ops.sample_tokens(x, seed=3, step=step, **kw)
            assert t.dtype == torch.int64 and ((t >= 0) & (t < V)).all(), (kw, t.tolist())
            t = t.tolist()
            assert t[0] == 0 and t[1] == 0 and t[3] == 777 and t[4] == 11, (kw, t)
            assert t[2] != 1002 and t[5] % 2 == 1 and t[5] % 4 != 1, (kw, t)
            if kw.get("temperature", 1.0) <= 1.0:
                assert t[6] == 500, (kw, t)


@pytest.mark.parametrize("how", [dict(), dict(do_sample=True, top_k=1, seed=4)])
def test_sample_step_equals_the_cpu_state_sequence(how):
    B, V, T, eos, pad = 3, 1003, 7, 4, 9
    g = torch.Generator().manual_seed(0)
    script = (torch.randn(T + 1, B, V, generator=g) * 3).bfloat16()
    script[:, :, eos] = -50.0
    script[2, 1, eos] = 50.0  # row 1 hits EOS at step 2 ...
    script[4, 1, eos] = 50.0  # ... and is done already here
    script[T - 1, 0, eos] = 50.0  # row 0 at the last step
    cpu = ops.SamplerState(B, T, "cpu", eos_token_id=eos, pad_token_id=pad)
    gpu = ops.SamplerState(B, T, dev, eos_token_id=eos, pad_token_id=pad)
    assert gpu.tok.is_cuda and gpu.step.dtype == torch.int32
    with count_launches() as c:
        for step in range(T + 1):  # one step past the end: no column is written, nothing else moves
            ops.sample_step(script[step].float(), cpu, **how)
            tok = ops.sample_step(on_device(script[step].float(), torch.bfloat16), gpu, **how)
            assert tok is gpu.tok
            for name in ("tok", "out", "lengths", "done", "step"):
                assert torch.equal(getattr(gpu, name).cpu(), getattr(cpu, name)), f"step {step}: {name}"
    assert c.n == T + 1
    assert cpu.lengths.tolist() == [T, 3, T] and cpu.out[1].tolist()[2:] == [eos] + [pad] * (T - 3)
