"""Token selection for generation: logits [B, V] -> the next token per row.

``sample_tokens`` / ``sample_step`` run ``csrc/kernels/sample.hip`` on GPU logits (bf16 or
fp32, unit column stride, ``1 <= V <= 131072``); CPU tensors and everything else run the
float64 definitions below, which are the specification and the oracle of the GPU tests.
Inference ops: nothing is recorded on the tape.

Contract (per row; NaN counts as ``-inf``, ``-0`` as ``+0``):

* greedy: the lowest index among the maxima;
* the random number of (seed, step, row) is Philox4x32-10 with key
  ``(seed & 0xffffffff, seed >> 32)`` and counter ``(step, row, 0, 0)``:
  ``u = (x0 >> 8) * 2**-24``, the same bits on the GPU and here.  A row's draw depends on
  (seed, step, row index, the row's logits) and on nothing else in the batch;
* top-k keeps ``{i : logit_i >= k-th largest logit}`` (ties at the k-th value all stay);
  ``0 < top_k < V``, else no filter;
* ``z = logit / max(temperature, 1e-6)``, ``p = softmax(z)`` over the kept set;
* top-p (``< 1``) keeps ``i`` iff the mass of the kept tokens with a strictly greater logit
  is ``< top_p``: equal logits stay or go together, the maximum always stays;
* ``q`` is ``p`` over the survivors, renormalised, ``c`` its running sum in vocabulary-index
  order; the token is the first ``i`` with ``u < c_i`` (the last survivor when rounding
  leaves none);
* the token is in ``[0, V)`` for any input: where sampling has nothing to draw from (the
  maximum is not finite, or the masses do not sum to a positive finite number) the greedy
  rule applies.

``sample_step`` adds the bookkeeping of ``generate()``'s loop on a :class:`SamplerState`, with
no host read: a done row emits ``pad``; ``out[:, step] = tok``; a first EOS sets
``lengths = step + 1`` and ``done``; then ``step += 1`` in a launch of its own, ordered after
every row's read of it.
"""
from __future__ import annotations

import math

import torch

from . import _native as N

__all__ = ["philox_uniform", "sample_tokens", "sample_step", "SamplerState", "sample_kernel_ok",
           "reference_distribution", "reference_pick", "reference_greedy", "reference_top_p_margin"]

MAX_VOCAB = 131072
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------- Philox4x32-10
def philox_x0(seed: int, c0: int, c1: int) -> int:
    """First output word of Philox4x32-10 for key (seed lo, seed hi), counter (c0, c1, 0, 0)."""
    seed = int(seed) & _M64
    k0, k1 = seed & _M32, seed >> 32
    x0, x1, x2, x3 = int(c0) & _M32, int(c1) & _M32, 0, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ k0, p1 & _M32, (p0 >> 32) ^ x3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return x0


def philox_u(seed: int, step: int, row: int) -> float:
    """The uniform of (seed, step, row): a multiple of 2**-24 in [0, 1), exact in fp32."""
    return (philox_x0(seed, step, row) >> 8) * 2.0 ** -24


def _step_args(step):
    """(device pointer or None, host value) of a step given as an int or an int32 device tensor [1]."""
    if torch.is_tensor(step):
        if step.is_cuda:
            if step.dtype != torch.int32 or step.numel() != 1:
                raise ValueError("step must be an int or an int32 tensor [1]")
            return N.ptr(step), 0
        return None, int(step)
    return None, int(step)


def philox_uniform(seed, step, B, device=None):
    """u [B] fp32 in [0, 1): row b's random number for (seed, step).  ``step`` is an int or an
    int32 device tensor [1] (read on the stream, no host read)."""
    device = torch.device(device if device is not None else "cpu")
    B = int(B)
    if B < 1:
        raise ValueError("philox_uniform: B must be at least 1")
    if device.type == "cuda":
        sp, sv = _step_args(step)
        u = torch.empty(B, dtype=torch.float32, device=device)
        N.call("pa_philox_uniform", int(seed) & _M64, sp, sv, N.ptr(u), B, N.stream())
        return u
    s = int(step)
    return torch.tensor([philox_u(seed, s, b) for b in range(B)], dtype=torch.float32, device=device)


# ---------------------------------------------------------------------- float64 reference
def _clean(row):
    x = row.detach().to("cpu", torch.float64).reshape(-1)
    return torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)


def reference_greedy(row) -> int:
    """The lowest index among the maxima of one row of logits."""
    x = _clean(row)
    return int((x == x.max()).nonzero()[0, 0])


def _kept_masses(x, temperature, top_k):
    """Unnormalised softmax masses of a cleaned row after top-k (0 where dropped)."""
    V = x.numel()
    keep = torch.ones(V, dtype=torch.bool)
    if top_k and 0 < int(top_k) < V:
        keep &= x >= x.topk(int(top_k)).values[-1]
    z = (x - x.max()) / max(float(temperature), 1e-6)
    return keep, torch.where(keep, torch.exp(z), torch.zeros_like(z))


def _mass_above(x, e):
    """(order, xs, greater): the row sorted downwards and, per sorted entry, the mass of the
    strictly greater logits (equal logits share one value)."""
    xs, order = x.sort(descending=True)
    es = e[order]
    before = es.cumsum(0) - es  # mass ahead in sorted order, equal logits ahead included
    _, inverse, counts = torch.unique_consecutive(xs, return_inverse=True, return_counts=True)
    starts = counts.cumsum(0) - counts
    return order, xs, before[starts][inverse]


def reference_distribution(row, temperature=1.0, top_k=0, top_p=1.0):
    """(keep [V] bool, c [V] float64) of one row: the survivor set of the filters and the
    running sum of the renormalised probabilities in index order; ``None`` where there is
    nothing to draw from (the greedy rule applies)."""
    x = _clean(row)
    xmax = x.max()
    if not math.isfinite(float(xmax)):
        return None
    keep, e = _kept_masses(x, temperature, top_k)
    if float(top_p) < 1.0:
        order, xs, greater = _mass_above(x, e)
        stay = (greater < float(top_p) * e.sum()) | (xs == xmax)
        keep2 = torch.zeros_like(keep)
        keep2[order] = stay
        keep &= keep2
        e = torch.where(keep, e, torch.zeros_like(e))
    total = float(e.sum())
    if not (total > 0.0 and math.isfinite(total)):
        return None
    return keep, (e / total).cumsum(0)


def reference_top_p_margin(row, temperature=1.0, top_k=0, top_p=1.0) -> float:
    """How far the top-p decision of one (finite-maximum) row is from flipping: the least
    ``|mass of the strictly greater logits - top_p|`` over the row's logits, as a fraction of
    the kept mass.  Tests choose inputs whose margin is far above fp32 rounding."""
    x = _clean(row)
    _, e = _kept_masses(x, temperature, top_k)
    _, _, greater = _mass_above(x, e)
    return float((greater / e.sum() - float(top_p)).abs().min())


def reference_pick(dist, u: float, row=None) -> int:
    """The token drawn from ``reference_distribution``'s result with the uniform ``u``."""
    if dist is None:
        return reference_greedy(row)
    keep, c = dist
    i = int(torch.searchsorted(c, torch.tensor(float(u), dtype=torch.float64), right=True))
    if i >= c.numel():  # rounding left u >= c[-1]: the last token with mass
        i = int((torch.diff(c, prepend=torch.zeros(1, dtype=c.dtype)) > 0).nonzero()[-1, 0])
    return i


def _reference_tokens(logits, seed, step, do_sample, temperature, top_k, top_p):
    out = []
    for b in range(logits.shape[0]):
        row = logits[b]
        if not do_sample:
            out.append(reference_greedy(row))
        else:
            out.append(reference_pick(reference_distribution(row, temperature, top_k, top_p),
                                      philox_u(seed, step, b), row))
    return torch.tensor(out, dtype=torch.long, device=logits.device)


# ---------------------------------------------------------------------- dispatch
def sample_kernel_ok(logits) -> bool:
    """Whether ``sample_tokens`` / ``sample_step`` run the gfx950 kernel on these logits
    (``pa_sample_ok``), else the float64 reference."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dim() == 2
            and logits.dtype in (torch.bfloat16, torch.float32)):
        return False
    B, V = logits.shape
    if B < 1 or V < 1 or V > MAX_VOCAB or (V > 1 and logits.stride(1) != 1):
        return False
    ld = logits.stride(0) if B > 1 else V
    return bool(N.lib().pa_sample_ok(N.dt(logits), B, V, ld, logits.data_ptr()))


def _launch(logits, seed, step_ptr, step_val, do_sample, temperature, top_k, top_p, tok, st):
    """The one place the sampling kernel is launched from (tests wrap this to count)."""
    B, V = logits.shape
    ld = logits.stride(0) if B > 1 else V
    if st is None:
        book = (None, 0, None, None, -1, 0)
    else:
        book = (N.ptr(st.out), st.max_new_tokens, N.ptr(st.lengths), N.ptr(st.done),
                -1 if st.eos_token_id is None else st.eos_token_id, st.pad_token_id)
    N.call("pa_sample", N.dt(logits), N.ptr(logits), ld, B, V, int(seed) & _M64, step_ptr, step_val,
           int(bool(do_sample)), float(temperature), int(top_k or 0), float(top_p), N.ptr(tok), *book, N.stream())
    return tok


def _check_logits(logits, what):
    if not (torch.is_tensor(logits) and logits.dim() == 2 and logits.shape[0] >= 1 and logits.shape[1] >= 1):
        raise ValueError(f"{what}: logits must be [B, V] with B, V >= 1")


@torch.no_grad()
def sample_tokens(logits, seed=0, step=0, do_sample=False, temperature=1.0, top_k=0, top_p=1.0):
    """tok [B] int64: the next token of each row of ``logits`` [B, V] (see the module
    docstring).  ``step`` is an int or an int32 device tensor [1]."""
    _check_logits(logits, "sample_tokens")
    if sample_kernel_ok(logits):
        sp, sv = _step_args(step)
        tok = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
        return _launch(logits, seed, sp, sv, do_sample, temperature, top_k, top_p, tok, None)
    return _reference_tokens(logits, seed, int(step), do_sample, temperature, top_k, top_p)


class SamplerState:
    """The device-side state of a generation loop (what ``generate()`` keeps per call):
    ``tok`` [B] int64 the last token, ``out`` [B, max_new_tokens] int64 (``pad_token_id``
    where nothing was written), ``lengths`` [B] int64 (``max_new_tokens`` until a row hits
    EOS), ``done`` [B] bool and ``step`` [1] int32, the number of ``sample_step`` calls."""

    def __init__(self, B, max_new_tokens, device=None, eos_token_id=None, pad_token_id=0):
        self.batch, self.max_new_tokens = int(B), int(max_new_tokens)
        if self.batch < 1 or self.max_new_tokens < 1:
            raise ValueError("SamplerState: B and max_new_tokens must be at least 1")
        self.device = torch.device(device if device is not None else "cpu")
        self.eos_token_id = None if eos_token_id is None else int(eos_token_id)
        self.pad_token_id = int(pad_token_id)
        if self.eos_token_id is not None and self.eos_token_id < 0:
            raise ValueError("SamplerState: eos_token_id must not be negative")
        d = self.device
        self.tok = torch.zeros(self.batch, dtype=torch.long, device=d)
        self.out = torch.full((self.batch, self.max_new_tokens), self.pad_token_id, dtype=torch.long, device=d)
        self.lengths = torch.full((self.batch,), self.max_new_tokens, dtype=torch.long, device=d)
        self.done = torch.zeros(self.batch, dtype=torch.bool, device=d)
        self.step = torch.zeros(1, dtype=torch.int32, device=d)


@torch.no_grad()
def sample_step(logits, st: SamplerState, seed=0, do_sample=False, temperature=1.0, top_k=0, top_p=1.0):
    """One step of the generation loop on ``st`` (see the module docstring): select a token
    per row for step ``st.step``, do the EOS / done / lengths bookkeeping, advance
    ``st.step``.  Returns ``st.tok``.  On the GPU: two launches, no host read (a step past
    ``max_new_tokens`` writes no column of ``out``)."""
    _check_logits(logits, "sample_step")
    if logits.shape[0] != st.batch or logits.device != st.tok.device:
        raise ValueError(f"sample_step: logits {tuple(logits.shape)} on {logits.device} do not match the state "
                         f"(B={st.batch} on {st.tok.device})")
    pos = getattr(st, "pos", None)  # an ops.SpecState counts the tokens written per row as well
    if sample_kernel_ok(logits):
        _launch(logits, seed, N.ptr(st.step), 0, do_sample, temperature, top_k, top_p, st.tok, st)
        N.call("pa_i32_add", N.ptr(st.step), 1, 1, N.stream())
        if pos is not None:
            N.call("pa_i32_add", N.ptr(pos), st.batch, 1, N.stream())
        return st.tok
    step = int(st.step)
    nxt = _reference_tokens(logits, seed, step, do_sample, temperature, top_k, top_p)
    nxt = torch.where(st.done, torch.full_like(nxt, st.pad_token_id), nxt)
    if 0 <= step < st.max_new_tokens:
        st.out[:, step] = nxt
    if st.eos_token_id is not None:
        hit = (nxt == st.eos_token_id) & ~st.done
        st.lengths.copy_(torch.where(hit, torch.full_like(st.lengths, step + 1), st.lengths))
        st.done |= hit
    st.tok.copy_(nxt)
    st.step += 1
    if pos is not None:
        pos += 1
    return st.tok
