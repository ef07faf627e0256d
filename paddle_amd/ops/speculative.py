"""Speculative decoding, one round: judge ``G`` candidate tokens per row, commit what survives.

``spec_judge`` / ``spec_commit`` / ``spec_verify`` run ``csrc/kernels/spec_verify.hip`` on GPU
logits (bf16 or fp32, unit column stride, ``1 <= V <= 131072``, ``1 <= G <= 16``); CPU tensors
and everything else run the float64 definitions below, which are the specification and the
oracle of the GPU tests.  They reuse the distribution, the draw and the greedy rule of
:mod:`paddle_amd.ops.sampling`.  Inference ops: nothing is recorded on the tape.

One round.  The target was fed ``x0, d_0 .. d_{G-1}`` (``x0`` the row's last emitted token,
not yet in the cache) and returned logits ``[B, G+1, V]``: logits ``j`` judge candidate
``d_j``.  The draft's logits ``[B, G, V]`` are those ``d_j`` was drawn from.

Random numbers: Philox4x32-10 as in ops/sampling.py with a third counter word, counter
``(c0, row, c2, 0)``; ``philox_u(seed, step, row)`` is ``c2 = 0``.  The judge uses
``c0 = round``, the accept test of candidate ``j`` ``c2 = 2j + 1``, the replacement or bonus
draw at position ``j`` ``c2 = 2j + 2``.  The draft's own draws are ordinary ``sample_tokens``
calls (``c2 = 0``) with ``step = 1 + round * G + j``, so no counter is used twice.

Judge, per (row, position ``j``), independent of every other position and row.  ``P_j`` is
``reference_distribution(target[j], temperature, top_k, top_p)`` as probabilities ``p`` (0
outside the survivor set), ``Q_j`` the same from the draft's logits: the filters apply to
both, which is what makes the output distributed as the *filtered* target.

* greedy (``do_sample=False``; the draft's logits may be ``None``):
  ``accept[j] = (d_j == greedy(target[j]))``, ``alt[j] = greedy(target[j])`` for ``j`` in ``0..G``;
* sampled, ``j < G``: ``accept[j]`` iff ``0 <= d_j < V`` and ``u * q(d_j) < p(d_j)`` (so
  ``q = 0, p > 0`` accepts and ``q = 0, p = 0`` rejects); ``alt[j]`` is drawn from
  ``r = max(p - q, 0)``: the first index, in vocabulary order, with ``u' * sum(r) <`` the
  running sum (the last index with ``r > 0`` when rounding leaves none); where ``sum(r)`` is
  not positive and finite, from ``p`` instead.  Where ``P_j`` is ``None`` (nothing to draw
  from) the greedy rule decides; where ``Q_j`` is ``None``, ``q`` is one-hot at the draft's
  greedy token;
* sampled, ``j = G``: ``alt[G]`` is drawn from ``P_G`` with ``u'``;
* a candidate outside ``[0, V)`` is rejected and never used as an index; NaN counts as
  ``-inf``; every ``alt`` is in ``[0, V)`` for any input.

Commit, per row, sequential, integers only, on a :class:`SpecState`.  ``a`` is the first
rejected ``j`` (``G`` if none); the emitted tokens are ``d_0 .. d_{a-1}, alt[a]``.  A row that is
``done`` emits nothing (``kept = 0``, ``tok = pad``).  Otherwise the tokens go to
``out[b, pos[b]++]`` in order; a token equal to ``eos`` sets ``lengths[b] = pos`` (after the
increment) and ``done`` and ends the row's round; reaching ``max_new_tokens`` sets ``done`` and
ends it too (``lengths`` stays ``max_new_tokens``).  Nothing is written outside
``out[b, 0:max_new_tokens]``.  ``kept[b]`` is the number of tokens emitted this round,
``0..G+1`` -- also the number of fed tokens that stay in the cache (``x0`` and the emitted
candidates); ``tok[b]`` the last emitted token, the next ``x0``; ``accepted[b] += min(a, emitted)``.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from . import sampling as S
from .sampling import SamplerState, reference_distribution, reference_greedy, reference_pick

__all__ = ["SpecState", "spec_judge", "spec_commit", "spec_verify", "spec_kernel_ok", "philox3_u",
           "spec_reference", "spec_margins", "reference_judge_one", "MAX_DRAFT"]

MAX_DRAFT = 16
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------- Philox4x32-10, three words
def philox3_x0(seed: int, c0: int, c1: int, c2: int = 0) -> int:
    """First output word of Philox4x32-10 for key (seed lo, seed hi), counter (c0, c1, c2, 0)."""
    seed = int(seed) & _M64
    k0, k1 = seed & _M32, seed >> 32
    x0, x1, x2, x3 = int(c0) & _M32, int(c1) & _M32, int(c2) & _M32, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ k0, p1 & _M32, (p0 >> 32) ^ x3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return x0


def philox3_u(seed: int, c0: int, row: int, c2: int = 0) -> float:
    """The uniform of counter (c0, row, c2, 0): a multiple of 2**-24 in [0, 1).  ``c2 = 0`` is
    ``sampling.philox_u(seed, c0, row)``."""
    return (philox3_x0(seed, c0, row, c2) >> 8) * 2.0 ** -24


# ---------------------------------------------------------------------- float64 reference
def _probs(row, dist, temperature):
    """p [V] float64 of a row and its ``reference_distribution`` result: the masses of the
    survivors over their sum, exactly 0 outside the survivor set (and not a difference of the
    running sum, which would round a tiny probability to 0)."""
    keep, _ = dist
    x = S._clean(row)
    e = torch.where(keep, torch.exp((x - x.max()) / max(float(temperature), 1e-6)), torch.zeros_like(x))
    return e / e.sum()


def _pick_from(c, u):
    """First index with ``u < c_i`` of a running sum ``c`` that ends at (about) 1; the last
    index with mass when rounding leaves none."""
    return reference_pick((None, c), u)


def reference_judge_one(t_row, d_row, d, u, u2, do_sample, temperature, top_k, top_p, last, dists=None):
    """One (row, position) of the judge (``dists``: the two ``reference_distribution`` results
    of the target's and the draft's row, when the caller has them already).  Returns a dict:
    ``accept`` (None at the last position); ``alt``; ``kind`` of the draw (``"greedy"``,
    ``"residual"``, or ``"target"``: a draw from P); ``margin`` = ``|u q(d) - p(d)|`` with ``p_d`` =
    ``p(d)`` and ``q_d`` = ``q(d)`` (None where no accept test with a margin ran); ``sum_r`` (None
    unless the residual was formed); ``keep`` / ``c``: the survivor set and the normalised
    running sum the draw was taken from (None for ``"greedy"``)."""
    V = t_row.numel()
    d = None if last else int(d)
    rec = dict(accept=None, alt=None, kind="greedy", margin=None, p_d=None, q_d=None, sum_r=None, keep=None,
               c=None)
    if dists is not None:
        P, Q = dists if do_sample else (None, None)
    else:
        P = reference_distribution(t_row, temperature, top_k, top_p) if do_sample else None
        Q = reference_distribution(d_row, temperature, top_k, top_p) if do_sample and P is not None and not last \
            else None
    if P is None:
        g = reference_greedy(t_row)
        rec["alt"] = g
        if not last:
            rec["accept"] = d == g
        return rec
    if last:
        rec.update(alt=reference_pick(P, u2, t_row), kind="target", keep=P[0], c=P[1])
        return rec
    p = _probs(t_row, P, temperature)
    if Q is None:
        q = torch.zeros_like(p)
        q[reference_greedy(d_row)] = 1.0
    else:
        q = _probs(d_row, Q, temperature)
    if 0 <= d < V:
        rec["p_d"], rec["q_d"] = float(p[d]), float(q[d])
        rec["margin"] = abs(u * float(q[d]) - float(p[d]))
        rec["accept"] = bool(u * float(q[d]) < float(p[d]))
    else:
        rec["accept"] = False
    r = (p - q).clamp_(min=0.0)
    s = float(r.sum())
    rec["sum_r"] = s
    if s > 0.0 and math.isfinite(s):
        c = (r / s).cumsum(0)
        rec.update(alt=_pick_from(c, u2), kind="residual", keep=r > 0, c=c)
    else:
        rec.update(alt=reference_pick(P, u2, t_row), kind="target", keep=P[0], c=P[1])
    return rec


def spec_reference(target_logits, draft_tokens, draft_logits, seed=0, round=0, do_sample=False, temperature=1.0,
                   top_k=0, top_p=1.0):
    """The float64 judge with everything the tests choose inputs by: a list over rows of
    lists over positions ``0..G`` of the records of ``reference_judge_one``."""
    B, G1, V = target_logits.shape
    G = G1 - 1
    rnd = int(round)
    t = target_logits.detach().cpu()
    dl = None if draft_logits is None else draft_logits.detach().cpu()
    dt = draft_tokens.detach().cpu()
    out = []
    for b in range(B):
        recs = []
        for j in range(G1):
            last = j == G
            recs.append(reference_judge_one(t[b, j], None if (last or dl is None) else dl[b, j],
                                           0 if last else dt[b, j],
                                           philox3_u(seed, rnd, b, 2 * j + 1),
                                           philox3_u(seed, rnd, b, 2 * j + 2),
                                           do_sample, temperature, top_k, top_p, last))
        out.append(recs)
    return out


def spec_margins(target_logits, draft_tokens, draft_logits, seed=0, round=0, do_sample=True, temperature=1.0,
                 top_k=0, top_p=1.0):
    """(margin [B, G], sum_r [B, G]) float64 of the sampled judge: per candidate
    ``|u q(d) - p(d)|``, how far its accept test is from flipping, and ``sum(r)``, the mass of
    the residual its replacement is drawn from (NaN where the position has none)."""
    recs = spec_reference(target_logits, draft_tokens, draft_logits, seed, round, do_sample, temperature, top_k, top_p)
    nan = float("nan")
    m = torch.tensor([[nan if r["margin"] is None else r["margin"] for r in row[:-1]] for row in recs],
                     dtype=torch.float64)
    s = torch.tensor([[nan if r["sum_r"] is None else r["sum_r"] for r in row[:-1]] for row in recs],
                     dtype=torch.float64)
    return m, s


def _reference_judge(target_logits, draft_tokens, draft_logits, seed, rnd, do_sample, temperature, top_k, top_p):
    recs = spec_reference(target_logits, draft_tokens, draft_logits, seed, rnd, do_sample, temperature, top_k, top_p)
    dev = target_logits.device
    accept = torch.tensor([[bool(r["accept"]) for r in row[:-1]] for row in recs], dtype=torch.bool, device=dev)
    alt = torch.tensor([[int(r["alt"]) for r in row] for row in recs], dtype=torch.long, device=dev)
    return accept, alt


# ---------------------------------------------------------------------- state
class SpecState(SamplerState):
    """The device-side state of a speculative generation loop: a ``SamplerState``'s fields
    plus, per row and int32, ``pos`` (the tokens written to ``out`` so far), ``kept`` (the
    tokens the last round emitted) and ``accepted`` (the accepted candidates, summed).  The
    first token goes through ``ops.sample_step`` on it, after which ``pos`` is 1."""

    def __init__(self, B, max_new_tokens, num_draft, device=None, eos_token_id=None, pad_token_id=0):
        super().__init__(B, max_new_tokens, device, eos_token_id, pad_token_id)
        self.num_draft = int(num_draft)
        if not 1 <= self.num_draft <= MAX_DRAFT:
            raise ValueError(f"SpecState: num_draft must be in 1..{MAX_DRAFT}, got {num_draft}")
        d = self.device
        self.pos = torch.zeros(self.batch, dtype=torch.int32, device=d)
        self.kept = torch.zeros(self.batch, dtype=torch.int32, device=d)
        self.accepted = torch.zeros(self.batch, dtype=torch.int32, device=d)


# ---------------------------------------------------------------------- dispatch
def _strides(t):
    """(row stride, position stride) in elements of a [B, T, V] tensor, for a size-1 dimension 0."""
    return (t.stride(0) if t.shape[0] > 1 else 0), (t.stride(1) if t.shape[1] > 1 else 0)


def _check_shapes(target_logits, draft_tokens, draft_logits, do_sample, what):
    if not (torch.is_tensor(target_logits) and target_logits.dim() == 3 and target_logits.shape[0] >= 1
            and target_logits.shape[1] >= 2 and target_logits.shape[2] >= 1):
        raise ValueError(f"{what}: target_logits must be [B, G+1, V] with B, G, V >= 1")
    B, G1, V = target_logits.shape
    G = G1 - 1
    if G > MAX_DRAFT:
        raise ValueError(f"{what}: at most {MAX_DRAFT} candidates per row, got {G}")
    if not (torch.is_tensor(draft_tokens) and tuple(draft_tokens.shape) == (B, G)
            and draft_tokens.dtype == torch.long and draft_tokens.device == target_logits.device):
        raise ValueError(f"{what}: draft_tokens must be int64 [{B}, {G}] on {target_logits.device}")
    if draft_logits is None:
        if do_sample:
            raise ValueError(f"{what}: do_sample=True needs the draft's logits")
    elif not (torch.is_tensor(draft_logits) and tuple(draft_logits.shape) == (B, G, V)
              and draft_logits.device == target_logits.device):
        raise ValueError(f"{what}: draft_logits must be [{B}, {G}, {V}] on {target_logits.device}")
    return B, G, V


def spec_kernel_ok(target_logits, draft_logits=None, do_sample=False) -> bool:
    """Whether ``spec_judge`` / ``spec_verify`` run the gfx950 kernel on these logits
    (``pa_spec_judge_ok``), else the float64 reference."""
    t, d = target_logits, draft_logits
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.dtype in (torch.bfloat16, torch.float32)):
        return False
    B, G1, V = t.shape
    if B < 1 or G1 < 2 or V < 1 or (V > 1 and t.stride(2) != 1):
        return False
    if d is not None and not (torch.is_tensor(d) and d.is_cuda and d.dtype == t.dtype
                              and tuple(d.shape) == (B, G1 - 1, V) and (V == 1 or d.stride(2) == 1)):
        return False
    if d is None and do_sample:
        return False
    trs, tps = _strides(t)
    drs, dps = _strides(d) if d is not None else (0, 0)
    return bool(N.lib().pa_spec_judge_ok(N.dt(t), B, G1 - 1, V, t.data_ptr(), trs, tps,
                                         0 if d is None else d.data_ptr(), drs, dps, int(bool(do_sample))))


def _launch_judge(target_logits, draft_tokens, draft_logits, seed, rp, rv, do_sample, temperature, top_k, top_p,
                  out=None):
    """The one place the judge kernel is launched from (tests wrap this to count)."""
    B, G1, V = target_logits.shape
    G = G1 - 1
    dev = target_logits.device
    if out is None:
        out = (torch.empty(B, G, dtype=torch.bool, device=dev), torch.empty(B, G1, dtype=torch.long, device=dev))
    accept, alt = out
    if not (tuple(accept.shape) == (B, G) and accept.dtype == torch.bool and accept.is_contiguous()
            and tuple(alt.shape) == (B, G1) and alt.dtype == torch.long and alt.is_contiguous()
            and accept.device == dev and alt.device == dev):
        raise ValueError(f"spec_judge: out must be contiguous (bool [{B}, {G}], int64 [{B}, {G1}]) on {dev}")
    cand = draft_tokens.contiguous()
    trs, tps = _strides(target_logits)
    drs, dps = _strides(draft_logits) if draft_logits is not None else (0, 0)
    N.call("pa_spec_judge", N.dt(target_logits), N.ptr(target_logits), trs, tps, N.ptr(draft_logits), drs, dps,
           N.ptr(cand), B, G, V, int(seed) & _M64, rp, rv, int(bool(do_sample)), float(temperature),
           int(top_k or 0), float(top_p), N.ptr(accept), N.ptr(alt), N.stream())
    return accept, alt


@torch.no_grad()
def spec_judge(target_logits, draft_tokens, draft_logits=None, seed=0, round=0, do_sample=False, temperature=1.0,
               top_k=0, top_p=1.0, out=None):
    """(accept [B, G] bool, alt [B, G+1] int64) of one round (see the module docstring).
    ``round`` is an int or an int32 device tensor [1]; ``out``: the two tensors to write."""
    _check_shapes(target_logits, draft_tokens, draft_logits, do_sample, "spec_judge")
    if not do_sample:
        draft_logits = None  # the greedy rule does not look at them
    if spec_kernel_ok(target_logits, draft_logits, do_sample):
        rp, rv = S._step_args(round)
        return _launch_judge(target_logits, draft_tokens, draft_logits, seed, rp, rv, do_sample, temperature,
                             top_k, top_p, out)
    accept, alt = _reference_judge(target_logits, draft_tokens, draft_logits, seed, int(round), do_sample,
                                   temperature, top_k, top_p)
    if out is not None:
        out[0].copy_(accept)
        out[1].copy_(alt)
        return out
    return accept, alt


def _reference_commit(accept, alt, draft_tokens, st):
    B, G = accept.shape
    acc, al, dt = accept.cpu().tolist(), alt.cpu().tolist(), draft_tokens.cpu().tolist()
    for b in range(B):
        pos = int(st.pos[b])
        if bool(st.done[b]) or pos < 0 or pos >= st.max_new_tokens:
            st.done[b] = True
            st.kept[b] = 0
            st.tok[b] = st.pad_token_id
            continue
        a = next((j for j in range(G) if not acc[b][j]), G)
        emitted, last, done = 0, st.pad_token_id, False
        for t in range(a + 1):
            last = dt[b][t] if t < a else al[b][a]
            st.out[b, pos] = last
            pos += 1
            emitted += 1
            if st.eos_token_id is not None and last == st.eos_token_id:
                st.lengths[b] = pos
                done = True
            elif pos >= st.max_new_tokens:
                done = True
            if done:
                break
        if done:
            st.done[b] = True
        st.pos[b] = pos
        st.tok[b] = last
        st.kept[b] = emitted
        st.accepted[b] += min(a, emitted)


@torch.no_grad()
def spec_commit(accept, alt, draft_tokens, st: SpecState):
    """The bookkeeping of one round on ``st`` (see the module docstring).  On the GPU: one
    launch of one thread per row, no host read.  Returns ``st.kept``."""
    if not (torch.is_tensor(accept) and accept.dim() == 2 and accept.dtype == torch.bool):
        raise ValueError("spec_commit: accept must be a bool tensor [B, G]")
    B, G = accept.shape
    if B != st.batch or not 1 <= G <= MAX_DRAFT or tuple(alt.shape) != (B, G + 1) or alt.dtype != torch.long \
            or tuple(draft_tokens.shape) != (B, G) or draft_tokens.dtype != torch.long:
        raise ValueError(f"spec_commit: need accept [{st.batch}, G], alt [B, G+1] int64 and draft_tokens [B, G] "
                         f"int64 with G in 1..{MAX_DRAFT}")
    dev = st.tok.device
    if not (accept.device == dev and alt.device == dev and draft_tokens.device == dev):
        raise ValueError(f"spec_commit: every tensor must be on the state's device ({dev})")
    if dev.type == "cuda":
        accept, alt, cand = accept.contiguous(), alt.contiguous(), draft_tokens.contiguous()
        N.call("pa_spec_commit", N.ptr(accept), N.ptr(alt), N.ptr(cand), B, G, N.ptr(st.out), st.max_new_tokens,
               N.ptr(st.lengths), N.ptr(st.done), N.ptr(st.pos), N.ptr(st.tok), N.ptr(st.kept), N.ptr(st.accepted),
               -1 if st.eos_token_id is None else st.eos_token_id, st.pad_token_id, N.stream())
    else:
        _reference_commit(accept, alt, draft_tokens, st)
    return st.kept


@torch.no_grad()
def spec_verify(target_logits, draft_tokens, draft_logits, st: SpecState, seed=0, round=0, do_sample=False,
                temperature=1.0, top_k=0, top_p=1.0):
    """``spec_judge`` then ``spec_commit`` on ``st``: two launches on the GPU, no host read.
    Returns ``(accept, alt)``."""
    accept, alt = spec_judge(target_logits, draft_tokens, draft_logits, seed, round, do_sample, temperature,
                             top_k, top_p)
    spec_commit(accept, alt, draft_tokens, st)
    return accept, alt
