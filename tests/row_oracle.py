"""Per-row float64 oracle for the row kernels (CPU only, plain torch): RMSNorm / LayerNorm,
softmax / log-softmax / softmax cross-entropy, embedding, rotary and SwiGLU.

The convention is the attention oracle's (tests/attn_oracle.py).  Every ``*_reference``
takes the rounded inputs the kernel gets and returns each output in float64, and next to
it a **magnitude** tensor: the same expression with every term replaced by its absolute
value (``magy = (|h| + |mean|) rstd |w| + |b|`` ...).  ``row_stat`` divides the 2-norm of
a row's error by the 2-norm of that row's magnitude, so a bound is a multiple of the unit
roundoff and does not depend on how much a sum cancels; dw / db are compared per column.
A backward reference is evaluated where the kernel evaluates it: at the h (or y) the
forward stored, rounded to the storage dtype, with mean / rstd / lse from unrounded data.

What torch leaves as NaN is defined here: a label equal to ``ignore_index`` or outside
[0, V) gives loss 0 and gradient 0 for its row, and a mean over no valid label is 0.

``*_emulated`` is the same formula in float32 with one rounding to the storage dtype at
each kernel output.  It is the yardstick the bounds are checked against on the CPU
(``EMU_MARGIN``), never an expected value.

Bounds (derived, not tuned; u = 2^-9 is the bf16 unit roundoff):

    bf16 outputs                     4u          one output rounding plus the rounded saved
                                                 h / y (half the attention oracle's 8u: no
                                                 intermediate P is rounded here)
    fp32 norm / rotary outputs, dx   2^-16       a lane sums at most H / 64 = 128 terms, then
                                                 6 shuffle steps: (128 + 6 + a few) 2^-24
    fp32 probabilities, dlogits,     2^-14       an __expf argument of magnitude up to 2^7
      softmax dx, SwiGLU                         carries 2^7 2^-23 of absolute error, times 4
    lse, per-row loss, mean loss     1e-4 max(1, |ref|)   (attn_oracle.LSE_TOL)
    dw / db, per column              4u (bf16); 2^-16 + N 2^-24 (fp32)
    embedding dW, per row            4u (bf16); 2^-16 + n 2^-24 (fp32), n = the largest
                                                 number of rows that carry one id

One term is added by derivation.  The cross-entropy kernels keep lse = m + log(s) as ONE
fp32 number and form p = exp(x - lse) and loss = lse - x[label] from it, so both inherit
the rounding of that number, 2^-24 |lse| absolute: ``lse_slack`` = 2^-23 |lse| (twice
that) is added to the fp32 probability bound (as a relative error of p) and to the loss
bounds.  At |lse| of about 12 (every profile but ``offset``) it is 1.4e-6, at the offset
profile's 3e4 it is 3.6e-3.  The CPU emulation shows the same figure.

Worst statistics measured on the MI355X (tests/test_row_kernels_oracle_gpu.py):

    apply_rotary                 bf16  dx 2.51e-03  roundtrip 4.07e-03  y 2.86e-03
    apply_rotary                 fp32  dx 5.93e-08  roundtrip 1.06e-07  y 5.62e-08
    embedding                    bf16  dW 1.46e-03
    embedding                    fp32  dW 3.51e-08
    layer_norm                   bf16  db 3.89e-03  dres 2.38e-03  dw 3.88e-03  dx 2.38e-03  h 3.40e-03  y 3.74e-03
    layer_norm                   fp32  db 1.26e-07  dres 3.27e-07  dw 5.28e-06  dx 3.59e-07  h 4.88e-08  y 5.87e-07
    layer_norm_stats             bf16  db 1.24e-03  dw 2.97e-03  dx 1.06e-03  mean 1.41e-07  rstd 1.81e-07  y 3.63e-03
    layer_norm_stats             fp32  db 5.05e-08  dw 2.21e-07  dx 8.08e-08  mean 2.39e-07  rstd 1.32e-07  y 1.45e-07
    log_softmax                  bf16  dx 1.88e-03  y 2.65e-03
    log_softmax                  fp32  dx 2.02e-07  y 6.05e-08
    norm, reference path         bf16  db 3.77e-03  dres 1.15e-03  dw 6.27e-03  dx 1.15e-03  h 1.55e-03  y 1.70e-03
    norm, reference path         fp32  db 1.31e-07  dres 3.77e-08  dw 2.03e-07  dx 3.77e-08  h 2.28e-08  y 8.95e-08
    pa_rope alias                bf16  y 1.99e-03
    pa_rope fp32_to_bf16         bf16  y 2.03e-03
    pa_rope n_rot                bf16  y 1.99e-03
    pa_rope pos                  bf16  y 1.98e-03
    pa_rope stride               bf16  y 1.99e-03
    rms_norm                     bf16  dres 3.20e-03  dw 3.88e-03  dx 3.20e-03  h 3.23e-03  y 3.87e-03
    rms_norm                     fp32  dres 5.64e-07  dw 7.69e-07  dx 5.64e-07  h 4.93e-08  y 5.99e-07
    softmax                      bf16  dx 1.96e-03  y 3.49e-03
    softmax                      fp32  dx 5.08e-07  y 8.72e-07
    softmax_cross_entropy        bf16  dlogits 2.78e-03  dlogits_off 3.53e-03  loss 1.68e-05  lse 1.54e-07  mean 1.68e-05  sum 1.68e-05
    softmax_cross_entropy        fp32  dlogits 6.38e-04  dlogits_off 9.74e-04  loss 2.56e-05  lse 1.54e-07  mean 1.57e-05  sum 1.50e-05
    swiglu                       bf16  dgu 3.63e-03  out 3.52e-03
    swiglu                       fp32  dgu 7.13e-08  out 5.81e-08
    swiglu, reference path       bf16  dgu 2.90e-03  out 2.24e-03
    swiglu, reference path       fp32  dgu 3.64e-08  out 3.04e-08

    (softmax_cross_entropy rows include the ``offset`` profile, whose fp32 bound is
    2^-14 + 2^-23 * 3e4 = 3.6e-3; "norm, reference path" and "swiglu, reference path" are the
    shapes the kernels refuse, run through the public ops.)
"""
import torch

from attn_oracle import LSE_TOL, U, row_stat  # noqa: F401  (re-exported)

BF16_BOUND = 4 * U
F32_SUM_BOUND = 2.0 ** -16
F32_EXP_BOUND = 2.0 ** -14
EMU_MARGIN = 2.0  # the emulation must meet every bound with this factor to spare

NORM_PROFILES = ("flat", "offset", "tiny", "mixed_rows", "spike")
LOGIT_PROFILES = ("flat", "offset", "spike", "masked_tail", "masked_groups", "ties")
MASKED_PROFILES = ("masked_tail", "masked_groups")

# the GPU test's shapes (the CPU feasibility test walks the same lists)
NORM_H = (8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
NORM_N = (1, 5, 67)
NORM_BIG = ((8193, 8), (8193, 520))  # (N, H): the backward's block cap binds, rows_per_block = 17
SOFTMAX_V = (1, 7, 8, 1001, 2048, 2056, 4104)
SOFTMAX_N = (1, 3, 33)
EMB_TOKENS = (1, 65, 8192, 8193, 8300)
EMB_H = (8, 264)
EMB_CASES = tuple((n, h) for n in EMB_TOKENS for h in EMB_H) + ((130, 4104),)  # (tokens, H); 4104: two column passes
ROPE_D = (16, 64, 128)
ROPE_S = (1, 100)
SWIGLU_I = (8, 1376)
SWIGLU_N = (1, 513)

# mirrors of the launchers' constants (csrc/kernels/norm.hip, elementwise.hip)
NORM_BWD_RPB_MIN = 16
NORM_BWD_GCAP = 512
EMB_BWD_ROWS = 8192
EMB_BWD_U = 16


def sum_bound(dtype):
    """Outputs that are short fp32 sums (norms, rotary)."""
    return BF16_BOUND if dtype == torch.bfloat16 else F32_SUM_BOUND


def exp_bound(dtype):
    """Outputs that go through __expf (probabilities, dlogits, SwiGLU)."""
    return BF16_BOUND if dtype == torch.bfloat16 else F32_EXP_BOUND


def acc_bound(dtype, n):
    """Column / row sums of n terms accumulated in fp32 (dw, db, embedding dW)."""
    return BF16_BOUND if dtype == torch.bfloat16 else F32_SUM_BOUND + n * 2.0 ** -24


def lse_slack(lse):
    return 2.0 ** -23 * lse.detach().double().abs()


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _to(cd, *ts):
    return [None if t is None else t.detach().cpu().to(cd) for t in ts]


def _rounder(store, on):
    if not on:
        return lambda t: t
    return lambda t: None if t is None else t.to(store).to(t.dtype)


def _stored(t, store):
    """t as the kernel reads it back from a tensor of dtype ``store``."""
    return t.to(store).to(t.dtype)


# ====================================================================== norm
def norm_bwd_blocks(N, rpi=4):
    """[(r0, r1, partial)] per block of the norm backward: its contiguous row range and
    the rows of its last block iteration when that iteration is not full (else None).
    ``rpi`` rows are in flight per iteration (4, or 2 when two waves share a row)."""
    G = min((N + NORM_BWD_RPB_MIN - 1) // NORM_BWD_RPB_MIN, NORM_BWD_GCAP)
    G = max(G, 1)
    rpb = (N + G - 1) // G
    out = []
    for r0 in range(0, N, rpb):
        r1 = min(N, r0 + rpb)
        tail = (r1 - r0) % rpi
        out.append((r0, r1, list(range(r1 - tail, r1)) if tail else None))
    return out


def norm_inputs(profile, N, H, dtype, with_res=False, with_bias=False, seed=0):
    """dict of CPU tensors in ``dtype``: x, res, w, b, dy, dh (res / b None unless asked)."""
    g = _gen(seed, N, H, NORM_PROFILES.index(profile), with_res, with_bias)
    x = torch.randn(N, H, generator=g, dtype=torch.float64)
    if profile == "offset":
        x = x + 1000.0
    elif profile == "tiny":
        x = x * 1e-4
    elif profile == "mixed_rows":
        x = x * (10.0 ** ((torch.arange(N) % 7) - 3).double()).view(N, 1)
    elif profile == "spike":
        x[torch.arange(N), (torch.arange(N) * 37) % H] = 1e4
    elif profile != "flat":
        raise ValueError(profile)
    res = torch.randn(N, H, generator=g, dtype=torch.float64) if with_res else None
    if res is not None and profile == "tiny":
        res = res * 1e-4
    if res is not None and profile == "mixed_rows":
        res = res * (10.0 ** ((torch.arange(N) % 7) - 3).double()).view(N, 1)
    w = 1 + 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(H, generator=g, dtype=torch.float64) if with_bias else None
    dy = torch.randn(N, H, generator=g, dtype=torch.float64)
    dh = torch.randn(N, H, generator=g, dtype=torch.float64) if with_res else None
    r = lambda t: None if t is None else t.to(dtype)
    return dict(x=r(x), res=r(res), w=r(w), b=r(b), dy=r(dy), dh=r(dh))


def _norm(x, res, w, b, dy, dh, eps, rms, cd, store, emu, mut=None):
    x, res, w, b, dy, dh = _to(cd, x, res, w, b, dy, dh)
    rnd = _rounder(store, emu)
    mut = mut or {}
    N, H = x.shape
    h = x + res if res is not None else x
    if rms:
        mean = torch.zeros(N, 1, dtype=cd)
        ms = (h * h).sum(-1, keepdim=True) / H
    else:
        mean = h.sum(-1, keepdim=True) / H
        ms = ((h - mean) ** 2).sum(-1, keepdim=True) / H
    if "rstd_short_row" in mut:  # the row's last 8-element vector left out of the sum
        i = mut["rstd_short_row"]
        ms[i] = ((h[i, : H - 8] - mean[i]) ** 2).sum() / H
    rstd = torch.rsqrt(ms + eps)
    y = (h - mean) * rstd * w
    if b is not None:
        y = y + b
    out = dict(y=rnd(y), h=rnd(h) if res is not None else None, mean=None if rms else mean.squeeze(-1),
               rstd=rstd.squeeze(-1))
    if dy is None:
        return out, None
    hs = _stored(h, store) if res is not None else h
    rb = rstd.clone()
    if "dx_rstd_from" in mut:  # row i normalised with row j's rstd
        i, j = mut["dx_rstd_from"]
        rb[i] = rstd[j]
    xhat = (hs - mean) * rb
    g = w * dy
    s2 = (g * xhat).sum(-1, keepdim=True) / H
    s1 = 0.0 if rms else g.sum(-1, keepdim=True) / H
    dx = rb * (g - s1 - xhat * s2)
    if dh is not None:
        dx = dx + dh
    keep = torch.ones(N, dtype=torch.bool)
    if "dw_drop_rows" in mut:
        keep[mut["dw_drop_rows"]] = False
    xh = (hs - mean) * rstd
    dw = (dy * xh)[keep].sum(0)
    db = dy[keep].sum(0)
    out.update(dx=rnd(dx), dw=rnd(dw), db=None if rms else rnd(db))
    if emu:
        return out, None
    axh = (hs.abs() + mean.abs()) * rstd
    ag = w.abs() * dy.abs()
    magdx = rstd * (ag + (0.0 if rms else ag.sum(-1, keepdim=True) / H) + axh * (ag * axh).sum(-1, keepdim=True) / H)
    if dh is not None:
        magdx = magdx + dh.abs()
    # rstd = (q + eps)^-1/2 with q = sum d^2 / H, d = h - mean: an error of gamma (|h| + |mean|) in
    # each d moves rstd by gamma * rstd * (sum |d| (|h| + |mean|) / H) / (q + eps) to first order
    magr = rstd * (((h - mean).abs() * (h.abs() + mean.abs())).sum(-1, keepdim=True) / H + eps) / (ms + eps)
    mag = dict(y=(h.abs() + mean.abs()) * rstd * w.abs() + (b.abs() if b is not None else 0.0),
               h=(x.abs() + res.abs()) if res is not None else None,
               mean=h.abs().sum(-1) / H, rstd=magr.squeeze(-1), dx=magdx,
               dw=(dy.abs() * axh).sum(0), db=dy.abs().sum(0))
    return out, mag


def norm_reference(x, res, w, b, dy, dh, eps, rms, _mut=None):
    """float64 RMSNorm / LayerNorm forward + backward on x [N, H] (h = x + res).
    Returns (out, mag): dicts with y, h, mean [N], rstd [N], dx (= dres), dw, db [H].
    ``dy`` None: forward only.  ``_mut`` builds the wrong results of the mutation tests."""
    return _norm(x, res, w, b, dy, dh, eps, rms, torch.float64, x.dtype, False, _mut)


def norm_emulated(x, res, w, b, dy, dh, eps, rms):
    return _norm(x, res, w, b, dy, dh, eps, rms, torch.float32, x.dtype, True)[0]


# ====================================================================== softmax / CE
def logit_inputs(profile, N, V, dtype, seed=0):
    """(logits [N, V] in ``dtype``, hot [N]): ``hot`` is a finite column of each row that
    the profile singles out (the spike, or the only finite column), else -1."""
    g = _gen(seed, N, V, LOGIT_PROFILES.index(profile))
    x = 3 * torch.randn(N, V, generator=g, dtype=torch.float64)
    hot = torch.full((N,), -1, dtype=torch.long)
    ninf = float("-inf")
    if profile == "offset":
        x = x + 3e4
    elif profile == "spike":
        hot = (torch.arange(N) * 7 + 3) % V
        x[torch.arange(N), hot] = x.max() + 80.0
    elif profile == "masked_tail":
        k = min(40, V - 1)
        if k:
            x[:, V - k:] = ninf
    elif profile == "masked_groups":
        grp = torch.arange(V) // 8
        x[:, grp % 2 == 1] = ninf
        i = N // 2  # one row with a single finite column (in the last group when that is a whole one)
        c = V - 1 if (V % 8 == 0 and ((V - 1) // 8) % 2 == 0) else 0
        keep = x[i, c].clone()
        x[i] = ninf
        x[i, c] = keep
        hot[i] = c
    elif profile == "ties":
        x = torch.randint(0, 2, (N, V), generator=g).double()  # many columns share the maximum
        x[0] = 2.5                                              # and one row is constant
    elif profile != "flat":
        raise ValueError(profile)
    return x.to(dtype), hot


LABEL_KINDS = ("first", "last", "ignored", "past_V", "negative", "random")


def make_labels(logits, hot, ignore_index=-100, kinds=LABEL_KINDS, on_hot=None, seed=0):
    """Row r gets label kind ``kinds[r % len(kinds)]``: the first / last finite column
    (0 / V - 1 unless masked), ``ignore_index``, a label >= V, a negative label that is not
    ``ignore_index``, or a random finite column.  Rows with a ``hot`` column take it when
    ``on_hot`` says so (default: even rows).  Labels never sit on a -inf column."""
    N, V = logits.shape
    g = _gen(seed, N, V, 99)
    fin = torch.isfinite(logits.float())
    lab = torch.empty(N, dtype=torch.long)
    for r in range(N):
        cols = fin[r].nonzero().flatten()
        k = kinds[r % len(kinds)]
        if k == "first":
            lab[r] = cols[0]
        elif k == "last":
            lab[r] = cols[-1]
        elif k == "ignored":
            lab[r] = ignore_index
        elif k == "past_V":
            lab[r] = V + (r % 3) * 5
        elif k == "negative":
            lab[r] = -7 if ignore_index != -7 else -8
        else:
            lab[r] = cols[torch.randint(0, len(cols), (1,), generator=g)]
        use_hot = (r % 2 == 0) if on_hot is None else on_hot
        if hot[r] >= 0 and use_hot and k in ("first", "last", "random"):
            lab[r] = hot[r]
    return lab


def _lse(x, mut=None):
    m = x.amax(-1, keepdim=True)
    e = torch.exp(x - m)
    if mut and "lse_drop_chunk" in mut:  # one aligned 8-column chunk missing from a row's sum
        i, c0 = mut["lse_drop_chunk"]
        e = e.clone()
        e[i, c0:c0 + 8] = 0
    return m + torch.log(e.sum(-1, keepdim=True))


def _ce(logits, label, dloss, ignore_index, reduction, cd, store, emu, mut=None):
    (x,) = _to(cd, logits)
    rnd = _rounder(store, emu)
    mut = mut or {}
    N, V = x.shape
    lab = label.detach().cpu().long()
    lse = _lse(x, mut)
    valid = (lab != ignore_index) & (lab >= 0) & (lab < V)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    if "label_shift" in mut:
        safe = (safe + mut["label_shift"]) % V
    xl = x.gather(1, safe.view(N, 1)).squeeze(1)
    loss = torch.where(valid, lse.squeeze(1) - xl, torch.zeros(N, dtype=cd))
    cnt = max(int(valid.sum()), 1)
    if reduction == "none":
        g = dloss.detach().cpu().to(cd).view(N)
    elif reduction == "sum":
        g = torch.full((N,), float(dloss), dtype=cd)
    else:
        g = torch.full((N,), float(dloss), dtype=cd) / cnt
    g = torch.where(valid, g, torch.zeros_like(g))
    p = torch.exp(x - lse)
    onehot = torch.zeros(N, V, dtype=cd)
    onehot[torch.arange(N), safe] = valid.to(cd)
    out = dict(lse=lse.squeeze(1), loss=loss, mean=loss.sum() / cnt, sum=loss.sum(), p=p, onehot=onehot, g=g,
               dlogits=rnd((p - onehot) * g.view(N, 1)))
    if emu:
        return out, None
    return out, dict(dlogits=(p + onehot) * g.abs().view(N, 1), p=p)


def ce_reference(logits, label, dloss=1.0, ignore_index=-100, reduction="mean", _mut=None):
    """float64 softmax cross-entropy on logits [N, V].  Returns (out, mag) with lse, loss
    [N], mean, sum (scalars), p [N, V] and dlogits for the upstream gradient ``dloss``: a
    scalar for reduction mean / sum, [N] for none."""
    return _ce(logits, label, dloss, ignore_index, reduction, torch.float64, logits.dtype, False, _mut)


def ce_emulated(logits, label, dloss=1.0, ignore_index=-100, reduction="mean"):
    return _ce(logits, label, dloss, ignore_index, reduction, torch.float32, logits.dtype, True)[0]


def _softmax(x, dy, log, cd, store, emu):
    x, dy = _to(cd, x, dy)
    rnd = _rounder(store, emu)
    lse = _lse(x)
    y = x - lse if log else torch.exp(x - lse)
    out = dict(y=rnd(y), lse=lse.squeeze(-1))
    mag = dict(y=(x.abs() + lse.abs()) if log else y)
    if dy is not None:
        ys = _stored(y, store)
        if log:
            ey = torch.exp(ys)
            dx = dy - ey * dy.sum(-1, keepdim=True)
            mag["dx"] = dy.abs() + ey * dy.abs().sum(-1, keepdim=True)
        else:
            dx = ys * (dy - (dy * ys).sum(-1, keepdim=True))
            mag["dx"] = ys * (dy.abs() + (dy.abs() * ys).sum(-1, keepdim=True))
        out["dx"] = rnd(dx)
    return out, (None if emu else mag)


def softmax_reference(x, dy=None, log=False):
    """float64 softmax / log-softmax over the last axis and its backward at the stored y."""
    return _softmax(x, dy, log, torch.float64, x.dtype, False)


def softmax_emulated(x, dy=None, log=False):
    return _softmax(x, dy, log, torch.float32, x.dtype, True)[0]


def masked_row_stat(got, ref, mag):
    """row_stat where the reference may hold -inf (log-softmax of a masked column): those
    elements must be exactly -inf in ``got`` and are left out of the norms."""
    got, ref, mag = (t.detach().cpu().double() for t in (got, ref, mag))
    neg = ref == float("-inf")
    if not (got[neg] == float("-inf")).all():
        return float("inf")
    z = torch.zeros((), dtype=torch.float64)
    return row_stat(torch.where(neg, z, got), torch.where(neg, z, ref), torch.where(neg, z, mag))


def loss_stat(got, ref, slack=0.0):
    """max |got - ref| / (max(1, |ref|) + slack / LSE_TOL): compare with LSE_TOL.  ``slack``
    (absolute, scalar or per row) is the resolution of the fp32 lse a loss is formed from
    (``lse_slack``, module docstring); 0 for lse itself."""
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    if not torch.isfinite(got).all():
        return float("inf")
    slack = torch.as_tensor(slack, dtype=torch.float64).reshape(-1)
    return ((got - ref).abs() / (ref.abs().clamp_min(1.0) + slack / LSE_TOL)).max().item()


def prob_bound(dtype, lse_ref):
    """Bound on row_stat of probabilities / dlogits formed as exp(x - lse) from a stored fp32 lse."""
    return exp_bound(dtype) + lse_slack(lse_ref).max().item()


# ====================================================================== embedding
def id_patterns(n_tok, vocab, seed=0):
    """name -> ids [n_tok] (all inside [0, vocab)); vocab >= max(n_tok, 8)."""
    g = _gen(seed, n_tok, vocab)
    pats = {"distinct": torch.randperm(vocab, generator=g)[:n_tok], "same": torch.full((n_tok,), 3, dtype=torch.long)}
    base = torch.randperm(vocab - 4, generator=g)[:n_tok] + 4  # distinct ids 4.. ; ids 0..3 are planted
    for k, cnt in enumerate((17, 33, 4000)):
        if cnt <= n_tok:
            ids = base.clone()
            ids[torch.randperm(n_tok, generator=g)[:cnt]] = k  # id k on cnt rows, anywhere
            pats[f"dup{cnt}"] = ids
    if n_tok > 130:
        ids = base.clone()
        ids[torch.tensor([62, 63, 64, 65, 127, 128])] = 0  # one id across 64-row chunk edges
        if n_tok > EMB_BWD_ROWS:
            ids[EMB_BWD_ROWS - 1] = 1  # and ids on both sides of the 8192-row range boundary
            ids[EMB_BWD_ROWS:] = torch.tensor([1, 0, 2])[torch.arange(n_tok - EMB_BWD_ROWS) % 3]
            ids[5] = 2
        pats["straddle"] = ids
    ids = base.clone()
    ids[::3] = 2
    pats["padding"] = ids  # with padding_idx = 2
    return pats


def _embedding(ids, W, dout, pad, cd, store, emu, mut=None, base=None):
    W, dout, base = _to(cd, W, dout, base)
    rnd = _rounder(store, emu)
    mut = mut or {}
    ids = ids.detach().cpu().long().reshape(-1)
    out = W[ids]
    out[ids == pad] = 0
    res, mag = dict(out=out), None
    if dout is not None:
        d = dout.reshape(ids.numel(), -1)
        keep = ids != pad
        if "drop_rows_past" in mut:
            keep[mut["drop_rows_past"]:] = False
        if "drop_nth_dup" in mut:  # the n-th (0-based) row of the most frequent id
            top = ids[keep].mode().values
            keep[(ids == top).nonzero().flatten()[mut["drop_nth_dup"]]] = False
        acc = torch.zeros_like(W) if base is None else base.clone()
        res["dW"] = rnd(acc.index_add(0, ids[keep], d[keep]))
        if not emu:
            mag = dict(dW=(torch.zeros_like(W) if base is None else base.abs()).index_add(0, ids[keep], d[keep].abs()))
    return res, mag


def embedding_reference(ids, W, dout=None, padding_idx=-1, base=None, _mut=None):
    """float64 gather ``out`` [n_tok, H] and scatter-add ``dW`` [vocab, H] (added to ``base``
    when given); rows whose id is ``padding_idx`` read zeros and contribute nothing."""
    return _embedding(ids, W, dout, padding_idx, torch.float64, W.dtype, False, _mut, base)


def embedding_emulated(ids, W, dout=None, padding_idx=-1):
    return _embedding(ids, W, dout, padding_idx, torch.float32, W.dtype, True)[0]


# ====================================================================== rotary
def rope_tables(S, D, base=10000.0):
    inv = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    return f.cos().float(), f.sin().float()


def _rot(x, c, s, sign, adjacent=False, mag=False):
    D = x.shape[-1]
    if adjacent:  # the wrong pairing (i, i + 1), for the mutation test
        a, b = x[..., 0::2], x[..., 1::2]
        return torch.stack([a * c - b * s * sign, b * c + a * s * sign], -1).reshape(x.shape)
    a, b = x[..., : D // 2], x[..., D // 2:]
    if mag:
        return torch.cat([a.abs() * c.abs() + b.abs() * s.abs(), b.abs() * c.abs() + a.abs() * s.abs()], -1)
    return torch.cat([a * c - b * s * sign, b * c + a * s * sign], -1)


def _rope(x, cos, sin, inverse, dy, pos, n_rot, cd, store, emu, mut=None):
    x, cos, sin, dy = _to(cd, x, cos, sin, dy)
    rnd = _rounder(store, emu)
    mut = mut or {}
    B, S, nh, D = x.shape
    n_rot = nh if n_rot is None else n_rot
    p = torch.arange(S).view(1, S).expand(B, S) if pos is None else pos.detach().cpu().long().view(B, S)
    c, s = cos[p].view(B, S, 1, D // 2), sin[p].view(B, S, 1, D // 2)
    sign = -1.0 if inverse else 1.0
    adj = bool(mut.get("adjacent_pairs"))

    def apply(t, sg, mag=False):
        r = _rot(t[:, :, :n_rot], c, s, sg, adj, mag)
        return torch.cat([r, t[:, :, n_rot:].abs() if mag else t[:, :, n_rot:]], 2)

    out = dict(y=rnd(apply(x, sign)))
    mag = dict(y=apply(x, sign, True))
    if dy is not None:
        out["dx"] = rnd(apply(dy, sign if mut.get("bwd_same_sign") else -sign))
        mag["dx"] = apply(dy, sign, True)
    return out, (None if emu else mag)


def rope_reference(x, cos, sin, inverse=False, dy=None, pos=None, n_rot=None, out_dtype=None, _mut=None):
    """float64 neox rotary of x [B, S, nh, D] (pairs (i, i + D/2)); heads >= n_rot are
    copied.  The backward is the rotation by the opposite angle applied to dy."""
    return _rope(x, cos, sin, inverse, dy, pos, n_rot, torch.float64, out_dtype or x.dtype, False, _mut)


def rope_emulated(x, cos, sin, inverse=False, dy=None, pos=None, n_rot=None, out_dtype=None):
    return _rope(x, cos, sin, inverse, dy, pos, n_rot, torch.float32, out_dtype or x.dtype, True)[0]


# ====================================================================== SwiGLU
SWIGLU_GATES = (30.0, -30.0, 100.0, -100.0, 0.0)


def swiglu_inputs(N, I, dtype, seed=0):
    """(gu [N, 2I] = [gate | up], dout [N, I]); the gates of every row start with
    +-30, +-100 and 0, where exp(-g) runs to 0 and past the fp32 range."""
    g = _gen(seed, N, I)
    gu = torch.randn(N, 2 * I, generator=g, dtype=torch.float64)
    gu[:, :I] *= 3
    k = min(I, len(SWIGLU_GATES))
    gu[:, :k] = torch.tensor(SWIGLU_GATES[:k], dtype=torch.float64)
    if N > 1 and I >= 8:
        gu[1::2, 3:8] = torch.tensor(SWIGLU_GATES, dtype=torch.float64)  # and at another lane offset
    return gu.to(dtype), torch.randn(N, I, generator=g, dtype=torch.float64).to(dtype)


def _swiglu(gu, dout, cd, store, emu):
    gu, dout = _to(cd, gu, dout)
    rnd = _rounder(store, emu)
    g, u = gu.chunk(2, -1)
    sg = torch.sigmoid(g)
    out = dict(out=rnd(g * sg * u))
    mag = dict(out=(g * sg * u).abs())
    if dout is not None:
        dg = dout * u * sg * (1 + g * (1 - sg))
        du = dout * g * sg
        out["dgu"] = rnd(torch.cat([dg, du], -1))
        mag["dgu"] = torch.cat([(dout * u).abs() * sg * (1 + g.abs() * (1 - sg)), du.abs()], -1)
    return out, (None if emu else mag)


def swiglu_reference(gu, dout=None):
    """float64 silu(gate) * up on gu [N, 2I] and its backward."""
    return _swiglu(gu, dout, torch.float64, gu.dtype, False)


def swiglu_emulated(gu, dout=None):
    return _swiglu(gu, dout, torch.float32, gu.dtype, True)[0]


# ====================================================================== cases and statistics
# (rms, with_res, use_dh, with_bias): with a residual, dh is both present and None
NORM_VARIANTS = [(True, False, False, False), (True, True, True, False), (True, True, False, False),
                 (False, False, False, False), (False, False, False, True), (False, True, True, False),
                 (False, True, True, True), (False, True, False, True), (False, True, False, False)]


def norm_cases(H):
    """(N, profile, rms, with_res, use_dh, with_bias) of one H: every variant at every N,
    all profiles at the largest N and ``flat`` elsewhere."""
    out = []
    for N in NORM_N:
        for prof in (NORM_PROFILES if N == NORM_N[-1] else ("flat",)):
            out += [(N, prof) + v for v in NORM_VARIANTS]
    return out


def norm_eps(rms):
    return 1e-6 if rms else 1e-5


def norm_case_reference(inp, rms, use_dh):
    return norm_reference(inp["x"], inp["res"], inp["w"], inp["b"], inp["dy"], inp["dh"] if use_dh else None,
                          norm_eps(rms), rms)


def ce_check(got, ref, mag, dtype):
    """{name: (statistic, bound)} of the cross-entropy results present in ``got``."""
    slack = lse_slack(ref["lse"])
    out = {}
    if "lse" in got:
        out["lse"] = (loss_stat(got["lse"], ref["lse"]), LSE_TOL)
    if "loss" in got:
        out["loss"] = (loss_stat(got["loss"], ref["loss"], slack), LSE_TOL)
    for n in ("mean", "sum"):
        if n in got:
            out[n] = (loss_stat(got[n], ref[n], slack.max() * (1 if n == "mean" else slack.numel())), LSE_TOL)
    if "dlogits" in got:
        b = prob_bound(dtype, ref["lse"])
        # a probability under the smallest normal fp32 number (the spike profile's exp(-85)) may be
        # flushed to zero or rounded to a denormal: an absolute error of up to 2^-126 |g|, which the
        # magnitude takes in as 2^-126 |g| / bound per element
        m = mag["dlogits"] + (2.0 ** -126 / b) * ref["g"].abs().view(-1, 1)
        out["dlogits"] = (row_stat(got["dlogits"], ref["dlogits"], m), b)
        # the label column (magnitude |g| (1 + p)) carries most of a row's norm and hides an error
        # in the other columns by |p row|_2: those columns again, on their own
        off = 1 - ref["onehot"]
        out["dlogits_off"] = (row_stat(got["dlogits"].detach().cpu().double() * off, ref["dlogits"] * off, m * off), b)
    return out


def col_stat(got, ref, mag):
    """row_stat with every column of a [H] vector as its own row (dw, db)."""
    return row_stat(got.reshape(-1, 1), ref.reshape(-1, 1), mag.reshape(-1, 1))


def norm_stats(got, ref, mag):
    """statistic per result present (not None) in ``got``; dw / db per column."""
    out = {}
    for n in ("y", "h", "dx", "dres"):
        if got.get(n) is not None:
            k = "dx" if n == "dres" else n
            out[n] = row_stat(got[n], ref[k], mag[k])
    for n in ("dw", "db", "mean", "rstd"):
        if got.get(n) is not None:
            out[n] = col_stat(got[n], ref[n], mag[n])
    return out


def norm_bounds(dtype, N):
    b = {n: sum_bound(dtype) for n in ("y", "h", "dx", "dres")}
    b.update(dw=acc_bound(dtype, N), db=acc_bound(dtype, N), mean=F32_SUM_BOUND, rstd=F32_SUM_BOUND)
    return b


def global_rel(a, b):
    """The whole-tensor ratio of tests/test_kernels_gpu.py (``_rel``), kept here to show what it misses."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()
