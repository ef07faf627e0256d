"""Per-element float64 oracle for the optimizer kernels (CPU only, plain torch / numpy):
AdamW, momentum / Nesterov / SGD, the multi-tensor momentum table, sum of squares, clip
coefficient, gradient fold (csrc/kernels/optimizer.hip) and Adamax, decayed Adagrad,
Adadelta, RMSProp, FTRL, proximal GD / Adagrad and LARS (csrc/kernels/optim_ext.hip).

The convention is the row oracle's (tests/row_oracle.py).  Every ``*_reference`` takes the
rounded inputs the kernel gets (fp32 / bf16 tensors, scalars rounded to fp32 the way the
launcher passes them) and returns each output in float64, and next to it a **magnitude**:
the same expression with every term replaced by its absolute value.  The work is
elementwise, so ``elem_stat`` is max |got - ref| / mag over the elements (no row norm):
one wrong element cannot hide behind the others.  Where a quantity goes through a
nonlinear step after a cancellation (the centered RMSProp denominator s - a^2 + eps, the
Adadelta ratio), its condition factor mag / |value| multiplies the downstream magnitude.

``*_emulated`` is the same formula in float32, one rounding per operation and one to the
storage dtype per kernel output.  It is the yardstick the bounds are checked against on
the CPU (``EMU_MARGIN``), never an expected value.

Bounds (derived, not tuned).  u = 2^-24 is the fp32 unit roundoff; a bound is
``2 * count * u``: ``count`` is the first-order sum of the roundings below as the kernel
evaluates the formula without contraction, and the factor 2 covers second-order terms and
an evaluation that differs only in where it rounds (the build contracts a * b + c to an
fma: -ffp-contract=fast).  The build has no fast-math flag, so ``/`` and ``sqrtf`` are
correctly rounded (hipcc's default): 1 u and, after halving the argument's error, 0.5 u.
``rsqrtf`` is taken at 2 ulp = 4 u.  1 - beta is exact for beta in [0.5, 1] (Sterbenz)
but is counted as 1.

    adamw     m   5   gg = g gs (1), 1 - b1 (1), its product (1), b1 m (1), the sum (1)
              v   7   gg twice (2), 1 - b2 (1), two products (2), b2 v (1), the sum (1)
              p  21   p (1 - lr wd): 3.  step = lr / c1: 2, m: 5 (on its magnitude), step m: 1,
                      sqrt(v): 4, rc2 = rsqrtf(c2): 4.5, their product: 1, + eps_: 1,
                      the division: 1; the final subtraction: 1
    momentum  vel 4   g gs (1), wd p (1), their sum (1); mu vel and the sum are no worse
              p   9   Nesterov: gg (3), mu v (5), sum (1), lr lr_scale (1), product (1) ...
    sumsq        S    S = terms per lane + 1 (the square) + 6 shuffle steps + 4 wave partials
                      + ceil(grid / 256) partials per lane of the second pass + 6 + 4 + 1
                      (``sumsq_count``: every term is positive, so the error is relative)
    clip_coef    4    sqrt (0.5), norm_scale (1), + 1e-6 (1), division (1)
    fold_grad    1
    adamax    m 4, u 2, p 11      decayed_adagrad  m 5, p 7
    adadelta  ag 5, au 16, p 7    rmsprop  ms 5, mg 4, mom 9, p 10 (both forms)
    ftrl -0.5 sq 2, lin 7, p 13   proximal  m 2, p 12 (both forms)
    lars      v L + 12, p L + 13  L = terms per lane + 1 + 6 + 4 + grid: the block partials
                      meet in float atomics in any order (``lars_count``)

A bf16 store adds one bf16 rounding to the fp32 bound (``bf16_bound``).  In the unit the
attention and row oracles count in, u = 2^-9 (``U16``), one round-to-nearest-even to bf16's 8
significant bits is 2 u: half a spacing of 2^-7 of the binade's lower end, i.e. up to 2^-8 of
a value just above a power of two (row_oracle's 4 u is two such roundings).  The rounding
is sharp, so EMU_MARGIN applies to the fp32 part only; the CPU emulation reaches 3.7e-03 of
the 3.9e-03.  ``bf16_store_ok`` is the same check without the slack of the binade: the store
must be the rounding of some value within the fp32 bound of the oracle.  Where the kernel's
own fp32 result is observable too (AdamW ``param_out`` against
``param``, the multi-tensor second output against an fp32 target) the store must equal the
round-to-nearest-even of that result bit for bit.

FTRL with a general ``lr_power`` goes through the device ``powf``, which is not libm's, so
its bound is measured, not derived: the worst ``elem_stat`` of the fp32 CPU emulation
(torch.pow in float32) over every size and seed the tests use is
lin 1.01e-07, p 1.88e-07 (sq is the derived 2 count); with a factor 4 for a different but
equally accurate ``powf`` the bounds are ``FTRL_POW_BOUND`` = lin 4.04e-07, p 7.52e-07.
The MI355X measures lin 1.00e-07, p 1.87e-07 (table below).

Worst statistics measured on the MI355X (tests/test_optim_kernels_oracle_gpu.py):

    adadelta               fp32         ag 1.28e-07  au 1.85e-07  p 1.56e-07
    adamax                 fp32         m 1.13e-07  p 2.14e-07  u 5.95e-08
    adamw                  bf16/bf16    m 1.43e-07  p 2.17e-07  param_out 3.89e-03  v 2.24e-07
    adamw                  bf16/fp32    m 1.14e-07  p 7.60e-08  v 2.24e-07
    adamw                  bf16/none    m 1.19e-07  p 8.47e-08  v 2.10e-07
    adamw                  fp32/bf16    m 1.11e-07  p 1.12e-07  param_out 3.89e-03  v 1.41e-07
    adamw                  fp32/fp32    m 1.31e-07  p 1.07e-07  v 1.74e-07
    adamw                  fp32/none    m 1.22e-07  p 7.60e-08  v 1.74e-07
    adamw 4-wide           bf16/bf16    m 1.16e-07  p 1.80e-07  param_out 3.89e-03  v 1.85e-07
    adamw 4-wide           bf16/fp32    m 1.09e-07  p 7.60e-08  v 2.24e-07
    adamw 4-wide           bf16/none    m 1.06e-07  p 9.31e-08  v 2.10e-07
    adamw 4-wide           fp32/bf16    m 1.10e-07  p 1.12e-07  param_out 3.89e-03  v 1.41e-07
    adamw 4-wide           fp32/fp32    m 1.10e-07  p 1.07e-07  v 1.74e-07
    adamw 4-wide           fp32/none    m 1.13e-07  p 7.60e-08  v 1.74e-07
    adamw mode 0           all          m 1.08e-07  p 7.50e-08  param_out 3.89e-03  v 1.76e-07
    adamw mode 2           all          m 1.22e-07  p 7.50e-08  param_out 3.89e-03  v 1.76e-07
    clip chain             bf16         coef 7.92e-08  m 8.91e-08  p 7.29e-08  sumsq 1.27e-07  v 5.85e-08
    clip_coef              fp32         coef 4.84e-08
    decayed_adagrad        fp32         m 1.43e-07  p 1.79e-07
    fold_grad              bf16         accumulate 5.96e-08  fresh 0.00e+00
    fold_grad              fp32         accumulate 5.96e-08  fresh 0.00e+00
    ftrl                   fp32         lin 1.06e-07  p 1.88e-07  sq 5.95e-08
    ftrl_pow               fp32         lin 1.00e-07  p 1.87e-07  sq 5.96e-08
    lars                   fp32         p 1.51e-07  v 5.21e-07
    momentum_multi         bf16/bf16    p 3.84e-03  vel 9.18e-08
    momentum_multi         bf16/fp32    out_bf16 1.09e-03  p 2.18e-08  vel 3.34e-08
    momentum_multi         device lr    p 1.25e-07  vel 8.64e-08
    momentum_multi         fp32/bf16    p 3.84e-03  vel 9.59e-08
    momentum_multi         fp32/fp32    out_bf16 3.80e-03  p 1.23e-07  vel 9.64e-08
    pa_momentum            bf16/fp32    p 1.44e-07  vel 1.08e-07
    pa_momentum            fp32/fp32    p 1.37e-07  vel 1.64e-07
    pa_momentum_p          bf16/bf16    p 3.89e-03  vel 1.05e-07
    pa_momentum_p          bf16/fp32    p 1.42e-07  vel 1.35e-07
    pa_momentum_p          fp32/bf16    p 3.89e-03  vel 1.58e-07
    pa_momentum_p          fp32/fp32    p 1.62e-07  vel 1.52e-07
    proximal_adagrad       fp32         m 5.95e-08  p 2.04e-07
    proximal_gd            fp32         p 1.47e-07
    rmsprop                fp32         mom 1.69e-07  ms 1.16e-07  p 1.28e-07
    rmsprop_centered       fp32         mg 1.11e-07  mom 1.86e-07  ms 1.15e-07  p 1.30e-07
    sumsq                  bf16         out 6.22e-08
    sumsq                  fp32         out 5.12e-08
    sumsq misaligned       bf16         out 2.54e-09
    sumsq misaligned       fp32         out 4.14e-08

    ("adamw 4-wide": windows offset by one fp32 element; "mode 0" / "mode 2": the PA_ADAMW_MODE
    children; a bf16 output's statistic is the store against the oracle under ``bf16_bound``.)
"""
import math

import numpy as np
import torch

from row_oracle import global_rel  # noqa: F401  (re-exported: what test_kernels_gpu._rel sees)

U32 = 2.0 ** -24
U16 = 2.0 ** -9              # the unit bf16 bounds are counted in (attn_oracle.U)
BF16_ROUNDING = 2 * U16      # one round-to-nearest-even to bf16, relative to the value
EMU_MARGIN = 2.0  # the emulation must meet every bound with this factor to spare

COUNTS = {
    "adamw": dict(m=5, v=7, p=21),
    "momentum": dict(vel=4, p=9),
    "clip_coef": dict(coef=4),
    "fold_grad": dict(dst=1),
    "adamax": dict(m=4, u=2, p=11),
    "decayed_adagrad": dict(m=5, p=7),
    "adadelta": dict(ag=5, au=16, p=7),
    "rmsprop": dict(ms=5, mg=4, mom=9, p=10),
    "ftrl": dict(sq=2, lin=7, p=13),
    "proximal": dict(m=2, p=12),
}
# measured on the CPU emulation (module docstring), times 4
FTRL_POW_EMU = dict(lin=1.01e-07, p=1.88e-07)
FTRL_POW_BOUND = {k: 4 * v for k, v in FTRL_POW_EMU.items()}

PROFILES = ("flat", "tiny", "large", "mixed", "zeros")

# ---------------------------------------------------------------- launch constants (optimizer.hip, common.h)
BLOCK = 256
GRID_CAP = 2048      # stream_grid
GRID8_CAP = 8192     # adamw8_kernel
MCHUNK = 4096        # momentum_multi_kernel

# ---------------------------------------------------------------- the GPU test's sizes (the CPU test walks the same lists)
ADAMW_N = (1, 3, 4, 7, 8, 9, 15, 16, 2055)
ADAMW_N4_WRAP = GRID_CAP * BLOCK * 4 + 13             # 4-wide arm: the grid stride wraps
ADAMW_N8_WRAP = GRID8_CAP * BLOCK * 8 + 8 * 300 + 5   # 8-wide arm: wraps, and leaves a tail
MOM_N = (1, 255, 256, 257, GRID_CAP * BLOCK + 77)
MULTI_LENS = (1, 4095, 4096, 4097, 3 * 4096, 13)
SUMSQ_N = (0, 1, 7, 8, 9, GRID_CAP * BLOCK * 8 + 5)
EXT_N = (1, 91, 255, 256, 257, GRID_CAP * BLOCK + 77)
EXT_KINDS = ("adamax", "decayed_adagrad", "adadelta", "rmsprop", "rmsprop_centered", "ftrl", "ftrl_pow",
             "proximal_gd", "proximal_adagrad", "lars")
GDTYPES = (torch.float32, torch.bfloat16)
PDTYPES = (torch.float32, torch.bfloat16, None)

ADAMW_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
# (lr on the device, beta-pow on the device, grad_scale_tensor value or None, lr_t_eps, grad_scale)
ADAMW_FLAGS = ((False, False, None, False, 1.0), (True, False, None, False, 1.0), (False, True, None, True, 1.0),
               (False, False, 0.37, False, 0.5), (True, True, 0.37, True, 1.0), (False, False, None, True, 2.0),
               (False, True, 1.7, False, 1.0))
# (velocity, nesterov, wd, grad_scale, lr on the device)
MOM_FLAGS = ((True, False, 0.0, 1.0, False), (True, True, 0.01, 1.0, False), (False, False, 0.01, 0.5, True),
             (True, True, 0.0, 0.25, True), (False, False, 0.0, 1.0, False), (True, False, 0.01, 2.0, True))
MOM_HP = dict(lr=0.05, mu=0.9)


def f32(x):
    """A Python scalar as the launcher passes it: rounded to fp32."""
    return float(np.float32(x))


def bf16_bound(b):
    return b + BF16_ROUNDING


def bound(op, out, dtype=torch.float32):
    b = 2 * COUNTS[op][out] * U32
    return bf16_bound(b) if dtype == torch.bfloat16 else b


def bf16_store_ok(got, ref, mag, b):
    """A bf16 store of a result that is not observable in fp32: ``got`` must be the bf16
    rounding of some value within the fp32 bound ``b`` of the oracle, i.e. lie between the
    roundings of ref - b mag and ref + b mag."""
    got, ref, mag = (t.detach().cpu().double().reshape(-1) for t in (got, ref, mag))
    lo = (ref - b * mag).float().bfloat16().double()
    hi = (ref + b * mag).float().bfloat16().double()
    return bool(((got >= lo) & (got <= hi)).all())


def elem_stat(got, ref, mag):
    """max over the elements of |got - ref| / mag; an element whose magnitude is 0 must be exact."""
    got, ref, mag = (torch.as_tensor(t).detach().cpu().double().reshape(-1) for t in (got, ref, mag))
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref).abs()
    s = torch.where(mag > 0, err / mag.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))
    return s.max().item()


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _c(t, cd):
    return None if t is None else t.detach().cpu().to(cd)


def _S(cd):
    return lambda x: torch.tensor(f32(x), dtype=cd)


def _stored(t, store):
    return t.to(store).to(t.dtype)


# ====================================================================== inputs
def profile_scale(profile, n):
    """Per-element magnitude of the gradient of a profile, float64 [n]."""
    if profile == "flat":
        return torch.ones(n, dtype=torch.float64)
    if profile == "tiny":
        return torch.full((n,), 1e-12, dtype=torch.float64)
    if profile == "large":
        return torch.full((n,), 1e4, dtype=torch.float64)
    if profile == "mixed":
        return 10.0 ** ((torch.arange(n) * 5 % 9) - 4).double()
    if profile == "zeros":
        return torch.zeros(n, dtype=torch.float64)
    raise ValueError(profile)


def adamw_inputs(profile, n, gdtype, seed=0):
    """(p, g, m, v) CPU tensors: fp32 state and a gradient in ``gdtype``; ``zeros`` is the first step."""
    g_ = _gen(seed, n, PROFILES.index(profile), 1)
    sc = profile_scale(profile, n)
    r = lambda: torch.randn(n, generator=g_, dtype=torch.float64)
    p, g, m, v = r(), r() * sc, 0.5 * r() * sc, (r() * sc) ** 2
    return p.float(), g.to(gdtype), m.float(), v.float()


def momentum_inputs(profile, n, gdtype, pdtype, seed=0):
    g_ = _gen(seed, n, PROFILES.index(profile), 2)
    sc = profile_scale(profile, n)
    r = lambda: torch.randn(n, generator=g_, dtype=torch.float64)
    p, g, vel = r(), r() * sc, 2 * r() * sc
    return p.to(pdtype), g.to(gdtype), vel.float()


def decay_ends(n):
    """The decay_end values of one size: 0, 1, mid-vector, around the 8-wide body's end, n - 1, n, None."""
    n8 = n // 8
    vals = [0, 1, (n8 // 2) * 8 + 3, n8 * 8 - 1, n8 * 8, n8 * 8 + 1, n - 1, n]
    out = []
    for d in vals:
        d = min(max(d, 0), n)
        if d not in out:
            out.append(d)
    return out + [None]


def adamw_cases(sizes=ADAMW_N):
    """(n, gdtype, pdtype, decay_end, flags, profile) over every size x dtype pair x decay_end;
    the flag sets (7) and the profiles (5) rotate through them, so each meets every dtype pair."""
    out, k = [], 0
    for gd in GDTYPES:
        for pd in PDTYPES:
            for n in sizes:
                for de in decay_ends(n):
                    out.append((n, gd, pd, de, ADAMW_FLAGS[k % len(ADAMW_FLAGS)], PROFILES[k % len(PROFILES)]))
                    k += 1
    return out


def adamw_scalars(flags, step):
    """Keyword arguments of ``adamw_flat`` for a flag set, device scalars as Python floats
    (the caller turns them into tensors).  A by-value argument that a device scalar
    overrides holds another value, so that reading the wrong one shows."""
    lr_dev, pow_dev, gst, lr_t_eps, gscale = flags
    hp = ADAMW_HP
    kw = dict(lr=hp["lr"] * (3.0 if lr_dev else 1.0), beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"],
              weight_decay=hp["weight_decay"], step=step, grad_scale=gscale, lr_t_eps=lr_t_eps)
    dev = dict(lr_tensor=f32(hp["lr"]) if lr_dev else None,
               beta1_pow=f32(hp["beta1"] ** (step + 2)) if pow_dev else None,
               beta2_pow=f32(hp["beta2"] ** (step + 2)) if pow_dev else None,
               grad_scale_tensor=f32(gst) if gst is not None else None)
    return kw, dev


# ====================================================================== AdamW
def _adamw(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step=1, decay_end=None, grad_scale=1.0,
           lr_tensor=None, beta1_pow=None, beta2_pow=None, grad_scale_tensor=None, lr_t_eps=False, cd, emu):
    p, g, m, v = (_c(t, cd) for t in (p, g, m, v))
    S = _S(cd)
    n = p.numel()
    de = n if decay_end is None else decay_end
    lr_ = S(lr_tensor if lr_tensor is not None else lr)
    # by value the wrapper passes 1 - beta^step, computed in double and rounded once
    c1 = 1 - S(beta1_pow) if beta1_pow is not None else S(1.0 - beta1 ** step)
    c2 = 1 - S(beta2_pow) if beta2_pow is not None else S(1.0 - beta2 ** step)
    gs = S(grad_scale_tensor) * S(grad_scale) if grad_scale_tensor is not None else S(grad_scale)
    b1, b2 = S(beta1), S(beta2)
    stp = lr_ / c1
    rc2 = torch.rsqrt(c2)
    eps_ = S(eps) * rc2 if lr_t_eps else S(eps)
    gg = g * gs
    mm = b1 * m + (1 - b1) * gg
    vv = b2 * v + (1 - b2) * gg * gg
    decay = torch.where(torch.arange(n) < de, S(weight_decay), torch.zeros((), dtype=cd))
    den = torch.sqrt(vv) * rc2 + eps_
    pp = p * (1 - lr_ * decay) - stp * mm / den
    out = dict(p=pp, m=mm, v=vv)
    if emu:
        return out, None
    magm = b1 * m.abs() + (1 - b1) * gg.abs()
    return out, dict(p=p.abs() * (1 + lr_ * decay) + stp * magm / den, m=magm, v=vv)


def adamw_reference(p, g, m, v, **kw):
    """float64 AdamW step.  ``lr_tensor`` / ``beta*_pow`` / ``grad_scale_tensor`` are the values
    of the device scalars (Python floats) or None.  Returns (out, mag) with p, m, v."""
    return _adamw(p, g, m, v, cd=torch.float64, emu=False, **kw)


def adamw_emulated(p, g, m, v, **kw):
    return _adamw(p, g, m, v, cd=torch.float32, emu=True, **kw)[0]


# ====================================================================== momentum / SGD
def _momentum(p, g, vel, *, lr, mu, nesterov=False, weight_decay=0.0, grad_scale=1.0, lr_tensor=None,
              lr_scale=None, cd, emu):
    store = p.dtype
    p, g, vel = (_c(t, cd) for t in (p, g, vel))
    S = _S(cd)
    lr_ = S(lr_tensor if lr_tensor is not None else lr)
    if lr_scale is not None:
        lr_ = lr_ * S(lr_scale)
    mu_, wd, gs = S(mu), S(weight_decay), S(grad_scale)
    gg = g * gs + wd * p
    magg = (g * gs).abs() + wd * p.abs()
    out, mag = {}, {}
    if vel is None:
        po = p - lr_ * gg
        mag["p"] = p.abs() + lr_ * magg
    else:
        v = mu_ * vel + gg
        magv = mu_ * vel.abs() + magg
        po = p - lr_ * ((gg + mu_ * v) if nesterov else v)
        mag["p"] = p.abs() + lr_ * ((magg + mu_ * magv) if nesterov else magv)
        out["vel"], mag["vel"] = v, magv
    out["p32"] = po                                  # before the store's rounding
    out["p"] = _stored(po, store) if emu else po
    return out, (None if emu else mag)


def momentum_reference(p, g, vel, **kw):
    """float64 momentum (``vel`` None: plain SGD) with L2 decay on the parameter.  Returns
    (out, mag) with p and vel; ``lr_scale``: the multi-tensor table's per-entry multiplier."""
    return _momentum(p, g, vel, cd=torch.float64, emu=False, **kw)


def momentum_emulated(p, g, vel, **kw):
    return _momentum(p, g, vel, cd=torch.float32, emu=True, **kw)[0]


def multi_reference(entries, *, lr, mu, nesterov=False, grad_scale=1.0, lr_tensor=None, _emu=False):
    """The multi-tensor table: entries of (target, out_or_None, grad, velocity, wd, lr_scale), each
    updated on its own.  Returns a list of (out, mag); the second output equals ``p``."""
    f = momentum_emulated if _emu else momentum_reference
    return [f(t, g, v, lr=lr, mu=mu, nesterov=nesterov, weight_decay=wd, grad_scale=grad_scale, lr_tensor=lr_tensor,
              lr_scale=ls) for t, _o, g, v, wd, ls in entries]


def multi_emulated(entries, **kw):
    return multi_reference(entries, _emu=True, **kw)


def multi_entries(gen_seed=0, lens=MULTI_LENS, second=True):
    """CPU tensors of a table over ``lens``: fp32 and bf16 targets alternate, an fp32 target gets
    a bf16 second output when ``second``; wd is 0 for every third entry (no_weight_decay)."""
    g_ = _gen(gen_seed, len(lens), 3)
    out = []
    for i, n in enumerate(lens):
        tdt = torch.float32 if i % 2 == 0 else torch.bfloat16
        gdt = torch.bfloat16 if i % 3 == 0 else torch.float32
        r = lambda: torch.randn(n, generator=g_, dtype=torch.float64)
        t, g, v = r().to(tdt), r().to(gdt), (2 * r()).float()
        o = torch.zeros(n, dtype=torch.bfloat16 if i % 4 == 0 else torch.float32) if (second and tdt == torch.float32) else None
        out.append((t, o, g, v, 0.0 if i % 3 == 2 else 0.01 * (i + 1), 1.0 + 0.25 * i))
    return out


# ====================================================================== sumsq / clip / fold
def _grid(work):
    return max(1, min((work + BLOCK - 1) // BLOCK, GRID_CAP))


def sumsq_count(n, aligned=True):
    """Roundings on the longest path of pa_sumsq's two passes (module docstring)."""
    if aligned:
        grid = _grid((n + 7) // 8)
        lanes = grid * BLOCK
        per_lane = 8 * (-(-(n // 8) // lanes)) + (-(-(n % 8) // lanes))
    else:
        grid = _grid(n)
        per_lane = -(-n // (grid * BLOCK))
    return per_lane + 1 + 6 + 4 + (-(-grid // BLOCK)) + 6 + 4 + 1


def sumsq_bound(n, aligned=True):
    return 2 * sumsq_count(n, aligned) * U32


def sumsq_reference(x, out0=0.0):
    """(value, mag) of out0 + sum x^2 in float64."""
    s = float((x.detach().cpu().double() ** 2).sum())
    return float(out0) + s, abs(float(out0)) + s


def _tree64(s):
    """wave_sum over rows of 64 lanes, as a pairwise tree in the array's dtype."""
    w = 64
    while w > 1:
        w //= 2
        s = s[:, :w] + s[:, w:2 * w]
    return s[:, 0]


def _block_sums(lane, grid):
    """block_sum<256> of per-lane values [grid * 256] -> [grid] (fp32)."""
    waves = _tree64(lane.reshape(-1, 64)).reshape(grid, 4)
    t = np.zeros(grid, np.float32)
    for i in range(4):
        t = t + waves[:, i]
    return t


def _lane_sums(sq, lanes):
    """Grid-stride sum of a float32 array: lane l adds elements l, l + lanes, ... in order."""
    n = sq.size
    trips = -(-n // lanes) if n else 0
    pad = np.zeros(trips * lanes, np.float32)
    pad[:n] = sq
    s = np.zeros(lanes, np.float32)
    for t in range(trips):
        s = s + pad[t * lanes:(t + 1) * lanes]
    return s


def sumsq_emulated(x, out0=0.0, aligned=True):
    """pa_sumsq in float32 with the kernel's summation shape (lane order within a wave aside)."""
    x = x.detach().cpu().float().numpy()
    n = x.size
    if n == 0:
        return f32(out0)
    sq = x * x
    if aligned:
        grid = _grid((n + 7) // 8)
        lanes = grid * BLOCK
        n8 = n // 8
        s = np.zeros(lanes, np.float32)
        trips = -(-n8 // lanes)
        body = np.zeros((trips * lanes, 8), np.float32)
        body[:n8] = sq[:n8 * 8].reshape(n8, 8)
        for t in range(trips):
            for j in range(8):
                s = s + body[t * lanes:(t + 1) * lanes, j]
        s = s + _lane_sums(sq[n8 * 8:], lanes)
    else:
        grid = _grid(n)
        s = _lane_sums(sq, grid * BLOCK)
    part = _block_sums(s, grid)
    lane2 = _lane_sums(part, BLOCK)
    tot = _block_sums(lane2, 1)[0]
    return float(np.float32(out0) + tot)


def clip_coef_reference(sumsq, norm_scale, max_norm):
    """(coef, mag): min(1, max_norm / (sqrt(sumsq) norm_scale + 1e-6)) from the fp32 scalars."""
    r = f32(max_norm) / (math.sqrt(f32(sumsq)) * f32(norm_scale) + f32(1e-6))
    c = min(1.0, r)
    return c, c


def clip_coef_emulated(sumsq, norm_scale, max_norm):
    F = np.float32
    r = F(max_norm) / (np.sqrt(F(sumsq)) * F(norm_scale) + F(1e-6))
    return float(min(F(1.0), r))


def fold_grad_reference(dst, g, fresh):
    d, g = dst.detach().cpu().double(), g.detach().cpu().double()
    if fresh:
        return g, g.abs()
    return d + g, d.abs() + g.abs()


def fold_grad_emulated(dst, g, fresh):
    return g.detach().cpu().float() if fresh else dst.detach().cpu().float() + g.detach().cpu().float()


# ====================================================================== optim_ext
EXT_HP = {
    "adamax": dict(bp1=0.9 ** 3, b1=0.9, b2=0.999, eps=1e-8),
    "decayed_adagrad": dict(decay=0.95, eps=1e-6),
    "adadelta": dict(rho=0.95, eps=1e-6),
    "rmsprop": dict(rho=0.9, mu=0.5, eps=1e-10),
    "rmsprop_centered": dict(rho=0.9, mu=0.5, eps=1e-10),
    "ftrl": dict(l1=0.2, l2=0.1, lr_power=-0.5),
    "ftrl_pow": dict(l1=0.2, l2=0.1, lr_power=-0.3),
    "proximal_gd": dict(l1=0.3, l2=0.2),
    "proximal_adagrad": dict(l1=0.3, l2=0.2),
    "lars": dict(mu=0.9, coeff=0.001, wd=0.0005),
}
EXT_LR = 0.05
# kernel kind (``opt_update_``'s) and state names of each case kind
EXT_KERNEL = {"adamax": ("adamax", ("m", "u")), "decayed_adagrad": ("decayed_adagrad", ("m",)),
              "adadelta": ("adadelta", ("ag", "au")), "rmsprop": ("rmsprop", ("ms", "mom", None)),
              "rmsprop_centered": ("rmsprop", ("ms", "mom", "mg")), "ftrl": ("ftrl", ("sq", "lin")),
              "ftrl_pow": ("ftrl", ("sq", "lin")), "proximal_gd": ("proximal", ()),
              "proximal_adagrad": ("proximal", ("m",)), "lars": ("lars", ("v",))}


def ext_inputs(kind, n, seed=0):
    """dict of fp32 CPU tensors p, g and the states of ``kind``, in the ranges for which the
    reference is well conditioned (the ranges of OPT_CASES)."""
    g_ = _gen(seed, n, EXT_KINDS.index(kind), 4)
    u = lambda lo, hi: (torch.rand(n, generator=g_, dtype=torch.float64) * (hi - lo) + lo).float()
    d = dict(p=u(-1, 1), g=u(-1, 1))
    for s in EXT_KERNEL[kind][1]:
        if s in ("m",) and kind in ("decayed_adagrad", "proximal_adagrad"):
            d[s] = u(0, 1)
        elif s in ("u", "sq"):
            d[s] = u(0.1, 1)
        elif s in ("ag", "au"):
            d[s] = u(0, 1)
        elif s == "ms":
            d[s] = u(0.5, 1)
        elif s == "mg":
            d[s] = u(-0.1, 0.1)
        elif s is not None:
            d[s] = u(-1, 1)
    return d


def lars_count(n):
    grid = _grid(n)
    return -(-n // (grid * BLOCK)) + 1 + 6 + 4 + grid


def ext_bounds(kind, n):
    k = EXT_KERNEL[kind][0]
    if kind == "lars":
        L = lars_count(n)
        return dict(v=2 * (L + 12) * U32, p=2 * (L + 13) * U32)
    b = {o: 2 * c * U32 for o, c in COUNTS[k].items()}
    if kind == "ftrl_pow":
        b.update(FTRL_POW_BOUND)
    return b


def _sqnorm_emulated(x, n_norm):
    x = x.numpy()[:n_norm]
    grid = _grid(x.size)
    part = _block_sums(_lane_sums(x * x, grid * BLOCK), grid)
    return torch.tensor(np.cumsum(part, dtype=np.float32)[-1])


def _ext(kind, d, lr, h, cd, emu, norm_n=None):
    S = _S(cd)
    t = {k: _c(v, cd) for k, v in d.items()}
    p, g = t["p"], t["g"]
    l = S(lr)
    out, mag = {}, {}
    if kind == "adamax":
        b1, b2, eps = S(h["b1"]), S(h["b2"]), S(h["eps"])
        step = l / (1 - S(h["bp1"]))
        mi = b1 * t["m"] + (1 - b1) * g
        magm = b1 * t["m"].abs() + (1 - b1) * g.abs()
        ui = torch.maximum(b2 * t["u"] + eps, g.abs())
        out.update(m=mi, u=ui, p=p - step * mi / ui)
        mag.update(m=magm, u=ui, p=p.abs() + step * magm / ui)
    elif kind == "decayed_adagrad":
        dc, eps = S(h["decay"]), S(h["eps"])
        mi = dc * t["m"] + (1 - dc) * g * g
        den = torch.sqrt(mi) + eps
        out.update(m=mi, p=p - l * g / den)
        mag.update(m=mi, p=p.abs() + (l * g).abs() / den)
    elif kind == "adadelta":
        rho, eps = S(h["rho"]), S(h["eps"])
        a = rho * t["ag"] + (1 - rho) * g * g
        num, den = t["au"] + eps, a + eps
        upd = -torch.sqrt(num / den) * g
        kap = (t["au"].abs() + eps) / num.abs() * (a.abs() + eps) / den.abs()  # condition of the ratio
        magu = upd.abs() * kap
        out.update(ag=a, au=rho * t["au"] + (1 - rho) * upd * upd, p=p + upd)
        mag.update(ag=a, au=rho * t["au"].abs() + (1 - rho) * magu * magu, p=p.abs() + magu)
    elif kind in ("rmsprop", "rmsprop_centered"):
        rho, mu, eps = S(h["rho"]), S(h["mu"]), S(h["eps"])
        s = rho * t["ms"] + (1 - rho) * g * g
        out["ms"], mag["ms"] = s, s
        if kind == "rmsprop_centered":
            a = rho * t["mg"] + (1 - rho) * g
            maga = rho * t["mg"].abs() + (1 - rho) * g.abs()
            den = s - a * a + eps
            kap = (s + maga * maga + eps) / den.abs()  # condition of s - a^2 + eps
            out["mg"], mag["mg"] = a, maga
        else:
            den, kap = s + eps, 1.0
        term = l * g / torch.sqrt(den)
        v = mu * t["mom"] + term
        magv = mu * t["mom"].abs() + term.abs() * kap
        out.update(mom=v, p=p - v)
        mag.update(mom=magv, p=p.abs() + magv)
    elif kind in ("ftrl", "ftrl_pow"):
        l1, l2, lp = S(h["l1"]), S(h["l2"]), f32(h["lr_power"])
        s0 = t["sq"]
        s1 = s0 + g * g
        if lp == -0.5:
            r1, r0 = torch.sqrt(s1), torch.sqrt(s0)
        else:
            r1, r0 = torch.pow(s1, S(-lp)), torch.pow(s0, S(-lp))
        sigma = (r1 - r0) / l
        y = r1 / l + 2 * l2
        nl = t["lin"] + g - sigma * p
        magnl = t["lin"].abs() + g.abs() + (r1 + r0) / l * p.abs()
        zero = torch.zeros((), dtype=cd)
        po = torch.where(nl.abs() > l1, (torch.minimum(torch.maximum(nl, -l1), l1) - nl) / y, zero)
        out.update(sq=s1, lin=nl, p=po)
        mag.update(sq=s1, lin=magnl, p=(magnl + l1) / y)
    elif kind in ("proximal_gd", "proximal_adagrad"):
        l1, l2 = S(h["l1"]), S(h["l2"])
        lt = l
        if kind == "proximal_adagrad":
            mi = t["m"] + g * g
            out["m"], mag["m"] = mi, mi
            lt = l / torch.sqrt(mi)
        prox = p - lt * g
        m_ = torch.clamp(prox.abs() - lt * l1, min=0)
        out["p"] = torch.copysign(m_, prox) * (prox != 0).to(cd) / (1 + lt * l2)
        mag["p"] = (p.abs() + (lt * g).abs() + lt * l1) / (1 + lt * l2)
    elif kind == "lars":
        mu, coeff, wd = S(h["mu"]), S(h["coeff"]), S(h["wd"])
        nn = p.numel() if norm_n is None else norm_n
        if emu:
            a0, a1 = _sqnorm_emulated(d["p"], nn), _sqnorm_emulated(d["g"], nn)
        else:
            a0, a1 = (p[:nn] * p[:nn]).sum(), (g[:nn] * g[:nn]).sum()
        pn, gn = torch.sqrt(a0), torch.sqrt(a1)
        local = l * coeff * pn / (gn + wd * pn + S(1e-12))
        vi = mu * t["v"] + local * (g + wd * p)
        magv = mu * t["v"].abs() + local * (g.abs() + wd * p.abs())
        out.update(v=vi, p=p - vi)
        mag.update(v=magv, p=p.abs() + magv)
    else:
        raise ValueError(kind)
    return out, (None if emu else mag)


def ext_reference(kind, d, lr=EXT_LR, h=None, _norm_n=None):
    """float64 update of one optim_ext kind on the dict of ``ext_inputs``.  Returns (out, mag)
    with p and every state written.  ``_norm_n`` builds the wrong LARS norm of the fault tests."""
    return _ext(kind, d, f32(lr), h or EXT_HP[kind], torch.float64, False, _norm_n)


def ext_emulated(kind, d, lr=EXT_LR, h=None, _norm_n=None):
    return _ext(kind, d, f32(lr), h or EXT_HP[kind], torch.float32, True, _norm_n)[0]
