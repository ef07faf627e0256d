"""The optimizer kernels (optimizer.hip, optim_ext.hip) against the per-element float64
oracle (tests/optim_oracle.py): every launch arm of AdamW (8-wide body + 4-wide tail, the
4-wide kernel alone behind a pointer that is not 16 B-aligned, PA_ADAMW_MODE 0 and 2 in
child processes), momentum / SGD through both entry points, the multi-tensor table, sumsq /
clip_coef / fold_grad and the eight optim_ext updates, at the smallest sizes where each piece
of index arithmetic exists and at the sizes where the grid stride wraps.

Every device buffer is a window into a larger allocation with 64 guard elements of a fixed
bit pattern (a NaN) on each side; the guards must be bit-identical afterwards, inputs must
be unchanged, and each step's reference is computed from the state the kernel itself left.
The module prints the worst statistic per operation, dtype and output when it finishes (the
table kept in optim_oracle's docstring; run with -s to see it)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import optim_oracle as O  # noqa: E402
from paddle_amd.ops import _native as N  # noqa: E402
from paddle_amd.ops import oplib, optim  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
GUARD = 64
PAT = {F32: (torch.int32, 0x7FC1A5A5), BF16: (torch.int16, 0x7FC1)}
WORST = {}


def _dn(dt):
    return {F32: "fp32", BF16: "bf16", None: "none"}[dt]


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nworst statistic per operation, dtypes and output")
    for k in sorted(WORST):
        print("    %-22s %-12s " % k + "  ".join(f"{n} {s:.2e}" for n, s in sorted(WORST[k].items())))


def _record(op, dts, name, s, b, what, fails):
    w = WORST.setdefault((op, dts), {})
    w[name] = max(w.get(name, 0.0), s)
    if not s <= b:
        fails.append((op, dts, what, name, s, b))


def _finish(fails):
    assert not fails, (len(fails), fails[:6])


class Win:
    """A CPU tensor as a device window: GUARD elements of a fixed bit pattern before and after
    it (``off`` more before it, to move the window off 16 B alignment)."""

    def __init__(self, t, off=0):
        it, pat = PAT[t.dtype]
        self.n, self.lo, self.pat = t.numel(), GUARD + off, pat
        self.parent = torch.empty(self.lo + self.n + GUARD, dtype=t.dtype, device=dev)
        self.bits = self.parent.view(it)
        self.bits.fill_(pat)
        self.v = self.parent[self.lo:self.lo + self.n]
        self.v.copy_(t)

    def intact(self):
        b = self.bits
        return bool((b[:self.lo] == self.pat).all()) and bool((b[self.lo + self.n:] == self.pat).all())

    def cpu(self):
        return self.v.cpu()


def scal(x):
    return Win(torch.tensor([x], dtype=F32))


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(PAT[a.dtype][0]), b.view(PAT[b.dtype][0]))


def _off(dt, off):
    """``off`` fp32 elements in elements of ``dt``."""
    return off * (2 if dt == BF16 else 1)


# ====================================================================== AdamW
def run_adamw(n, gd, pd, de, flags, profile, off, steps, fails, op="adamw", digest=None):
    p, g, m, v = O.adamw_inputs(profile, n, gd)
    wp, wm, wv, wg = Win(p, off), Win(m, off), Win(v, off), Win(g, _off(gd, off))
    wo = Win(torch.zeros(n, dtype=pd), _off(pd, off)) if pd is not None else None
    what = (n, de, flags, profile, off)
    dts = f"{_dn(gd)}/{_dn(pd)}"
    for step in steps:
        kw, devs = O.adamw_scalars(flags, step)
        dw = {k: (scal(x) if x is not None else None) for k, x in devs.items()}
        p0, m0, v0 = wp.cpu(), wm.cpu(), wv.cpu()
        ref, mag = O.adamw_reference(p0, g, m0, v0, decay_end=de, **kw, **devs)
        optim.adamw_flat(wp.v, wg.v, wm.v, wv.v, param_out=wo.v if wo else None, decay_end=de,
                         **kw, **{k: (w.v if w is not None else None) for k, w in dw.items()})
        got = dict(p=wp.cpu(), m=wm.cpu(), v=wv.cpu())
        for name in ("p", "m", "v"):
            _record(op, dts, name, O.elem_stat(got[name], ref[name], mag[name]), O.bound("adamw", name), what, fails)
        if wo is not None:
            po = wo.cpu()
            if not _same_bits(po, got["p"].to(pd)):  # round-to-nearest-even of the kernel's own fp32 result
                fails.append((op, dts, what, "param_out is not the rounding of param"))
            if pd == BF16:  # and the store against the oracle: one bf16 rounding on top of the fp32 bound
                _record(op, dts, "param_out", O.elem_stat(po, ref["p"], mag["p"]), O.bound("adamw", "p", BF16), what, fails)
            if digest is not None:
                digest.update(po.view(PAT[pd][0]).numpy().tobytes())
        if digest is not None:
            for name in ("p", "m", "v"):
                digest.update(got[name].numpy().tobytes())
        wins = [wp, wm, wv, wg] + ([wo] if wo else []) + [w for w in dw.values() if w is not None]
        if not all(w.intact() for w in wins):
            fails.append((op, dts, what, "guard changed"))
        if not _same_bits(wg.cpu(), g) or any(w is not None and w.cpu().item() != devs[k] for k, w in dw.items()):
            fails.append((op, dts, what, "input changed"))


@pytest.mark.parametrize("gd", O.GDTYPES, ids=_dn)
@pytest.mark.parametrize("pd", O.PDTYPES, ids=_dn)
def test_adamw_small(gd, pd):
    """Every size x decay_end x dtype pair, three steps carrying state, 16 B-aligned windows (8-wide
    body + 4-wide tail) and windows offset by one fp32 element (the 4-wide kernel alone)."""
    fails = []
    for n, g_, p_, de, flags, profile in O.adamw_cases():
        if (g_, p_) == (gd, pd):
            for off in (0, 1):
                run_adamw(n, gd, pd, de, flags, profile, off, (1, 2, 3), fails, op="adamw" if off == 0 else "adamw 4-wide")
    _finish(fails)


def test_adamw_profiles_and_flags():
    """Every profile x flag set at n = 2055 (the combinations the rotation above does not meet)."""
    fails = []
    for profile in O.PROFILES:
        for flags in O.ADAMW_FLAGS:
            run_adamw(2055, BF16, BF16, 1027, flags, profile, 0, (1, 2), fails)
    _finish(fails)


def test_adamw_4wide_stride_wraps():
    fails = []
    n = O.ADAMW_N4_WRAP
    run_adamw(n, BF16, BF16, n // 2 + 1, O.ADAMW_FLAGS[4], "mixed", 1, (1,), fails, op="adamw 4-wide")
    _finish(fails)


def test_adamw_8wide_stride_wraps_with_tail():
    fails = []
    n = O.ADAMW_N8_WRAP
    run_adamw(n, BF16, BF16, n - 2, O.ADAMW_FLAGS[4], "mixed", 0, (1,), fails)
    _finish(fails)


def reduced_table(op):
    """The table the PA_ADAMW_MODE children run: (fails, sha256 of every output, worst)."""
    fails, h = [], hashlib.sha256()
    for n, gd, pd, de, flags, profile in O.adamw_cases((7, 8, 9, 16, 2055)):
        run_adamw(n, gd, pd, de, flags, profile, 0, (1,), fails, op=op, digest=h)
    worst = {}
    for (o, _dts), w in WORST.items():
        if o == op:
            for k, s in w.items():
                worst[k] = max(worst.get(k, 0.0), s)
    return fails, h.hexdigest(), worst


def _child(mode):
    env = dict(os.environ, PA_ADAMW_MODE=str(mode))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(mode)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_adamw_mode0_child():
    """PA_ADAMW_MODE=0: the 4-wide kernel on aligned pointers, in a fresh process."""
    out = _child(0)
    assert not out["fails"], out["fails"][:6]
    WORST[("adamw mode 0", "all")] = out["worst"]


def test_adamw_mode2_child_matches_mode1():
    """PA_ADAMW_MODE=2 differs from the default only in the cache hint: the same bits."""
    out = _child(2)
    assert not out["fails"], out["fails"][:6]
    WORST[("adamw mode 2", "all")] = out["worst"]
    fails, digest, _ = reduced_table("adamw reduced")
    WORST.pop(("adamw reduced", "all"), None)
    for k in [k for k in WORST if k[0] == "adamw reduced"]:
        WORST.pop(k)
    _finish(fails)
    assert out["digest"] == digest


# ====================================================================== momentum / SGD
def run_momentum(n, gd, pd, flags, profile, entry, fails):
    has_vel, nest, wd, gs, lr_dev = flags
    p, g, vel = O.momentum_inputs(profile, n, gd, pd)
    vel = vel if has_vel else None
    wp, wg = Win(p), Win(g)
    wv = Win(vel) if has_vel else None
    wl = scal(O.MOM_HP["lr"]) if lr_dev else None
    lr = O.MOM_HP["lr"] * (3.0 if lr_dev else 1.0)
    kw = dict(lr=lr, mu=O.MOM_HP["mu"], nesterov=nest, weight_decay=wd, grad_scale=gs)
    ref, mag = O.momentum_reference(p, g, vel, lr_tensor=O.f32(O.MOM_HP["lr"]) if lr_dev else None, **kw)
    if entry == "pa_momentum_p":
        optim.momentum_flat(wp.v, wg.v, wv.v if wv else None, lr_tensor=wl.v if wl else None, **kw)
    else:
        N.call("pa_momentum", N.dt(wg.v), N.ptr(wp.v), N.ptr(wg.v), N.ptr(wv.v if wv else None), n, float(lr),
               N.ptr(wl.v if wl else None), float(kw["mu"]), int(nest), float(wd), float(gs), N.stream())
    what, dts = (n, flags, profile), f"{_dn(gd)}/{_dn(pd)}"
    got = wp.cpu()
    b = O.bound("momentum", "p")
    if pd == BF16:
        if not O.bf16_store_ok(got, ref["p"], mag["p"], b):
            fails.append((entry, dts, what, "bf16 parameter is not a rounding of a value within the fp32 bound"))
        _record(entry, dts, "p", O.elem_stat(got, ref["p"], mag["p"]), O.bound("momentum", "p", BF16), what, fails)
    else:
        _record(entry, dts, "p", O.elem_stat(got, ref["p"], mag["p"]), b, what, fails)
    if has_vel:
        _record(entry, dts, "vel", O.elem_stat(wv.cpu(), ref["vel"], mag["vel"]), O.bound("momentum", "vel"), what, fails)
    if not all(w.intact() for w in (wp, wg, wv, wl) if w is not None) or not _same_bits(wg.cpu(), g):
        fails.append((entry, dts, what, "guard or input changed"))


@pytest.mark.parametrize("entry", ["pa_momentum_p", "pa_momentum"])
def test_momentum(entry):
    fails, k = [], 0
    for n in O.MOM_N:
        for gd in O.GDTYPES:
            for pd in (O.GDTYPES if entry == "pa_momentum_p" else (F32,)):
                for flags in O.MOM_FLAGS:
                    run_momentum(n, gd, pd, flags, O.PROFILES[k % len(O.PROFILES)], entry, fails)
                    k += 1
    _finish(fails)


def _multi_step(mm, wins, ent, kw, fails, what):
    """One MomentumMulti step on the windows, checked against the oracle at the windows' state."""
    cur = [(wt.cpu(), None, wg.cpu(), wv.cpu(), wd, ls) for (wt, wo, wg, wv), (_t, _o, _g, _v, wd, ls) in zip(wins, ent)]
    refs = O.multi_reference(cur, **kw)
    mm.step([(wt.v, wo.v if wo else None, wg.v, wv.v, e[4], e[5]) for (wt, wo, wg, wv), e in zip(wins, ent)], **kw)
    for i, ((wt, wo, wg, wv), (ref, mag)) in enumerate(zip(wins, refs)):
        tdt = wt.v.dtype
        dts, w = f"{_dn(wg.v.dtype)}/{_dn(tdt)}", what + (i, wt.n)
        got = wt.cpu()
        if tdt == BF16:
            if not O.bf16_store_ok(got, ref["p"], mag["p"], O.bound("momentum", "p")):
                fails.append(("momentum_multi", dts, w, "bf16 target is not a rounding of a value within the fp32 bound"))
            _record("momentum_multi", dts, "p", O.elem_stat(got, ref["p"], mag["p"]), O.bound("momentum", "p", BF16), w, fails)
        else:
            _record("momentum_multi", dts, "p", O.elem_stat(got, ref["p"], mag["p"]), O.bound("momentum", "p"), w, fails)
        _record("momentum_multi", dts, "vel", O.elem_stat(wv.cpu(), ref["vel"], mag["vel"]), O.bound("momentum", "vel"), w, fails)
        if wo is not None and not _same_bits(wo.cpu(), got.to(wo.v.dtype)):
            fails.append(("momentum_multi", dts, w, "second output is not the rounding of the target"))
        if wo is not None and wo.v.dtype == BF16:
            _record("momentum_multi", dts, "out_bf16", O.elem_stat(wo.cpu(), ref["p"], mag["p"]),
                    O.bound("momentum", "p", BF16), w, fails)
        if not all(x.intact() for x in (wt, wo, wg, wv) if x is not None) or not _same_bits(wg.cpu(), cur[i][2]):
            fails.append(("momentum_multi", dts, w, "guard or input changed"))


@pytest.mark.parametrize("second", [True, False], ids=["second_out", "no_second_out"])
def test_momentum_multi(second):
    fails = []
    ent = O.multi_entries(second=second)
    wins = [(Win(t), Win(o) if o is not None else None, Win(g), Win(v)) for t, o, g, v, _wd, _ls in ent]
    kw = dict(lr=O.MOM_HP["lr"], mu=O.MOM_HP["mu"], nesterov=second, grad_scale=0.5)
    mm = optim.MomentumMulti()
    _multi_step(mm, wins, ent, kw, fails, ("first",))
    key = mm._key
    _multi_step(mm, wins, ent, kw, fails, ("cached table",))
    assert mm._key is key
    j = O.MULTI_LENS.index(4097)
    wins[j] = wins[j][:2] + (Win(ent[j][2]),) + wins[j][3:]  # one gradient reallocated: the table is uploaded again
    _multi_step(mm, wins, ent, kw, fails, ("re-uploaded table",))
    assert mm._key != key
    # one tensor alone: the binary search with nt = 1
    _multi_step(optim.MomentumMulti(), wins[j:j + 1], ent[j:j + 1], kw, fails, ("nt = 1",))
    lrw = scal(O.MOM_HP["lr"])
    kw_dev = dict(kw, lr=O.MOM_HP["lr"] * 3)
    cur_kw = dict(kw_dev, lr_tensor=lrw.v)
    # device lr: the oracle gets its value, the kernel the tensor
    cur = [(wt.cpu(), None, wg.cpu(), wv.cpu(), e[4], e[5]) for (wt, wo, wg, wv), e in zip(wins, ent)]
    refs = O.multi_reference(cur, **dict(kw_dev, lr_tensor=O.f32(O.MOM_HP["lr"])))
    optim.MomentumMulti().step([(wt.v, wo.v if wo else None, wg.v, wv.v, e[4], e[5]) for (wt, wo, wg, wv), e in zip(wins, ent)],
                               **cur_kw)
    for (wt, wo, wg, wv), (ref, mag) in zip(wins, refs):
        s = O.elem_stat(wv.cpu(), ref["vel"], mag["vel"])
        _record("momentum_multi", "device lr", "vel", s, O.bound("momentum", "vel"), ("device lr", wt.n), fails)
        if wt.v.dtype == F32:
            _record("momentum_multi", "device lr", "p", O.elem_stat(wt.cpu(), ref["p"], mag["p"]), O.bound("momentum", "p"),
                    ("device lr", wt.n), fails)
    assert lrw.intact()
    _finish(fails)


# ====================================================================== sumsq / clip_coef / fold_grad
def test_sumsq():
    fails = []
    for n in O.SUMSQ_N:
        for dt in O.GDTYPES:
            for off in ((0, 1) if n in (1, 9, O.SUMSQ_N[-1]) else (0,)):  # off: the scalar route of a misaligned pointer
                x = torch.randn(n, generator=O._gen(n, 6)).to(dt)
                wx, wo = Win(x, _off(dt, off)), scal(3.25)
                assert (wx.v.data_ptr() % 16 == 0) == (off == 0)
                ref, mag = O.sumsq_reference(x, 3.25)
                out = optim.sumsq(wx.v, wo.v)
                assert out.data_ptr() == wo.v.data_ptr()
                got = wo.cpu().item()
                what = (n, off)
                if n == 0:
                    if got != 3.25:
                        fails.append(("sumsq", _dn(dt), what, "out changed with n = 0"))
                else:
                    _record("sumsq" if off == 0 else "sumsq misaligned", _dn(dt), "out", abs(got - ref) / mag,
                            O.sumsq_bound(n, off == 0), what, fails)
                if not (wx.intact() and wo.intact() and _same_bits(wx.cpu(), x)):
                    fails.append(("sumsq", _dn(dt), what, "guard or input changed"))
    _finish(fails)


AT_THRESHOLD = float(np.float32(1) + np.float32(1e-6))
CLIP_CASES = ((4.0, 0.5, 2.0, "below"), (4.0, 0.5, 0.3, "above"), (4.0, 0.5, AT_THRESHOLD, "at"), (123.456, 0.125, 1.0, "above"))


def test_clip_coef():
    fails = []
    for ss, ns, mx, kind in CLIP_CASES:
        ws, wc = scal(ss), scal(-1.0)
        N.call("pa_clip_coef", N.ptr(ws.v), float(ns), float(mx), N.ptr(wc.v), N.stream())
        got = wc.cpu().item()
        ref, mag = O.clip_coef_reference(ss, ns, mx)
        _record("clip_coef", "fp32", "coef", abs(got - ref) / mag, O.bound("clip_coef", "coef"), (ss, ns, mx), fails)
        if kind in ("below", "at"):
            assert got == 1.0, (kind, got)
        else:
            assert got < 1.0
        assert ws.intact() and wc.intact() and ws.cpu().item() == O.f32(ss)
    _finish(fails)


def test_clip_chain():
    """sumsq -> pa_clip_coef -> adamw_flat(grad_scale_tensor=coef) against the same chain in float64."""
    fails = []
    n = 2055
    p, g, m, v = O.adamw_inputs("large", n, BF16)
    wp, wg, wm, wv, wss, wc = Win(p), Win(g), Win(m), Win(v), scal(0.0), scal(-1.0)
    optim.sumsq(wg.v, wss.v)
    N.call("pa_clip_coef", N.ptr(wss.v), 1.0, 1.0, N.ptr(wc.v), N.stream())
    hp = O.ADAMW_HP
    optim.adamw_flat(wp.v, wg.v, wm.v, wv.v, step=1, grad_scale_tensor=wc.v, **hp)
    ss_ref, ss_mag = O.sumsq_reference(g)
    _record("clip chain", "bf16", "sumsq", abs(wss.cpu().item() - ss_ref) / ss_mag, O.sumsq_bound(n), n, fails)
    c_ref, _ = O.clip_coef_reference(wss.cpu().item(), 1.0, 1.0)
    assert c_ref < 1e-3  # the clip is active
    _record("clip chain", "bf16", "coef", abs(wc.cpu().item() - c_ref) / c_ref, O.bound("clip_coef", "coef"), n, fails)
    # the end-to-end chain in float64: the coefficient's own error (sumsq, then clip_coef) scales every gg
    ref, mag = O.adamw_reference(p, g, m, v, step=1, grad_scale_tensor=wc.cpu().item(), **hp)
    for name, w in (("p", wp), ("m", wm), ("v", wv)):
        _record("clip chain", "bf16", name, O.elem_stat(w.cpu(), ref[name], mag[name]), O.bound("adamw", name), n, fails)
    c64 = min(1.0, 1.0 / (ss_ref ** 0.5 + 1e-6))
    assert abs(wc.cpu().item() - c64) <= (O.sumsq_bound(n) + O.bound("clip_coef", "coef")) * c64
    assert all(w.intact() for w in (wp, wg, wm, wv, wss, wc))
    _finish(fails)


def test_fold_grad():
    fails = []
    for n in (1, 257, O.MOM_N[-1]):
        for dt in O.GDTYPES:
            for fresh in (0, 1):
                dst, g = torch.randn(n, generator=O._gen(n, 7)), torch.randn(n, generator=O._gen(n, 8)).to(dt)
                wd, wg = Win(dst), Win(g)
                if fresh:
                    wd.bits[wd.lo:wd.lo + n] = PAT[F32][1]  # a fresh fold must not read what was there
                N.call("pa_fold_grad", N.dt(wg.v), N.ptr(wd.v), N.ptr(wg.v), n, fresh, N.stream())
                ref, mag = O.fold_grad_reference(dst, g, fresh)
                _record("fold_grad", _dn(dt), "fresh" if fresh else "accumulate", O.elem_stat(wd.cpu(), ref, mag),
                        O.bound("fold_grad", "dst"), (n, fresh), fails)
                if not (wd.intact() and wg.intact() and _same_bits(wg.cpu(), g)):
                    fails.append(("fold_grad", _dn(dt), (n, fresh), "guard or input changed"))
    _finish(fails)


# ====================================================================== optim_ext
@pytest.mark.parametrize("kind", O.EXT_KINDS)
def test_optim_ext(kind):
    fails = []
    kernel, states = O.EXT_KERNEL[kind]
    for n in O.EXT_N:
        d = O.ext_inputs(kind, n)
        w = {k: Win(t) for k, t in d.items()}
        ref, mag = O.ext_reference(kind, d)
        r = oplib.opt_update_(kernel, w["p"].v, w["g"].v, [w[s].v if s is not None else None for s in states],
                              None if kind == "adadelta" else O.EXT_LR, **O.EXT_HP[kind])
        assert r is not None
        b = O.ext_bounds(kind, n)
        for name in ref:
            _record(kind, "fp32", name, O.elem_stat(w[name].cpu(), ref[name], mag[name]), b[name], n, fails)
        if not all(x.intact() for x in w.values()) or not _same_bits(w["g"].cpu(), d["g"]):
            fails.append((kind, "fp32", n, "guard or input changed"))
    _finish(fails)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    f, dg, worst = reduced_table("adamw mode " + sys.argv[2])
    print(json.dumps(dict(fails=[str(x) for x in f], digest=dg, worst=worst)))
