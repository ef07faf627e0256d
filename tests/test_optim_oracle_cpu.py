"""The optimizer oracle (tests/optim_oracle.py) on the CPU: it agrees with the CPU paths of
paddle_amd.ops.optim and with the NumPy expectations of OPT_CASES, its float32 emulation
meets every bound with EMU_MARGIN to spare on every size and profile the GPU test uses, and
the per-element statistic catches one-element and one-path faults injected into the
emulation."""
import numpy as np
import pytest
import torch

import optim_oracle as O
from paddle_amd.ops import optim
from test_optimizer_ops_cpu import OPT_CASES

F32 = torch.float32


def _t(x):
    return None if x is None else torch.tensor([x], dtype=F32)


def _adamw_kw(flags, step, decay_end, **over):
    kw, dev = O.adamw_scalars(flags, step)
    return dict(kw, decay_end=decay_end, **dev, **over)


# ---------------------------------------------------------------- the oracle against the CPU paths
@pytest.mark.parametrize("flags", O.ADAMW_FLAGS, ids=[str(i) for i in range(len(O.ADAMW_FLAGS))])
def test_oracle_matches_adamw_flat_cpu(flags):
    for gd in O.GDTYPES:
        for pd in O.PDTYPES:
            for n, de in ((9, 4), (2055, None), (16, 0)):
                p, g, m, v = O.adamw_inputs("flat", n, gd)
                # betas that fp32 holds exactly: the CPU path forms 1 - beta in double, the kernel
                # (and the oracle) from the fp32 beta, 5e-5 apart in 1 - 0.999
                kw = _adamw_kw(flags, 2, de, beta1=0.875, beta2=1 - 2.0 ** -10)
                ref, mag = O.adamw_reference(p, g, m, v, **kw)
                po =torch.zeros(n, dtype=pd) if pd is not None else None
                tk = {k: (_t(x) if k in ("lr_tensor", "beta1_pow", "beta2_pow", "grad_scale_tensor") else x)
                      for k, x in kw.items()}
                optim.adamw_flat(p, g, m, v, param_out=po, **tk)
                for name, got in (("p", p), ("m", m), ("v", v)):
                    assert O.elem_stat(got, ref[name], mag[name]) <= O.bound("adamw", name), (name, gd, pd, n)
                if po is not None:
                    assert torch.equal(po, p.to(pd))


@pytest.mark.parametrize("flags", O.MOM_FLAGS, ids=[str(i) for i in range(len(O.MOM_FLAGS))])
def test_oracle_matches_momentum_flat_cpu(flags):
    has_vel, nest, wd, gs, lr_dev = flags
    for gd in O.GDTYPES:
        for pd in O.GDTYPES:
            p, g, vel = O.momentum_inputs("flat", 257, gd, pd)
            vel = vel if has_vel else None
            lr = O.MOM_HP["lr"]
            kw = dict(lr=lr * 3 if lr_dev else lr, mu=O.MOM_HP["mu"], nesterov=nest, weight_decay=wd, grad_scale=gs)
            ref, mag = O.momentum_reference(p, g, vel, lr_tensor=O.f32(lr) if lr_dev else None, **kw)
            optim.momentum_flat(p, g, vel, lr_tensor=_t(lr) if lr_dev else None, **kw)
            if pd == torch.bfloat16:
                assert O.bf16_store_ok(p, ref["p"], mag["p"], O.bound("momentum", "p"))
            else:
                assert O.elem_stat(p, ref["p"], mag["p"]) <= O.bound("momentum", "p")
            if has_vel:
                assert O.elem_stat(vel, ref["vel"], mag["vel"]) <= O.bound("momentum", "vel")


def test_oracle_matches_sumsq_cpu():
    for n in (0, 1, 9, 4099):
        for dt in O.GDTYPES:
            x = torch.randn(n, generator=O._gen(n, 5)).to(dt)
            out = torch.tensor([2.5])
            ref, mag = O.sumsq_reference(x, 2.5)
            optim.sumsq(x, out)
            assert abs(out.item() - ref) <= 2 * (n + 2) * O.U32 * mag


# ---------------------------------------------------------------- the oracle against OPT_CASES
_OP_KIND = {"adamax": "adamax", "decayed_adagrad": "decayed_adagrad", "adadelta": "adadelta", "rmsprop": "rmsprop",
            "ftrl": "ftrl", "proximal_gd": "proximal_gd", "proximal_adagrad": "proximal_adagrad",
            "lars_momentum": "lars"}
_IN = {"Moment": "m", "InfNorm": "u", "AvgSquaredGrad": "ag", "AvgSquaredUpdate": "au", "MeanSquare": "ms",
       "MeanGrad": "mg", "SquaredAccumulator": "sq", "LinearAccumulator": "lin", "Velocity": "v"}
_OUT = {"ParamOut": "p", "MomentOut": "m", "InfNormOut": "u", "AvgSquaredGradOut": "ag", "AvgSquaredUpdateOut": "au",
        "MeanSquareOut": "ms", "MeanGradOut": "mg", "SquaredAccumOut": "sq", "LinearAccumOut": "lin",
        "VelocityOut": "v"}


@pytest.mark.parametrize("case", [c for c in OPT_CASES if c[0] in _OP_KIND or c[0] in ("momentum", "sgd", "adam")],
                         ids=lambda c: c[0])
def test_oracle_matches_opt_cases(case):
    op, ins, outs, attrs = case
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    lr = float(ins["LearningRate"][0]) if "LearningRate" in ins else 0.0

    def close(got, want):
        np.testing.assert_allclose(got.numpy(), want.reshape(-1), rtol=2e-5, atol=2e-6)

    if op in ("momentum", "sgd"):
        vel = T(ins["Velocity"]) if op == "momentum" else None
        ref, _ = O.momentum_reference(T(ins["Param"]), T(ins["Grad"]), vel, lr=lr, mu=attrs.get("mu", 0.0),
                                      nesterov=attrs.get("use_nesterov", False))
        close(ref["p"], outs["ParamOut"])
        if vel is not None:
            close(ref["vel"], outs["VelocityOut"])
        return
    if op == "adam":
        ref, _ = O.adamw_reference(T(ins["Param"]), T(ins["Grad"]), T(ins["Moment1"]), T(ins["Moment2"]), lr=lr,
                                   beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                                   beta1_pow=float(ins["Beta1Pow"][0]), beta2_pow=float(ins["Beta2Pow"][0]),
                                   lr_t_eps=True)
        close(ref["p"], outs["ParamOut"])
        close(ref["m"], outs["Moment1Out"])
        close(ref["v"], outs["Moment2Out"])
        return
    kind = _OP_KIND[op]
    if op == "rmsprop" and attrs.get("centered"):
        kind = "rmsprop_centered"
    h = dict(O.EXT_HP[kind])
    if op == "ftrl":
        kind = "ftrl" if attrs["lr_power"] == -0.5 else "ftrl_pow"
        h = dict(O.EXT_HP[kind])
    d = dict(p=T(ins["Param"]), g=T(ins["Grad"]))
    d.update({_IN[k]: T(v) for k, v in ins.items() if k in _IN})
    if op == "rmsprop":
        d["mom"] = d.pop("m")
    if op == "adamax":
        h["bp1"] = float(ins["Beta1Pow"][0])
    ref, _ = O.ext_reference(kind, d, lr=lr, h=h)
    for k, want in outs.items():
        close(ref["mom" if (op == "rmsprop" and k == "MomentOut") else _OUT[k]], want)


# ---------------------------------------------------------------- the emulation meets every bound
WORST = {}


def _rec(op, name, s, b):
    WORST[(op, name)] = max(WORST.get((op, name), 0.0), s)
    assert s * O.EMU_MARGIN <= b, (op, name, s, b)


def _rec_bf16(op, name, s, b32):
    """A bf16 store: EMU_MARGIN on the fp32 part of the bound, the store's own rounding is sharp."""
    WORST[(op, name)] = max(WORST.get((op, name), 0.0), s)
    assert s <= b32 / O.EMU_MARGIN + O.BF16_ROUNDING, (op, name, s)
    assert O.bf16_bound(b32) == b32 + O.BF16_ROUNDING


def _adamw_emu_case(n, gd, de, flags, profile):
    p, g, m, v = O.adamw_inputs(profile, n, gd)
    for step in (1, 2, 3):
        kw = _adamw_kw(flags, step, de)
        ref, mag = O.adamw_reference(p, g, m, v, **kw)
        emu = O.adamw_emulated(p, g, m, v, **kw)
        for name in ("p", "m", "v"):
            _rec("adamw", name, O.elem_stat(emu[name], ref[name], mag[name]), O.bound("adamw", name))
        assert O.bf16_store_ok(emu["p"].bfloat16(), ref["p"], mag["p"], O.bound("adamw", "p"))
        _rec_bf16("adamw", "param_out bf16", O.elem_stat(emu["p"].bfloat16(), ref["p"], mag["p"]), O.bound("adamw", "p"))
        p, m, v = emu["p"], emu["m"], emu["v"]


def test_emulation_meets_adamw_bounds():
    seen = set()
    for n, gd, _pd, de, flags, profile in O.adamw_cases():
        if (n, gd, de, flags, profile) not in seen:
            seen.add((n, gd, de, flags, profile))
            _adamw_emu_case(n, gd, de, flags, profile)
    for profile in O.PROFILES:
        _adamw_emu_case(2055, torch.bfloat16, 1027, O.ADAMW_FLAGS[4], profile)
    _adamw_emu_case(O.ADAMW_N4_WRAP, torch.bfloat16, O.ADAMW_N4_WRAP // 2 + 1, O.ADAMW_FLAGS[4], "mixed")


def test_emulation_meets_adamw_bounds_largest():
    n = O.ADAMW_N8_WRAP
    p, g, m, v = O.adamw_inputs("mixed", n, torch.bfloat16)
    kw = _adamw_kw(O.ADAMW_FLAGS[4], 1, n - 2)
    ref, mag = O.adamw_reference(p, g, m, v, **kw)
    emu = O.adamw_emulated(p, g, m, v, **kw)
    for name in ("p", "m", "v"):
        _rec("adamw", name, O.elem_stat(emu[name], ref[name], mag[name]), O.bound("adamw", name))


def test_emulation_meets_momentum_bounds():
    for n in O.MOM_N:
        for k, flags in enumerate(O.MOM_FLAGS):
            has_vel, nest, wd, gs, lr_dev = flags
            for gd in O.GDTYPES:
                for pd in O.GDTYPES:
                    for profile in (O.PROFILES if n == 257 else (O.PROFILES[k % 5],)):
                        p, g, vel = O.momentum_inputs(profile, n, gd, pd)
                        kw = dict(lr=O.MOM_HP["lr"], mu=O.MOM_HP["mu"], nesterov=nest, weight_decay=wd, grad_scale=gs)
                        ref, mag = O.momentum_reference(p, g, vel if has_vel else None, **kw)
                        emu = O.momentum_emulated(p, g, vel if has_vel else None, **kw)
                        _rec("momentum", "p", O.elem_stat(emu["p32"], ref["p"], mag["p"]), O.bound("momentum", "p"))
                        if pd == torch.bfloat16:
                            assert O.bf16_store_ok(emu["p"], ref["p"], mag["p"], O.bound("momentum", "p"))
                            _rec_bf16("momentum", "p bf16", O.elem_stat(emu["p"], ref["p"], mag["p"]),
                                      O.bound("momentum", "p"))
                        if has_vel:
                            _rec("momentum", "vel", O.elem_stat(emu["vel"], ref["vel"], mag["vel"]),
                                 O.bound("momentum", "vel"))
    for second in (True, False):
        ent = O.multi_entries(second=second)
        kw = dict(lr=O.MOM_HP["lr"], mu=O.MOM_HP["mu"], nesterov=second, grad_scale=0.5)
        for e, (ref, mag), emu in zip(ent, O.multi_reference(ent, **kw), O.multi_emulated(ent, **kw)):
            _rec("multi", "p", O.elem_stat(emu["p32"], ref["p"], mag["p"]), O.bound("momentum", "p"))
            if e[0].dtype == torch.bfloat16:
                assert O.bf16_store_ok(emu["p"], ref["p"], mag["p"], O.bound("momentum", "p"))
                _rec_bf16("multi", "p bf16", O.elem_stat(emu["p"], ref["p"], mag["p"]), O.bound("momentum", "p"))
            _rec("multi", "vel", O.elem_stat(emu["vel"], ref["vel"], mag["vel"]), O.bound("momentum", "vel"))


def test_emulation_meets_sumsq_clip_fold_bounds():
    for n in O.SUMSQ_N:
        for dt in O.GDTYPES:
            for aligned in (True, False):
                x = torch.randn(n, generator=O._gen(n, 6)).to(dt)
                ref, mag = O.sumsq_reference(x, 3.25)
                emu = O.sumsq_emulated(x, 3.25, aligned)
                if n == 0:
                    assert emu == 3.25
                    continue
                _rec("sumsq", "out", abs(emu - ref) / mag, O.sumsq_bound(n, aligned))
    for ss, ns, mx in ((4.0, 0.5, 2.0), (4.0, 0.5, 0.3), (4.0, 0.5, float(np.float32(1) + np.float32(1e-6))),
                       (123.456, 0.125, 1.0)):
        ref, mag = O.clip_coef_reference(ss, ns, mx)
        _rec("clip_coef", "coef", abs(O.clip_coef_emulated(ss, ns, mx) - ref) / mag, O.bound("clip_coef", "coef"))
    assert O.clip_coef_emulated(4.0, 0.5, float(np.float32(1) + np.float32(1e-6))) == 1.0  # exactly at the threshold
    for n in (1, 257, O.MOM_N[-1]):
        for dt in O.GDTYPES:
            for fresh in (0, 1):
                dst, g = torch.randn(n, generator=O._gen(n, 7)), torch.randn(n, generator=O._gen(n, 8)).to(dt)
                ref, mag = O.fold_grad_reference(dst, g, fresh)
                _rec("fold_grad", "dst", O.elem_stat(O.fold_grad_emulated(dst, g, fresh), ref, mag),
                     O.bound("fold_grad", "dst"))


@pytest.mark.parametrize("kind", O.EXT_KINDS)
def test_emulation_meets_ext_bounds(kind):
    for n in O.EXT_N:
        d = O.ext_inputs(kind, n)
        ref, mag = O.ext_reference(kind, d)
        emu = O.ext_emulated(kind, d)
        b = O.ext_bounds(kind, n)
        assert set(ref) == set(emu) <= set(b)
        for name in ref:
            s = O.elem_stat(emu[name], ref[name], mag[name])
            if kind == "ftrl_pow" and name in O.FTRL_POW_EMU:
                # the measured figure itself: the emulation is where the bound comes from
                WORST[(kind, name)] = max(WORST.get((kind, name), 0.0), s)
                assert s <= O.FTRL_POW_EMU[name], (name, s)
            else:
                _rec(kind, name, s, b[name])


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nworst emulation statistic")
    for k in sorted(WORST):
        print("    %-18s %-16s %.2e" % (k + (WORST[k],)))


# ---------------------------------------------------------------- fault injection
def _adamw_fault_setup(profile="flat", n=2055, flags=O.ADAMW_FLAGS[4], de=1027):
    p, g, m, v = O.adamw_inputs(profile, n, torch.bfloat16)
    kw = _adamw_kw(flags, 1, de)
    ref, mag = O.adamw_reference(p, g, m, v, **kw)
    return (p, g, m, v), kw, ref, mag


def _p_stat(emu, ref, mag):
    return O.elem_stat(emu["p"], ref["p"], mag["p"])


def test_faults_are_caught():
    """Each fault is built into the float32 emulation and must push the per-element statistic
    over the bound, while the clean emulation stays under it.

    What ``test_kernels_gpu.py::test_adamw_flat``'s criterion (whole-tensor ``_rel`` < 1e-5 on
    the parameter) makes of the same faults is printed as ``global_rel``.  At n = 2055 it lets
    through decay_end off by one in either direction (4.9e-06, 3.1e-06), the last tail element
    not updated (1.4e-06) and epsilon in the wrong placement (1.6e-07, on the tiny profile);
    one group of 8 updated twice sits at 1.8e-05, just over it, and would pass at n = 10007.
    The other faults of the list move every element and exceed 1e-5."""
    (p, g, m, v), kw, ref, mag = _adamw_fault_setup()
    n = p.numel()
    b = O.bound("adamw", "p")
    clean = O.adamw_emulated(p, g, m, v, **kw)
    assert _p_stat(clean, ref, mag) <= b
    faults = {}

    for name, de in (("decay_end + 1", kw["decay_end"] + 1), ("decay_end - 1", kw["decay_end"] - 1)):
        faults[name] = O.adamw_emulated(p, g, m, v, **dict(kw, decay_end=de))
    f = {k: t.clone() for k, t in clean.items()}
    f["p"][n - 1] = p[n - 1]
    faults["last tail element not updated"] = f
    f = {k: t.clone() for k, t in clean.items()}
    s = slice(8 * 100, 8 * 101)
    twice = O.adamw_emulated(clean["p"][s], g[s], clean["m"][s], clean["v"][s], **dict(kw, decay_end=n))
    f["p"][s] = twice["p"]
    faults["elements [8k, 8k + 8) updated twice"] = f
    f = {k: t.clone() for k, t in clean.items()}
    f["p"][s] = torch.cat([clean["p"][s][4:], clean["p"][s][:4]])
    faults["lanes 4..7 swapped with lanes 0..3"] = f
    faults["grad_scale_tensor ignored"] = O.adamw_emulated(p, g, m, v, **dict(kw, grad_scale_tensor=None))
    faults["beta-pow from the by-value argument"] = O.adamw_emulated(p, g, m, v,
                                                                    **dict(kw, beta1_pow=None, beta2_pow=None))
    print()
    for name, emu in faults.items():
        s_ = _p_stat(emu, ref, mag)
        print("    %-40s elem_stat %.2e  global_rel %.2e" % (name, s_, O.global_rel(emu["p"], ref["p"])))
        assert s_ > 4 * b, name

    # epsilon placement: seen where eps matters, on the tiny profile (v underflows against eps)
    (pt, gt, mt, vt), kwt_, reft, magt = _adamw_fault_setup("tiny")
    assert _p_stat(O.adamw_emulated(pt, gt, mt, vt, **kwt_), reft, magt) <= b
    wrong = O.adamw_emulated(pt, gt, mt, vt, **dict(kwt_, lr_t_eps=not kwt_["lr_t_eps"]))
    print("    %-40s elem_stat %.2e  global_rel %.2e" % ("epsilon in the wrong placement", _p_stat(wrong, reft, magt),
                                                      O.global_rel(wrong["p"], reft["p"])))
    assert _p_stat(wrong, reft, magt) > 4 * b

    # momentum: the Nesterov flag ignored
    pm, gm, vel = O.momentum_inputs("flat", 257, torch.float32, torch.float32)
    kwm = dict(lr=0.05, mu=0.9, nesterov=True, weight_decay=0.01)
    refm, magm = O.momentum_reference(pm, gm, vel, **kwm)
    bm = O.bound("momentum", "p")
    assert O.elem_stat(O.momentum_emulated(pm, gm, vel, **kwm)["p"], refm["p"], magm["p"]) <= bm
    assert O.elem_stat(O.momentum_emulated(pm, gm, vel, **dict(kwm, nesterov=False))["p"], refm["p"], magm["p"]) > 4 * bm

    # multi-tensor table: wd on a no_weight_decay entry; the element at a chunk boundary skipped
    ent = O.multi_entries()
    kwt = dict(lr=0.05, mu=0.9)
    refs = O.multi_reference(ent, **kwt)
    i = [k for k, e in enumerate(ent) if e[4] == 0.0][0]
    bad = list(ent)
    bad[i] = ent[i][:4] + (0.01,) + ent[i][5:]
    emu = O.multi_emulated(bad, **kwt)[i]
    assert O.elem_stat(emu["p32"], refs[i][0]["p"], refs[i][1]["p"]) > 4 * O.bound("momentum", "p")
    j = O.MULTI_LENS.index(4097)
    emu = O.multi_emulated(ent, **kwt)[j]
    bj = O.bound("momentum", "p", ent[j][0].dtype)
    assert ent[j][0].dtype == torch.bfloat16  # the bf16 target: a skipped element must show through the store's rounding
    assert O.bf16_store_ok(emu["p"], refs[j][0]["p"], refs[j][1]["p"], O.bound("momentum", "p"))
    skipped = emu["p"].clone()
    skipped[O.MCHUNK] = ent[j][0][O.MCHUNK]
    assert not O.bf16_store_ok(skipped, refs[j][0]["p"], refs[j][1]["p"], O.bound("momentum", "p"))
    assert O.elem_stat(skipped, refs[j][0]["p"], refs[j][1]["p"]) > 4 * bj
    print("    %-40s global_rel %.2e" % ("chunk boundary (4096) skipped", O.global_rel(skipped.float(), refs[j][0]["p"])))

    # LARS: the norm of the first block only
    d = O.ext_inputs("lars", 2055)
    refl, magl = O.ext_reference("lars", d)
    bl = O.ext_bounds("lars", 2055)["p"]
    assert O.elem_stat(O.ext_emulated("lars", d)["v"], refl["v"], magl["v"]) <= bl
    assert O.elem_stat(O.ext_emulated("lars", d, _norm_n=256)["v"], refl["v"], magl["v"]) > 4 * bl


def test_emulation_meets_bf16_store_bound():
    """One bf16 rounding is 2 u with u = 2^-9, not 1 u: the correctly rounded in-place bf16
    parameter of the emulation exceeds fp32 bound + 2^-9 and stays under ``bf16_bound``."""
    worst = 0.0
    for n in O.MOM_N[:4]:
        p, g, vel = O.momentum_inputs("flat", n, torch.float32, torch.bfloat16)
        kw = dict(lr=O.MOM_HP["lr"], mu=O.MOM_HP["mu"])
        ref, mag = O.momentum_reference(p, g, vel, **kw)
        worst = max(worst, O.elem_stat(O.momentum_emulated(p, g, vel, **kw)["p"], ref["p"], mag["p"]))
    assert O.bound("momentum", "p") + O.U16 < worst <= O.bound("momentum", "p", torch.bfloat16)
