"""The torque-driven plant and the public dynamics calls on the GPU against the CPU oracle over the postures of a fall.

Inputs: fall_cases.fall_states(band), band in (1.0, 3.1) -- 16 states each whose joints, roll, pitch and yaw span the band, moving at
+-2 m/s, +-5 rad/s (base) and +-5 rad/s (joints), every contact regime on both feet with margin, soles on edge and upside down -- with
fall_cases.fall_planes(band) (normals tilted 5 .. 35 degrees) for the ground table, and fall_cases.pitch_ladder() up to 1e-6 rad from the
Euler-rate singularity.  test_fall_cases.py asserts on the CPU what the draw covers.  Every check runs on lmh_plant_kernel (a handle
without a table) and on its GROUND instantiation (set_ground); every launch is 16 robots at the most and 20 substeps at the most.

References, reused from the existing tests: test_gpu_terms._oracle_terms / _check_terms, plant_step_cases.oracle_plant_xdot /
oracle_plant_steps, ground_cases.ground_plant_xdot / ground_plant_steps, Oracle.contact() and trajectories.ground_contact.

Tolerances are the project's own, unchanged: 1e-11 for the terms, the inverse dynamics and the contact forces on their scales; qdot 1e-13
relative; backward error of the solve 1e-12 and forward error over cond(M) 1e-12; 1e-7 `close` behind 20 substeps.  The reference judged
alone on these 32 states (test_fall_cases.test_the_reference_alone) agrees with the independent restatement to 2.8e-15 at the worst (J; M
8.4e-16, C 1.5e-15, AG 8.6e-16, AGpqp 1.8e-15, Jpqp 1.8e-15, CoM 4.4e-16), numpy's solve with a long-double solve to 7.9e-20 of
cond(M) max|a|, and the helper's Euler-rate map with a long-double one to 2.1e-16 on the ladder: every figure is below a hundredth of its
tolerance, so none is widened.  cond(M) is 8.4e4 .. 4.3e5 over the 32 states."""
import numpy as np
import pytest
import torch

import fall_cases as fc
import ground_cases as gc
import plant_step_cases as pc
from dynamics_support import check_contact as _check_contact, check_terms as _check_terms, ninf as _ninf, oracle_terms as _oracle_terms, to_m_coordinates as _to_m_coordinates
from helpers import WEIGHT, close, close_on, make_controller, rel_err, same_bits, to_device

pytestmark = pytest.mark.gpu
DT, TH, B = pc.DT, pc.TH, pc.B
G = pc.GROUND
GROUNDS = ("flat", "planes")

_cache = {}


def _setup(band):
    """The 16 states of a band with their oracle terms, the helper's derivative on both grounds and the random qdd of the dynamics tests
    (computed once, shared, never written)."""
    if band not in _cache:
        S, P = fc.fall_states(band), fc.fall_planes(band)
        o = pc.make_oracle()
        terms = [_oracle_terms(S["q"][i], S["v"][i]) for i in range(B)]
        flat, planes = [], []
        for i in range(B):
            xdot, parts = pc.oracle_plant_xdot(o, S["q"][i], S["v"][i], S["tau"][i])
            flat.append(dict(xdot=xdot, pos=S["pos"][i], vel=S["vel"][i], **parts))
            xdot, parts = gc.ground_plant_xdot(o, S["q"][i], S["v"][i], S["tau"][i], P["planes"][i])
            planes.append(dict(xdot=xdot, **parts))
        qdd = np.random.default_rng([fc.FALL_SEED, 5]).normal(0.0, 10.0, (B, 30))
        w = S["w"]                                                 # the oracle's contact wrench of the state
        tau_id = np.stack([r["t"]["M"] @ qdd[i] + r["t"]["C"] - r["t"]["J"].T @ w[i] for i, r in enumerate(terms)])
        _cache[band] = dict(S=S, P=P, terms=terms, flat=flat, planes=planes, qdd=qdd, w=w, tau_id=tau_id)
    return _cache[band]


def _ctl(K, ground, n=B):
    ctl = make_controller(n, DT, TH, K["S"]["zcom"])
    if ground == "planes":
        ctl.set_ground(K["P"]["planes"][:n])
    return ctl


# ------------------------------------------------------------------------------- terms, inverse and forward dynamics
@pytest.mark.parametrize("band", fc.BANDS)
def test_terms(band):
    K = _setup(band)
    S = K["S"]
    ctl = _ctl(K, "flat")
    rec = ctl.terms(to_device(ctl, S["q"]), to_device(ctl, S["v"]))
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    mass = float(ctl.mass()[0])
    worst, bad = {}, []
    for i in range(B):
        bad += _check_terms(rec[i], K["terms"][i], S["v"][i], mass, worst, i)
    print("\nterms, band %g: " % band + ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert not bad, bad[:12]
    ctl.close()


@pytest.mark.parametrize("band", fc.BANDS)
def test_inverse_and_forward_dynamics(band):
    """test_gpu_terms' criteria: tau30 on its scale at 1e-11; the solve's backward error and forward error / cond(M) at 1e-12, from the
    oracle's tau30 and from the device's own (round trip).  w is the oracle's contact wrench of the state."""
    K = _setup(band)
    S = K["S"]
    ctl = _ctl(K, "flat")
    q, v, qdd, w, tau = (to_device(ctl, a) for a in (S["q"], S["v"], K["qdd"], K["w"], K["tau_id"]))
    tau_dev = ctl.inverse_dynamics(q, v, qdd, w)
    x, flags = ctl.forward_dynamics(q, v, tau, w)
    x2, flags2 = ctl.forward_dynamics(q, v, tau_dev, w)
    torch.cuda.synchronize()
    assert flags.dtype == torch.int32 and int(flags.abs().max()) == 0 and int(flags2.abs().max()) == 0
    tau_dev, x, x2 = tau_dev.cpu().numpy(), x.cpu().numpy(), x2.cpu().numpy()
    worst = dict(inverse=0.0, backward=0.0, forward=0.0, round_trip=0.0)
    for i in range(B):
        t = K["terms"][i]["t"]
        M = t["M"]
        scale = _ninf(M) * np.abs(K["qdd"][i]).max() + np.abs(t["C"]).max() + _ninf(t["J"].T) * np.abs(K["w"][i]).max()
        inv = float(np.abs(tau_dev[i] - K["tau_id"][i]).max() / scale)
        rhs = K["tau_id"][i] + t["J"].T @ K["w"][i] - t["C"]
        back = _ninf(M @ x[i] - rhs) / (_ninf(M) * _ninf(x[i]) + _ninf(rhs))
        fwd = _ninf(x[i] - K["qdd"][i]) / (S["cond"][i] * _ninf(K["qdd"][i]))
        rt = _ninf(x2[i] - K["qdd"][i]) / (S["cond"][i] * _ninf(K["qdd"][i]))
        for k, val in (("inverse", inv), ("backward", back), ("forward", fwd), ("round_trip", rt)):
            worst[k] = max(worst[k], float(val))
        assert close_on(tau_dev[i], K["tau_id"][i], 1e-11, scale), (i, inv)
        assert np.isfinite(x[i]).all() and np.isfinite(x2[i]).all() and back <= 1e-12 and fwd <= 1e-12 and rt <= 1e-12, (i, back, fwd, rt)
    print("\ndynamics, band %g: inverse %.2e of its scale; forward: backward %.2e, forward/cond %.2e, device round trip forward/cond %.2e (max |w| %.0f N)"
          % (band, worst["inverse"], worst["backward"], worst["forward"], worst["round_trip"], np.abs(K["w"]).max()))
    assert np.abs(K["w"]).max() > WEIGHT                           # the wrench of a robot pressed into the ground, not of one standing
    ctl.close()


# ------------------------------------------------------------------------------- contact
def _check_planes_contact(rec, r, planes, tag):
    """test_gpu_ground.test_contact_wrench_is_the_statement's checks of one record."""
    from linearmpchumanoid_amd.controller import BatchedController
    s = BatchedController.split_contact(rec)
    scale = G["k"] * np.abs(r["pos"]).max() + (G["d"] + G["dt"]) * np.abs(r["vel"]).max()
    pen = gc.thresholds(r["pos"], r["vel"], planes)[0]
    assert not s["vertex_force"][~(pen > 0.0)].any(), tag           # exactly 0 out of the ground
    assert np.array_equal(s["vertex_force"] == 0.0, r["vf"] == 0.0), tag             # and the statement's clamps
    assert close_on(s["vertex_force"], r["vf"], 1e-11, scale), (tag, np.abs(s["vertex_force"] - r["vf"]).max() / scale)
    got, w = s["w"].reshape(2, 2, 3), r["w"].reshape(2, 2, 3)
    assert close_on(got[:, 1], w[:, 1], 1e-11, 4 * scale), (tag, np.abs(got[:, 1] - w[:, 1]).max() / scale)
    assert close_on(got[:, 0], w[:, 0], 1e-11, 4 * scale * 0.11), (tag, np.abs(got[:, 0] - w[:, 0]).max() / scale)
    assert not s["pad"].any()
    return float(max(np.abs(s["vertex_force"] - r["vf"]).max(), np.abs(s["w"] - r["w"]).max()) / scale)


def _contact_errors(c, K, ground):
    if ground == "flat":
        return [_check_contact(c[i], K["flat"][i], i) for i in range(B)]
    return [_check_planes_contact(c[i], K["planes"][i], K["P"]["planes"][i], i) for i in range(B)]


@pytest.mark.parametrize("ground", GROUNDS)
@pytest.mark.parametrize("band", fc.BANDS)
def test_contact_wrench(band, ground):
    """Against Oracle.contact() (flat) / trajectories.ground_contact on the oracle's vertex kinematics (planes): the same zero pattern,
    1e-11 of test_gpu_plant_step._check_contact's force scale, pads zero."""
    K = _setup(band)
    S = K["S"]
    ctl = _ctl(K, ground)
    c = ctl.contact_wrench(to_device(ctl, S["q"]), to_device(ctl, S["v"]))
    torch.cuda.synchronize()
    c = c.cpu().numpy()
    if ground == "planes":                                         # the statement's forces are the cached ones of the draw
        assert all(np.array_equal(K["planes"][i]["vf"], K["P"]["force"][i]) for i in range(B))
    errs = _contact_errors(c, K, ground)
    print("\ncontact wrench, band %g, %s: worst error on the force scale %.2e (largest vertex force %.0f N)"
          % (band, ground, max(errs), max(np.abs(r["vf"]).max() for r in K[ground])))
    ctl.close()


# ------------------------------------------------------------------------------- derivative
def _check_derivative(xdot, r, tau, cond, tag):
    """The three criteria of test_plant_derivative_against_the_helper -> (qdot, backward, forward / cond)."""
    M, J, Cv = r["terms"]["M"], r["terms"]["J"], r["terms"]["C"]
    e = rel_err(xdot[:30], r["xdot"][:30])
    x = _to_m_coordinates(xdot[30:], r["terms"]["X"][0])
    rhs = tau + J.T @ r["w"] - Cv
    back = _ninf(M @ x - rhs) / (_ninf(M) * _ninf(x) + _ninf(rhs))
    fwd = _ninf(x - r["a"]) / (cond * _ninf(r["a"]))
    assert np.isfinite(xdot).all() and e <= 1e-13 and back <= 1e-12 and fwd <= 1e-12, (tag, e, back, fwd)
    return float(e), float(back), float(fwd)


@pytest.mark.parametrize("ground", GROUNDS)
@pytest.mark.parametrize("band", fc.BANDS)
def test_plant_derivative(band, ground):
    K = _setup(band)
    S = K["S"]
    ctl = _ctl(K, ground)
    q, v, tau = (to_device(ctl, S[k]) for k in ("q", "v", "tau"))
    xdot, c, flags = ctl.plant_derivative(q, v, tau)
    cw = ctl.contact_wrench(q, v)
    torch.cuda.synchronize()
    assert same_bits(c, cw)                                        # the contact record is contact_wrench's, bitwise
    assert flags.dtype == torch.int32 and int(flags.abs().max()) == 0
    _contact_errors(c.cpu().numpy(), K, ground)
    xdot = xdot.cpu().numpy()
    res = np.array([_check_derivative(xdot[i], K[ground][i], S["tau"][i], S["cond"][i], i) for i in range(B)])
    print("\nplant derivative, band %g, %s: qdot %.2e, backward %.2e, forward/cond %.2e (largest |a| %.1e)"
          % (band, ground, *res.max(axis=0), max(np.abs(r["a"]).max() for r in K[ground])))
    ctl.close()


def test_plant_derivative_on_the_pitch_ladder():
    """pitch = +-(pi/2 - delta), every vertex out of the ground: qdot[3:6] = E(rpy) w has entries of size 1 / cos(pitch) up to 1e6, from the
    device's reduced-range cosine and reciprocal against libm's and a division.  The same three criteria at every rung."""
    Ld = fc.pitch_ladder()
    n = len(Ld["q"])
    o = pc.make_oracle()
    ctl = make_controller(n, DT, TH, Ld["zcom"])
    q, v, tau = (to_device(ctl, Ld[k]) for k in ("q", "v", "tau"))
    xdot, c, flags = ctl.plant_derivative(q, v, tau)
    torch.cuda.synchronize()
    assert int(flags.abs().max()) == 0 and float(c.abs().max()) == 0.0
    xdot = xdot.cpu().numpy()
    print()
    for i in range(n):
        want, parts = pc.oracle_plant_xdot(o, Ld["q"][i], Ld["v"][i], Ld["tau"][i])
        cond = float(np.linalg.cond(parts["terms"]["M"]))
        e, back, fwd = _check_derivative(xdot[i], dict(xdot=want, **parts), Ld["tau"][i], cond, i)
        eu = float(np.abs(xdot[i, 3:6] - want[3:6]).max() / np.abs(want[3:6]).max())
        print("pitch %+.6f (delta %.0e): qdot %.2e (Euler rates alone %.2e, largest %.2e rad/s), backward %.2e, forward/cond %.2e"
              % (Ld["q"][i, 4], Ld["delta"][i], e, eu, np.abs(want[3:6]).max(), back, fwd))
    ctl.close()


# ------------------------------------------------------------------------------- step
@pytest.mark.parametrize("ground", GROUNDS)
@pytest.mark.parametrize("band", fc.BANDS)
def test_plant_step(band, ground):
    """The states with their velocities x 1/4 (fall_cases.step_references: 20 ms then carry no vertex to within round-off of a regime
    threshold, asserted on the CPU): 7 + 13 substeps are 20 bit for bit, and 20 substeps are the helper's RK4 within the 1e-7 `close`."""
    K = _setup(band)
    T = fc.step_references(band)
    ctl = _ctl(K, ground)
    tau = to_device(ctl, T["tau"])
    mk = lambda: ctl.new_state(T["x0"][:, :30], T["x0"][:, 30:], t=0.25)
    s20, f20 = ctl.plant_step(mk(), tau, 20)
    s7, f7 = ctl.plant_step(mk(), tau, 7)
    s713, f13 = ctl.plant_step(s7.clone(), tau, 13)
    torch.cuda.synchronize()
    assert same_bits(s713, s20)
    for f in (f20, f7, f13):
        assert int(f.abs().max()) == 0
    a, worst = s20.cpu().numpy(), 0.0
    for i in range(B):
        ref = T[ground]["x"][i]
        worst = max(worst, rel_err(a[i, :60], ref))
        assert close(a[i, :60], ref, 1e-7), (i, rel_err(a[i, :60], ref))
    print("\nplant step, band %g, %s, 20 substeps vs the helper's RK4: %.2e (largest |x| of a reference %.1e)" % (band, ground, worst, np.abs(T[ground]["x"]).max()))
    ctl.close()


# ------------------------------------------------------------------------------- non-finite words
def _every_call(ctl, q, v, tau, qdd, w):
    """Every plant and dynamics call on one batch -> [(name, bytes as a CPU tensor, flags or None)].  plant_step runs 3 substeps."""
    dq, dv, dtau, dqdd, dw = (to_device(ctl, a) for a in (q, v, tau, qdd, w))
    x, ff = ctl.forward_dynamics(dq, dv, dtau, dw)
    xdot, c, fd = ctl.plant_derivative(dq, dv, dtau)
    st, fs = ctl.plant_step(ctl.new_state(q, v, t=0.0), dtau, 3)
    res = [("forward_dynamics", x, ff), ("plant_derivative", torch.cat([xdot, c], dim=1), fd), ("plant_step", st, fs),
           ("terms", ctl.terms(dq, dv), None), ("inverse_dynamics", ctl.inverse_dynamics(dq, dv, dqdd, dw), None), ("contact_wrench", ctl.contact_wrench(dq, dv), None)]
    torch.cuda.synchronize()
    return [(name, a.cpu(), None if f is None else f.cpu().numpy()) for name, a, f in res]


@pytest.mark.parametrize("ground", GROUNDS)
def test_nonfinite_words_stay_with_their_robot(ground):
    """Robot 5 with q[8] = NaN; separately robot 9 with v[6:] = 1e160, whose velocity products overflow.  forward_dynamics,
    plant_derivative and plant_step (3 substeps) flag that robot FLAG_NONFINITE; every other robot's flags and bytes -- and for terms,
    inverse_dynamics and contact_wrench, which have no flags, its bytes -- are those of a clean batch.  The kernels' loops have trip
    counts fixed by n_substeps and compile-time sizes and index nothing by data: a non-finite word changes values only."""
    from linearmpchumanoid_amd import capi
    K = _setup(1.0)
    S = K["S"]
    ctl = _ctl(K, ground)
    clean = _every_call(ctl, S["q"], S["v"], S["tau"], K["qdd"], K["w"])
    for robot, poison in ((5, "q"), (9, "v")):
        q, v = S["q"].copy(), S["v"].copy()
        if poison == "q":
            q[robot, 8] = np.nan
        else:
            v[robot, 6:] = 1.0e160
        others = [i for i in range(B) if i != robot]
        for (name, a, f), (_, a0, f0) in zip(_every_call(ctl, q, v, S["tau"], K["qdd"], K["w"]), clean):
            assert same_bits(a[others].contiguous(), a0[others].contiguous()), (poison, name)
            if name != "contact_wrench":                           # (a foot out of the ground stays at exactly 0 whatever its velocity)
                assert not same_bits(a[robot], a0[robot]), (poison, name)         # the word was read
            if f is not None:
                assert f[robot] & capi.FLAG_NONFINITE, (poison, name, f[robot])
                assert np.array_equal(f[others], f0[others]) and not (f0 & capi.FLAG_NONFINITE).any(), (poison, name, f, f0)
    ctl.close()
