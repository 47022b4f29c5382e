"""The rigid-contact plant (lmh_plant_derivative_rigid, lmh_plant_step_rigid) and the joint servo in the plant hold (lmh_plant_step_servo)
on the GPU over the postures of a fall, where test_gpu_rigid.py and test_gpu_servo.py stay within 5 degrees and 0.3 m/s of standing.

Inputs: fall_rigid_cases.py on fall_cases' 16 states per band (joints, roll, pitch and yaw across +-1.0 and +-3.1 rad, +-2 m/s and
+-5 rad/s, soles on edge and upside down), its step references' x0 (velocities x 1/4), its planes tilted 5 .. 35 degrees and its pitch
ladder.  test_fall_rigid_cases.py asserts on the CPU that the reference alone meets every condition below with orders to spare.  Every
launch is 16 robots at the most and 20 substeps at the most.

Tolerances are the project's own, unchanged (test_gpu_rigid.py, test_gpu_servo.py): backward error 1e-12, the constraint residual 1e-12
on |A| |lam| + |g|, forward error 1e-12 cond(KKT) against the long-double-refined KKT solve, 1e-7 `close` behind 20 substeps (the
multiplier with the weight's floor).  The pull and slip flags are compared with the statement's wherever its multiplier decides them by
more than fall_rigid_cases.flag_margin, what that forward tolerance lets the multiplier differ by; on the CPU that is all 192 decisions
of each band."""
import numpy as np
import pytest
import torch

import fall_cases as fc
import fall_rigid_cases as frc
import plant_step_cases as pc
import rigid_cases as rc
from helpers import WEIGHT, close, make_controller, rel_err, same_bits as _same, to_device, vec_err
from rigid_support import check_figures, derivative_against as _derivative_against, device_terms, flight_against_the_plain_derivative, imode as _imode

pytestmark = pytest.mark.gpu
DT, TH, B = pc.DT, pc.TH, pc.B


def _ctl(S, n=B):
    return make_controller(n, DT, TH, S["zcom"])


def _state(ctl, x0, t=0.25):
    return ctl.new_state(x0[:, :30], x0[:, 30:], t=t)


# ------------------------------------------------------------------------------- derivative
@pytest.mark.parametrize("band", fc.BANDS)
def test_derivative_against_the_statement_on_the_oracles_terms(band):
    S = frc.rigid_fall_cases(band)
    _derivative_against(lambda i: S["terms"][i], "the oracle's terms, band %g" % band, S=S, decided=frc.decided_on)


@pytest.mark.parametrize("band", fc.BANDS)
def test_derivative_against_the_statement_on_the_devices_terms(band):
    """The statement fed with the GPU's own terms(q, v) record (M, C, J, Jpqp; vhat and the base's X_0 stay the oracle's)."""
    S = frc.rigid_fall_cases(band)
    ctl = _ctl(S)
    dev = device_terms(ctl, S)
    _derivative_against(lambda i: dev[i], "the device's terms, band %g" % band, S=S, decided=frc.decided_on)
    ctl.close()


@pytest.mark.parametrize("band", fc.BANDS)
def test_flight_is_the_plain_derivative_out_of_the_ground(band):
    """The 16 states lifted until their lowest vertex is 5 cm above z = 0, LMH_PHASE_FLIGHT: xdot is lmh_plant_derivative's bit for bit --
    the first right-hand side of the multi-right-hand-side solve sees plant_minv's operations in plant_minv's order at tilted postures
    too -- and lambda is exactly 0."""
    S, F = frc.rigid_fall_cases(band), fc.fall_states(band)
    ctl = _ctl(S)
    qn = S["q"].copy()
    qn[:, 2] += 0.05 - F["pos"][:, :, 2].min(axis=1)
    q, v, tau = to_device(ctl, qn), to_device(ctl, S["v"]), to_device(ctl, S["tau"])
    xd, held = flight_against_the_plain_derivative(ctl, q, v, tau, "band %g, " % band)
    assert all(not _same(held[i], xd[i]) for i in range(B))        # held soles act 5 cm up too, on every robot
    ctl.close()


def test_derivative_on_the_pitch_ladder():
    """pitch = +-(pi/2 - delta) down to 1e-6 rad from the Euler-rate singularity, both soles held, kv = 50: qdot is lmh_plant_derivative's
    bit for bit and the three bounds hold at every rung."""
    from linearmpchumanoid_amd import capi
    Ld = frc.rigid_ladder_cases()
    n = len(Ld["q"])
    ctl = _ctl(Ld, n)
    q, v, tau = (to_device(ctl, Ld[k]) for k in ("q", "v", "tau"))
    xd, _, _ = ctl.plant_derivative(q, v, tau)
    xr, lam, flags = ctl.plant_derivative_rigid(q, v, tau, _imode(ctl, np.zeros(n)), 50.0)
    torch.cuda.synchronize()
    assert _same(xr[:, :30], xd[:, :30])
    xr, lam, flags = xr.cpu().numpy(), lam.cpu().numpy(), flags.cpu().numpy()
    print()
    for i in range(n):
        worst = dict(backward=0.0, constraint=0.0, forward=0.0)
        b = rc.bounds(Ld["terms"][i], Ld["tau"][i], 0, 50.0, rc.a_from_xdot(xr[i], Ld["terms"][i]["X"][0]), lam[i])
        check_figures(b, xr[i], lam[i], rc.RIGID_ROWS[0], worst, i)
        assert not flags[i] & (capi.FLAG_NOT_SPD | capi.FLAG_NONFINITE), (i, flags[i])
        print("pitch %+.6f (delta %.0e): backward %.2e, constraint %.2e, forward/cond %.2e (largest |qdot| %.2e)"
              % (Ld["q"][i, 4], Ld["delta"][i], worst["backward"], worst["constraint"], worst["forward"], np.abs(xr[i, :30]).max()))
    ctl.close()


# ------------------------------------------------------------------------------- step
@pytest.mark.parametrize("config", [c[0] for c in frc.STEP_CONFIGS])
@pytest.mark.parametrize("band", fc.BANDS)
def test_twenty_substeps_against_the_statement(band, config):
    """Configuration a: kv = 50, both soles held; b: kv = 0, mode (i + 1) % 3.  7 + 13 substeps are 20 bit for bit in state, multiplier
    and OR-ed flags; 20 substeps are rk4_tick over the statement on the oracle within the 1e-7 `close`."""
    from linearmpchumanoid_amd import capi
    R = frc.rigid_step_references(band)
    C = R[config]
    ctl = _ctl(fc.fall_states(band))
    tau, mode, kv = to_device(ctl, R["tau"]), _imode(ctl, C["mode"]), C["kv"]
    s20, l20, f20 = ctl.plant_step_rigid(_state(ctl, R["x0"]), tau, mode, kv, 20)
    s7, _, f7 = ctl.plant_step_rigid(_state(ctl, R["x0"]), tau, mode, kv, 7)
    s713, l13, f13 = ctl.plant_step_rigid(s7.clone(), tau, mode, kv, 13)
    torch.cuda.synchronize()
    assert _same(s713, s20) and _same(l13, l20) and _same(f7 | f13, f20)
    a, lam, flags = s20.cpu().numpy(), l20.cpu().numpy(), f20.cpu().numpy()
    worst, worst_lam = 0.0, 0.0
    for i in range(B):
        worst, worst_lam = max(worst, rel_err(a[i, :60], C["x"][i])), max(worst_lam, vec_err(lam[i], C["lam"][i]))
        assert close(a[i, :60], C["x"][i], 1e-7), (i, rel_err(a[i, :60], C["x"][i]))
        assert close(lam[i], C["lam"][i], 1e-7, scale=WEIGHT), (i, vec_err(lam[i], C["lam"][i]))
        assert not flags[i] & (capi.FLAG_NOT_SPD | capi.FLAG_NONFINITE), (i, flags[i])
    assert np.array_equal(a[:, 90], np.full(B, sum([0.25] + [DT] * 20)))
    print("\nrigid step, band %g, configuration %s, 20 substeps vs the statement's RK4: state %.2e, lambda %.2e (largest |x| %.1e, |lambda| %.0f N)"
          % (band, config, worst, worst_lam, np.abs(C["x"]).max(), np.abs(C["lam"]).max()))
    ctl.close()


# ------------------------------------------------------------------------------- robots stay apart
def _both_calls(ctl, S, R, rows, mode_np, kv=50.0, n_substeps=3, poison=None):
    """The derivative at the states and 3 substeps from the step references' x0 of the robots `rows` -> (xdot, lam, flags, state, lam,
    flags).  poison(q, v) may write into copies of the [len(rows), 30] inputs of both calls."""
    q, v, x0 = S["q"][rows].copy(), S["v"][rows].copy(), R["x0"][rows].copy()
    if poison is not None:
        poison(q, v)
        poison(x0[:, :30], x0[:, 30:])
    mode = _imode(ctl, mode_np[rows])
    res = ctl.plant_derivative_rigid(to_device(ctl, q), to_device(ctl, v), to_device(ctl, S["tau"][rows]), mode, kv) \
        + ctl.plant_step_rigid(_state(ctl, x0), to_device(ctl, R["tau"][rows]), mode, kv, n_substeps)
    torch.cuda.synchronize()
    return tuple(x.cpu() for x in res)


@pytest.mark.parametrize("band", fc.BANDS)
def test_permutation_and_one_robot_handles(band):
    """A permuted batch gives the permuted bytes, and robots 3 and 12 alone in a handle give the batch's bytes, derivative and step."""
    S, R = frc.rigid_fall_cases(band), frc.rigid_step_references(band)
    mode_np = np.array([(i * 7 + 1) % 4 for i in range(B)], dtype=np.int32)            # all four modes
    ctl = _ctl(S)
    whole = _both_calls(ctl, S, R, np.arange(B), mode_np)
    perm = np.random.default_rng([fc.FALL_SEED, 7]).permutation(B)
    assert all(_same(x[perm].contiguous(), y) for x, y in zip(whole, _both_calls(ctl, S, R, perm, mode_np)))
    ctl.close()
    for i in (3, 12):
        one = _ctl(S, 1)
        assert all(_same(x[i:i + 1].contiguous(), y) for x, y in zip(whole, _both_calls(one, S, R, np.array([i]), mode_np))), i
        one.close()
    assert len({whole[0][i].numpy().tobytes() for i in range(B)}) == B


@pytest.mark.parametrize("band", fc.BANDS)
def test_nonfinite_words_stay_with_their_robot(band):
    """Robot 5 with q[8] = NaN; separately robot 9 with v[6:] = 1e160, whose velocity products overflow: the derivative and 3 substeps
    flag that robot FLAG_NONFINITE, and every other robot's flags and bytes are the clean batch's.  These are IEEE values, not faults:
    the kernel's loops have fixed trip counts and index nothing by data."""
    from linearmpchumanoid_amd import capi
    S, R = frc.rigid_fall_cases(band), frc.rigid_step_references(band)
    mode_np = np.array([i % 3 for i in range(B)], dtype=np.int32)
    ctl = _ctl(S)
    clean = _both_calls(ctl, S, R, np.arange(B), mode_np)
    assert not (clean[2].numpy() & capi.FLAG_NONFINITE).any() and not (clean[5].numpy() & capi.FLAG_NONFINITE).any()

    def nan_in_q(q, v):
        q[5, 8] = np.nan

    def huge_v(q, v):
        v[9, 6:] = 1.0e160

    for robot, poison in ((5, nan_in_q), (9, huge_v)):
        bad = _both_calls(ctl, S, R, np.arange(B), mode_np, poison=poison)
        others = [i for i in range(B) if i != robot]
        for k, (x, y) in enumerate(zip(clean, bad)):
            assert _same(x[others].contiguous(), y[others].contiguous()), (poison.__name__, k)
        for k in (0, 3):                                           # the word was read
            assert not _same(clean[k][robot], bad[k][robot]), (poison.__name__, k)
        for k in (2, 5):
            assert int(bad[k][robot]) & capi.FLAG_NONFINITE, (poison.__name__, k, int(bad[k][robot]))
    ctl.close()


# ------------------------------------------------------------------------------- servo
@pytest.mark.parametrize("ground", ("flat", "planes"))
@pytest.mark.parametrize("band", fc.BANDS)
def test_plant_step_servo_over_a_fall(band, ground):
    """plant_step_servo from the step references' x0 with servo_cases' gains and setpoints drawn at those states, on z = 0 and on the
    state's planes: 20 substeps within the 1e-7 `close` of the oracle's RK4 with trajectories.servo_torque at every stage, 7 + 13 = 20 bit
    for bit, no flag, and every robot away from plant_step without the table."""
    V = frc.servo_fall_cases(band)
    ref = V["ref_flat"] if ground == "flat" else V["ref_planes"]
    ctl = _ctl(V)
    ctl.set_servo(V["rec"][:, 0:24], V["rec"][:, 24:48])
    if ground == "planes":
        ctl.set_ground(V["planes"])
    tau, sp = to_device(ctl, V["tau"]), to_device(ctl, V["sp"])
    s20, f20 = ctl.plant_step_servo(_state(ctl, V["x0"]), sp, tau, 20)
    s7, f7 = ctl.plant_step_servo(_state(ctl, V["x0"]), sp, tau, 7)
    s713, f13 = ctl.plant_step_servo(s7.clone(), sp, tau, 13)
    free, _ = ctl.plant_step(_state(ctl, V["x0"]), tau, 20)
    torch.cuda.synchronize()
    assert _same(s713, s20)
    for f in (f20, f7, f13):
        assert int(f.abs().max()) == 0
    a, worst = s20.cpu().numpy(), 0.0
    for i in range(B):
        e = rel_err(a[i, :60], ref[i])
        worst = max(worst, e)
        assert close(a[i, :60], ref[i], 1e-7), (i, e)
        assert not _same(s20[i, :60], free[i, :60]), i             # the servo matters on every robot
    print("\nplant_step_servo over a fall, band %g, %s, 20 substeps vs the oracle's RK4 with the servo at every stage: %.2e (largest |x| %.1e)"
          % (band, ground, worst, np.abs(ref).max()))
    ctl.close()
