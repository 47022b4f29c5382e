"""The register tail of a rollout evaluation: the recovery hands the integrator its xdot in registers, the non-finite guard tests those
registers, and the state, Robot::v_ and (at the fourth stage only) the accelerations are published once per stage.

(a) short rollouts from the posture sweep's integrator states against RK4 on the host over the plain evaluation kernel, the out record's
    accelerations included; (b) launches that end one tick before, on and one tick behind a chunk boundary against the same ticks
    ending in single-tick launches, bit for bit; (c) a non-finite state in a rollout is flagged, its neighbours are untouched."""
import numpy as np
import pytest
import torch

from helpers import SWEEP_BANDS, TOL_REL, WEIGHT, close, make_controller, oracle_system, perturbed_velocities, posture_sweep, start_posture, vec_err

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DT, TH = 1e-3, 0.016
B_ROLL = 8                       # the rollout comparison of tests/test_gpu_posture_sweep.py: posture_sweep(q0, 8, band) in every band
CHUNK = 250                      # LMH_CHUNK_TICKS of the shipped build


@pytest.fixture(scope="module")
def consts():
    return start_posture(oracle_system(DT, TH))


def _xdot(x, qpp):
    """apps/offline/main.cpp:107-121: classic base velocity, Euler rates, accelerations"""
    xd = np.zeros_like(x)
    xd[:, :30] = x[:, 30:]
    xd[:, :3] = x[:, 30:33] + np.cross(x[:, 33:36], x[:, :3])
    p_, y_, w = x[:, 4], x[:, 5], x[:, 33:36]
    xd[:, 3] = (np.cos(y_) * w[:, 0] + np.sin(y_) * w[:, 1]) / np.cos(p_)
    xd[:, 4] = -np.sin(y_) * w[:, 0] + np.cos(y_) * w[:, 1]
    xd[:, 5] = (np.cos(y_) * w[:, 0] + np.sin(y_) * w[:, 1]) * np.tan(p_) + w[:, 2]
    xd[:, 30:] = qpp
    return xd


@pytest.mark.parametrize("ticks", (1, 2, 3))
@pytest.mark.parametrize("band", SWEEP_BANDS)
def test_short_rollouts_equal_host_rk4_over_plain_evaluations_accelerations_included(consts, band, ticks):
    """1, 2 and 3 ticks from the sweep's states: final state (1e-7), the last tick's tau / f (TOL_REL, weight floor) and the out record's
    accelerations (TOL_REL) against rk4.hpp on the host over lmh_eval; the accelerations must be those lmh_eval returns for the k4 stage
    state of the last tick.  The tolerances are those of the one-tick comparison in tests/test_gpu_posture_sweep.py; every robot counts."""
    q, v, vp = posture_sweep(consts["q0"], B_ROLL, band)
    B = q.shape[0]
    ctl = make_controller(B, DT, TH, consts["zcom"], warm_start=0)
    ctl.set_refs_stance(2.0, 2)
    st = ctl.new_state(q, v, t=0.0, v_prev=vp)
    out, status, log = ctl.rollout(st, ticks, log=True)
    torch.cuda.synchronize()
    assert (status[:, 2] == 0).all(), status.cpu().numpy()
    roll_state, roll_out = st.cpu().numpy(), out.cpu().numpy()
    # host side: four chained plain evaluations per tick; each leaves Robot::v_ (state[:, 60:90]) = its velocity for the next one
    hs = ctl.new_state(q, v, t=0.0, v_prev=vp)
    x0, t, last = np.concatenate([q, v], axis=1), 0.0, None
    for _ in range(ticks):
        ks = []
        for stage, (h, ts) in enumerate(((0.0, t), (0.5 * DT, t + 0.5 * DT), (0.5 * DT, t + 0.5 * DT), (DT, t + DT))):
            xs = x0 if stage == 0 else x0 + h * ks[-1]
            hs[:, :60] = torch.as_tensor(xs).to(hs.device)
            hs[:, 90] = ts
            o, sst = ctl.stand_step(hs)
            torch.cuda.synchronize()
            assert (sst[:, 2] == 0).all()
            last = o.cpu().numpy()
            ks.append(_xdot(xs, last[:, 36:66]))
        x0 = x0 + (DT / 6.0) * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
        t += DT
    worst, bad = dict(state=0.0, tau=0.0, f=0.0, qdd=0.0), []
    for i in range(B):
        worst["state"] = max(worst["state"], vec_err(roll_state[i, :60], x0[i]))
        worst["tau"] = max(worst["tau"], vec_err(roll_out[i, :24], last[i, :24]))
        worst["f"] = max(worst["f"], float(np.abs(roll_out[i, 24:36] - last[i, 24:36]).max() / WEIGHT))
        worst["qdd"] = max(worst["qdd"], vec_err(roll_out[i, 36:66], last[i, 36:66]))
    print("\nband %.1f, %d tick(s): " % (band, ticks) + ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    for i in range(B):
        if not close(roll_state[i, :60], x0[i], 1e-7):
            bad.append((i, "state", vec_err(roll_state[i, :60], x0[i])))
        if not close(roll_out[i, :24], last[i, :24], TOL_REL):
            bad.append((i, "tau", vec_err(roll_out[i, :24], last[i, :24])))
        if not close(roll_out[i, 24:36], last[i, 24:36], TOL_REL, scale=WEIGHT):
            bad.append((i, "f", float(np.abs(roll_out[i, 24:36] - last[i, 24:36]).max())))
        if not close(roll_out[i, 36:66], last[i, 36:66], TOL_REL):
            bad.append((i, "qdd", vec_err(roll_out[i, 36:66], last[i, 36:66])))
    assert np.array_equal(roll_out[:, :36], log.cpu().numpy()[ticks - 1])
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("ticks", (CHUNK - 1, CHUNK, CHUNK + 1))
def test_launch_and_chunk_ends_publish_what_single_tick_launches_publish(consts, ticks):
    """A launch ending one tick before, on and one tick behind the chunk boundary equals, bit for bit, the same ticks run as one launch of
    ticks - 3 followed by three single-tick launches: state (q, v, Robot::v_, t), out record (tau, f, accelerations, CoM, MPC reference)
    and status ([0] k and [3] active set of the last tick, [1] the maximum and [2] the OR over the launches)."""
    B = 96
    v = perturbed_velocities(B, seed=4242)
    ctl = make_controller(B, DT, TH, consts["zcom"], warm_start=1)
    ctl.set_refs_stance(2.0, 2)
    st = ctl.new_state(consts["q0"], v, t=0.0)
    out, status, _ = ctl.rollout(st, ticks)
    torch.cuda.synchronize()
    st2 = ctl.new_state(consts["q0"], v, t=0.0)
    out2, status2 = ctl.new_out(), ctl.new_status()
    itmax = np.zeros(B, dtype=np.int64); flags = np.zeros(B, dtype=np.int64)
    for n in (ticks - 3, 1, 1, 1):
        ctl.rollout(st2, n, out2, status2)
        torch.cuda.synchronize()
        s_ = status2.cpu().numpy()
        itmax = np.maximum(itmax, s_[:, 1]); flags |= s_[:, 2]
    a, b = status.cpu().numpy(), status2.cpu().numpy()
    assert (a[:, 2] == 0).all()
    assert np.isfinite(out.cpu().numpy()[:, :78]).all()
    assert np.array_equal(st.cpu().numpy(), st2.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), out2.cpu().numpy())
    assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 3], b[:, 3])
    assert np.array_equal(a[:, 1], itmax) and np.array_equal(a[:, 2], flags)


def test_non_finite_state_in_a_rollout_is_flagged_and_stays_with_its_robot(consts):
    """The rollout form of test_non_finite_state_is_flagged_not_propagated_silently (which goes through the evaluation kernel): three
    robots, the middle one with a NaN joint velocity, three ticks.  The rollout's guard tests the recovery's registers."""
    from linearmpchumanoid_amd import capi
    ctl = make_controller(3, DT, TH, consts["zcom"])
    ctl.set_refs_stance(2.0, 2)
    v = np.zeros((3, 30)); v[1, 7] = np.nan
    st = ctl.new_state(consts["q0"], v, t=0.0)
    out, status, _ = ctl.rollout(st, 3)
    torch.cuda.synchronize()
    status, out, stn = status.cpu().numpy(), out.cpu().numpy(), st.cpu().numpy()
    assert status[1, 2] & capi.FLAG_NONFINITE
    assert status[0, 2] == 0 and status[2, 2] == 0
    assert np.isfinite(out[0, :78]).all() and np.isfinite(stn[0, :91]).all()
    assert np.array_equal(out[0], out[2]) and np.array_equal(stn[0], stn[2]) and np.array_equal(status[0], status[2])
