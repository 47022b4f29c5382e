"""GPU tests of the MPC preview window (refs_prepare, load_common, refs_chain_a) at the horizons where its code changes path, on ZMP
references that differ at every sample: gain rows at every N = 1 .. 64, single evaluations and short rollouts either side of the
on-chip / in-memory gain record (N = 45 | 46) and of the second trip of the window loop (N = 64), per-robot gain rows across that seam,
and the VALUES of the clamped window.  preview_cases.py holds the cases; test_preview_cases.py has checked on the CPU that a dropped
last term or a window shifted by one sample moves the compared numbers by at least 1e3 tolerances in every case below.

x_ref | y_ref (out[72:78]) are compared within 1e-11 * S, S the size of the terms of u = -K (Px x - z) (preview_cases.scales);
tau and f at the suite's 1e-6; k exactly."""
import numpy as np
import pytest
import torch

import preview_cases as pc
from helpers import TOL_REL, WEIGHT, close, horizon_controller, rel_err

pytestmark = pytest.mark.gpu
MODE_IDS = list(pc.MODES)


def mode_controller(B, N, mode, zcom, **kw):
    m = pc.MODES[mode]
    ctl = horizon_controller(B, N, zcom, m["mpc_dt"], pc.DT, **kw)
    assert ctl.N == N
    zx, zy, ph = pc.zmp_arrays(m["n"])
    ctl.set_refs(zx, zy, ph)
    return ctl


@pytest.fixture(scope="module")
def nao():
    o = pc.make_oracle(16, "coupled")
    return dict(zcom=o.zcom, q0=o.robot()["q"].copy())


def _window_ratio(x6, o, mode, k):
    """Worst |x_ref | y_ref - oracle| in units of its tolerance, at the evaluation the oracle has just made; k is the kernel's index
    into the unpadded arrays."""
    m = pc.MODES[mode]
    K, (Px, _), rb = o.gain_row(), o.mpc_mats(), o.robot()
    zx, zy, _ = pc.zmp_arrays(m["n"])
    _, tol = pc.scales(K, Px, zx, zy, k, rb["CoM"], rb["comVel"], m["mpc_dt"])
    return float((np.abs(np.asarray(x6) - o.qp()["mpcRef"]).reshape(2, 3) / tol).max())


def _check_eval(out, status, o, e, mode, k, flags=0):
    assert status[0] == k and status[2] == flags, (status, k)
    ratio = _window_ratio(out[72:78], o, mode, k)
    assert ratio <= 1.0, ratio
    assert rel_err(out[:24], e["tau"]) < TOL_REL and rel_err(out[24:36], e["f"]) < TOL_REL
    return ratio


def _check_rollout(stn, out, status, log, o, q0, v, mode, nt):
    """One robot's rollout against Oracle.rollout(dt = 1 ms): k of the launch, tau / f of every 3rd tick, the final state, and the last
    tick's x_ref / y_ref.  -> that last ratio."""
    m = pc.MODES[mode]
    o.set_prev_velocity(np.zeros(30))
    r = o.rollout(np.concatenate([q0, v]), 0.0, nt, dt=pc.DT, log=True)
    ks = pc.k4_sequence(nt, m["mpc_dt"])
    assert list(r["k"]) == ks and status[0] == ks[-1] and status[2] == 0, (status, ks[-1])
    for tk in range(0, nt, 3):
        ref = r["log"][tk]
        assert close(log[tk, :24], ref[:24], TOL_REL), tk
        assert close(log[tk, 24:], ref[24:], TOL_REL, scale=WEIGHT), tk
    assert close(stn[:60], r["state"], 1e-7)
    ratio = _window_ratio(out[72:78], o, mode, ks[-1])
    assert ratio <= 1.0, ratio
    return ratio


# ------------------------------------------------------------------------------- 1. gain rows
@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("first", (1, 17, 33, 49))
def test_gain_row_at_every_horizon(nao, first, mode):
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    from oracle.pyoracle import Oracle
    mpc_dt = pc.MODES[mode]["mpc_dt"]
    worst = 0.0
    for N in range(first, first + 16):
        th = pc.horizon_time(N, mpc_dt)
        ctl = BatchedController(1, default_config(dt=pc.DT, time_horizon=th, z_com=nao["zcom"], mpc_dt=mpc_dt))
        o = Oracle(sim_time=1.0, dt=mpc_dt, horizon_time=th, do_ik=False)
        o.set_zcom(nao["zcom"])
        assert ctl.N == N == o.horizon
        K, Ko = ctl.mpc_gain(), o.gain_row()
        ctl.close()
        assert K.shape == (N + 1,)
        worst = max(worst, rel_err(K, Ko))
        assert rel_err(K, Ko) < 1e-10, (N, rel_err(K, Ko))
    print(f"\ngain rows N = {first} .. {first + 15}, {mode}: worst rel err {worst:.2e}")


# ------------------------------------------------------------------------------- 2. single evaluations
@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("N", pc.H)
def test_single_evaluation_on_a_varying_window(nao, N, mode):
    m = pc.MODES[mode]
    v = pc.velocities(pc.B_EVAL)
    ctl = mode_controller(pc.B_EVAL, N, mode, nao["zcom"], warm_start=0)
    st = ctl.new_state(nao["q0"], v, t=m["t"])
    out, status = ctl.stand_step(st)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    ctl.close()
    o = pc.make_oracle(N, mode)
    assert abs(o.zcom - nao["zcom"]) == 0.0
    worst = 0.0
    for i in range(pc.B_EVAL):
        o.set_prev_velocity(np.zeros(30))
        e = o.eval(nao["q0"], v[i], m["t"])
        worst = max(worst, _check_eval(out[i], status[i], o, e, mode, e["k"]))
    print(f"\npreview window N = {N}, {mode}: worst x_ref / y_ref error {worst:.3f} tolerances")


# ------------------------------------------------------------------------------- 3. short rollouts
ROLLOUTS = [(N, False) for N in pc.H_ROLLOUT] + [(45, True)]


@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("N,pushed", ROLLOUTS, ids=[f"{N}{'-pushed' if p else ''}" for N, p in ROLLOUTS])
def test_short_rollout_on_a_varying_window(nao, N, pushed, mode):
    """25 warm-started ticks: coupled, k moves every tick; decoupled, the cached references are refreshed on every 10th.  The pushed
    N = 45 case has active bounds (test_preview_cases.py), so the K_f^-1 block that starts where the N = 45 gain record ends is live."""
    nt = pc.ROLLOUT_TICKS
    v = pc.pushed_velocities(pc.B_EVAL) if pushed else pc.velocities(pc.B_EVAL)
    ctl = mode_controller(pc.B_EVAL, N, mode, nao["zcom"], warm_start=1)
    st = ctl.new_state(nao["q0"], v, t=0.0)
    out, status, log = ctl.rollout(st, nt, log=True)
    torch.cuda.synchronize()
    stn, out, status, log = st.cpu().numpy(), out.cpu().numpy(), status.cpu().numpy(), log.cpu().numpy()
    ctl.close()
    o = pc.make_oracle(N, mode)
    worst = max(_check_rollout(stn[i], out[i], status[i], log[:, i], o, nao["q0"], v[i], mode, nt) for i in range(pc.B_EVAL))
    print(f"\npreview window rollout N = {N}{' pushed' if pushed else ''}, {mode}: last tick's x_ref / y_ref error {worst:.3f} tolerances")


# ------------------------------------------------------------------------------- 4. per-robot gain rows across the seam
@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("N", pc.H_ZCOM)
def test_per_robot_gain_rows_across_the_seam(nao, N, mode):
    m = pc.MODES[mode]
    B = len(pc.ZCOMS)
    v = pc.velocities(B)
    worst = 0.0
    ctl = mode_controller(B, N, mode, nao["zcom"], warm_start=0)
    ctl.set_zcom(np.array(pc.ZCOMS))
    st = ctl.new_state(nao["q0"], v, t=m["t"])
    out, status = ctl.stand_step(st)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    ctl.close()
    oracles = [pc.make_oracle(N, mode, zcom=z) for z in pc.ZCOMS]
    for i, o in enumerate(oracles):
        e = o.eval(nao["q0"], v[i], m["t"])
        worst = max(worst, _check_eval(out[i], status[i], o, e, mode, e["k"]))
    ctl = mode_controller(B, N, mode, nao["zcom"], warm_start=1)
    ctl.set_zcom(np.array(pc.ZCOMS))
    st = ctl.new_state(nao["q0"], v, t=0.0)
    out, status, log = ctl.rollout(st, pc.ZCOM_TICKS, log=True)
    torch.cuda.synchronize()
    stn, out, status, log = st.cpu().numpy(), out.cpu().numpy(), status.cpu().numpy(), log.cpu().numpy()
    ctl.close()
    for i, o in enumerate(oracles):
        worst = max(worst, _check_rollout(stn[i], out[i], status[i], log[:, i], o, nao["q0"], v[i], mode, pc.ZCOM_TICKS))
    print(f"\nper-robot gain rows N = {N}, {mode}: worst x_ref / y_ref error {worst:.3f} tolerances")


# ------------------------------------------------------------------------------- 5. the clamp's values
@pytest.mark.parametrize("N,mode,where,t", pc.clamp_cases(), ids=[f"{N}-{mode}-{where}" for N, mode, where, _ in pc.clamp_cases()])
def test_clamped_window_values(nao, N, mode, where, t):
    """The window leaves the arrays: the kernel pins every index to them and raises FLAG_ZMP_RANGE.  The oracle gets the same arrays
    padded by repeating the end sample and the clock of an in-range sample with the same window (preview_cases.clamp_oracle)."""
    from linearmpchumanoid_amd import capi
    v = pc.velocities(pc.B_EVAL)
    ctl = mode_controller(pc.B_EVAL, N, mode, nao["zcom"], warm_start=0)
    st = ctl.new_state(nao["q0"], v, t=t)
    out, status = ctl.stand_step(st)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    ctl.close()
    o, t_o, k = pc.clamp_oracle(N, mode, where, t)
    worst = 0.0
    for i in range(pc.B_EVAL):
        o.set_prev_velocity(np.zeros(30))
        e = o.eval(nao["q0"], v[i], t_o)
        worst = max(worst, _check_eval(out[i], status[i], o, e, mode, k, flags=capi.FLAG_ZMP_RANGE))
    print(f"\nclamped window N = {N}, {mode}, {where} (k = {k}): worst x_ref / y_ref error {worst:.3f} tolerances")
