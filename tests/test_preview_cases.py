"""CPU checks of the preview-window cases (preview_cases.py), with the oracle alone: at every horizon and every evaluation that
test_gpu_preview_window.py compares, a window that drops its last term or starts one sample late would move the MPC step by at least
1e3 times the tolerance of that comparison; the oracle's evaluations and short rollouts are finite and unflagged; the clamped windows
can be posed to the oracle by padding; the pushed N = 45 rollout has active bounds."""
import numpy as np
import pytest

import preview_cases as pc


def _state(o, B=pc.B_EVAL, pushed=False):
    return o.robot()["q"].copy(), (pc.pushed_velocities(B) if pushed else pc.velocities(B))


def _assert_sensitive(o, mode, k, what, need_last=False):
    """The preconditions at the evaluation the oracle has just made (its CoM and CoM velocity are that evaluation's)."""
    m = pc.MODES[mode]
    K, (Px, _), rb = o.gain_row(), o.mpc_mats(), o.robot()
    zx, zy, _ = pc.zmp_arrays(m["n"])
    S, tol = pc.scales(K, Px, zx, zy, k, rb["CoM"], rb["comVel"], m["mpc_dt"])
    sn = pc.sensitivity(K, zx, zy, k, S)
    assert sn["drop"] >= pc.SENSITIVITY and sn["shift"] >= pc.SENSITIVITY, (what, sn)
    if need_last:
        assert sn["last"] >= pc.SENSITIVITY, (what, sn)
    # the oracle's Cholesky solve and the gain-row form of the same step agree far inside the tolerance: the tolerance is not the oracle's error
    ref = pc.mpc_reference_longdouble(K, Px, zx, zy, k, rb["CoM"], rb["comVel"], m["mpc_dt"])
    assert (np.abs(ref - o.qp()["mpcRef"]).reshape(2, 3) <= 1e-2 * tol).all(), what
    return sn


@pytest.mark.parametrize("mode", list(pc.MODES))
@pytest.mark.parametrize("N", pc.H)
def test_single_evaluations_are_sensitive_finite_and_unflagged(N, mode):
    m = pc.MODES[mode]
    o = pc.make_oracle(N, mode)
    q0, v = _state(o)
    for i in range(pc.B_EVAL):
        e = o.eval(q0, v[i], m["t"])
        assert e["k"] == pc.k_of(m["t"], m["mpc_dt"]) and e["k"] + N < m["n"]
        assert e["qp_status"] == 0 and np.isfinite(e["tau"]).all() and np.isfinite(e["f"]).all()
        _assert_sensitive(o, mode, e["k"], (N, mode, i), need_last=(N == 64))


@pytest.mark.parametrize("mode", list(pc.MODES))
@pytest.mark.parametrize("N", pc.H)
def test_short_rollouts_are_finite_and_unflagged(N, mode):
    m = pc.MODES[mode]
    o = pc.make_oracle(N, mode)
    q0, v = _state(o)
    ks = pc.k4_sequence(pc.ROLLOUT_TICKS, m["mpc_dt"])
    for i in range(pc.B_EVAL):
        o.set_prev_velocity(np.zeros(30))
        r = o.rollout(np.concatenate([q0, v[i]]), 0.0, pc.ROLLOUT_TICKS, dt=pc.DT, log=True)
        assert np.isfinite(r["state"]).all() and np.isfinite(r["log"]).all() and r["info"][3] == 0
        assert list(r["k"]) == ks
        if N in pc.H_ROLLOUT:                                      # the last tick's x_ref / y_ref is compared on the GPU
            _assert_sensitive(o, mode, ks[-1], (N, mode, i, "rollout"), need_last=(N == 64))
    # coupled: k moves every tick; decoupled: the references are refreshed on every 10th tick only
    assert len(set(ks)) == (pc.ROLLOUT_TICKS if mode == "coupled" else 3)


@pytest.mark.parametrize("mode", list(pc.MODES))
def test_pushed_rollout_at_the_lds_seam_has_active_bounds(mode):
    """N = 45 with the 0.15 m/s push: on at least one tick the contact QP's active set is not empty, so the warm start's K_f^-1 block
    -- which starts where the N = 45 gain record ends -- is live in the kernel."""
    m = pc.MODES[mode]
    o = pc.make_oracle(45, mode)
    q0, v = _state(o, pushed=True)
    assert np.allclose(np.hypot(v[:, 0], v[:, 1]), 0.15)
    for i in range(pc.B_EVAL):
        o.set_prev_velocity(np.zeros(30))
        st, t, masks = np.concatenate([q0, v[i]]), 0.0, []
        for _ in range(pc.ROLLOUT_TICKS):                          # tick by tick: the oracle carries Robot::v_ between the calls
            r = o.rollout(st, t, 1, dt=pc.DT)
            st, t = r["state"], r["t"]
            assert r["info"][3] == 0 and np.isfinite(st).all()
            masks.append(int(np.uint32(r["info"][4])))
        assert any(masks), (mode, i)
    _assert_sensitive(o, mode, pc.k4_sequence(pc.ROLLOUT_TICKS, m["mpc_dt"])[-1], (45, mode, "pushed"))


@pytest.mark.parametrize("mode", list(pc.MODES))
@pytest.mark.parametrize("N", pc.H_ZCOM)
def test_per_robot_heights_are_sensitive(N, mode):
    m = pc.MODES[mode]
    rows = []
    for i, z in enumerate(pc.ZCOMS):
        o = pc.make_oracle(N, mode, zcom=z)
        q0, v = _state(o)
        rows.append(o.gain_row())
        e = o.eval(q0, v[i], m["t"])
        assert e["qp_status"] == 0
        _assert_sensitive(o, mode, e["k"], (N, mode, z), need_last=(N == 64))
        o.set_prev_velocity(np.zeros(30))
        r = o.rollout(np.concatenate([q0, v[i]]), 0.0, pc.ZCOM_TICKS, dt=pc.DT, log=True)
        assert np.isfinite(r["state"]).all() and r["info"][3] == 0
        _assert_sensitive(o, mode, pc.k4_sequence(pc.ZCOM_TICKS, m["mpc_dt"])[-1], (N, mode, z, "rollout"), need_last=(N == 64))
    # the rows differ by far more than the 1e-10 they are compared at: a robot reading its neighbour's row would be seen
    assert min(np.abs(rows[a] - rows[b]).max() / np.abs(rows[b]).max() for a in range(3) for b in range(3) if a != b) > 1e-3


def test_the_clock_enters_a_standing_evaluation_through_k_alone():
    """What lets a clamped evaluation be posed to the oracle at another clock: two clocks inside one sample give the same bits."""
    o = pc.make_oracle(17, "coupled")
    q0, v = _state(o)
    a = o.eval(q0, v[0], 0.0571)
    o.set_prev_velocity(np.zeros(30))
    b = o.eval(q0, v[0], 0.0579)
    assert a["k"] == b["k"] == 57
    assert np.array_equal(a["tau"], b["tau"]) and np.array_equal(a["f"], b["f"]) and np.array_equal(a["qpp"], b["qpp"])


def test_front_clamp_index_truncates_towards_zero():
    """(int)(t / mpc_dt) at t = -0.0035: -3 on the 1 ms grid (clamped at the front), 0 on the 10 ms grid (in range: no clamp there)."""
    assert pc.k_of(pc.T_FRONT, 1e-3) == -3 and pc.k_of(pc.T_FRONT, 1e-2) == 0
    assert int(np.trunc(np.float64(pc.T_FRONT) / np.float64(1e-3))) == -3


@pytest.mark.parametrize("N,mode,where,t", pc.clamp_cases())
def test_clamped_windows_posed_to_the_oracle(N, mode, where, t):
    m = pc.MODES[mode]
    o, t_o, k = pc.clamp_oracle(N, mode, where, t)
    assert (k < 0) if where == "front" else (k + N == m["n"] - 1 + pc.PAST_END)
    q0, v = _state(o)
    zx, zy, _ = pc.zmp_arrays(m["n"])
    K, (Px, _) = o.gain_row(), o.mpc_mats()
    for i in range(pc.B_EVAL):
        o.set_prev_velocity(np.zeros(30))
        e = o.eval(q0, v[i], t_o)
        assert e["qp_status"] == 0 and e["k"] == k + max(0, -k)
        rb = o.robot()
        # the padded oracle reads the window the clamp reads: its x_ref / y_ref is the numpy statement of the clamp
        S, tol = pc.scales(K, Px, zx, zy, k, rb["CoM"], rb["comVel"], m["mpc_dt"])
        ref = pc.mpc_reference_longdouble(K, Px, zx, zy, k, rb["CoM"], rb["comVel"], m["mpc_dt"])
        assert (np.abs(ref - o.qp()["mpcRef"]).reshape(2, 3) <= 1e-2 * tol).all()
        sn = pc.sensitivity(K, zx, zy, k, S)
        assert sn["drop"] >= pc.SENSITIVITY and sn["shift"] >= pc.SENSITIVITY, sn
        # and the clamp matters: the clamped terms carry far more than a tolerance, so reading anything else there would be seen
        idx = k + np.arange(N + 1)
        out = (idx < 0) | (idx >= m["n"])
        assert out.sum() == (3 if where == "front" else pc.PAST_END)
        assert max(abs(K[out] @ pc.window(z, k, N)[out]) / (pc.TOL_WINDOW * S[ax]) for ax, z in enumerate((zx, zy))) >= pc.SENSITIVITY
