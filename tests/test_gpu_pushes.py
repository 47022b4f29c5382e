"""Timed per-robot velocity pushes inside lmh_rollout (lmh_set_pushes): a launch with the schedule set against a host that stops the
launch at every push tick and adds dv to state[:, 30:60] itself, launch splitting, shared against per-robot schedules, the setters, and
the CPU oracle pushed the same way.  Scenarios and the split-launch host: tests/push_cases.py.  "The same computation" means
bit-identical (compared as bytes); parity with the oracle is helpers.close's 1e-6 relative on
tau / f and on the final state, k bit-exact."""
import os

import numpy as np
import pytest
import torch

from helpers import WEIGHT, close, run_probe, vec_err
from push_cases import WALK_B, WALK_NT, Run, bits_differ, in_kernel_against_split, walking_controller, walking_pushes

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from linearmpchumanoid_amd import capi
from push_cases import in_kernel_against_split
res = in_kernel_against_split(precision=int(sys.argv[1]), plant=int(sys.argv[2]))
res["build_flags"] = capi.lib().lmh_debug_build_flags()
print(json.dumps(res))
"""


def check_in_kernel_result(res, precision, plant):
    print("in-kernel against split launches:", precision, plant, res)
    assert res["launches"] > 100                                    # the host really stopped at (nearly) every drawn tick
    assert res["finite"] and res["nonfinite_robots"] == 0           # numbers are compared, not NaNs
    assert res["robots_moved"] == res["robots_pushed"] >= WALK_B - 2      # the pushes changed exactly the robots that got one inside the launch
    assert res["diff_never"] == [] and res["next_applied"]          # pushes at ticks >= 1000: absent from the 1000-tick launch, applied by the next
    if precision == 0 and plant == 0:
        assert res["flags"] == 0                                    # the reference loop in fp64: nobody falls over a 0.05 m/s kick
    assert res["diff"] == [], res
    assert res["diff_next"] == [], res


# ------------------------------------------------------------------------------- 1. in-kernel = split launches, bit for bit
@pytest.mark.parametrize("plant", [0, 1])
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("build", ["shipped", "poison"])
def test_in_kernel_pushes_equal_split_launches_bit_for_bit(build, precision, plant):
    """64 robots on the mixed per-robot walking plan, three pushes each (the draw with the corner cases of push_cases.EDGE_TICKS: ticks
    0, 250, 500, 249-250-251, 999, 1000, 5000), one 1000-tick launch with the schedule set.  Reference: a handle without a schedule run
    launch by launch between the sorted distinct push ticks, the host adding each dv to its robot's state[30:60]: state, out, status [0]
    and [3] and the log identical, [1] / [2] merged as max / OR.  Then one more tick on both: the pushes at tick 1000, which the first
    launch's record must not hold, are applied by the launch that starts there; the robot whose pushes all lie at or beyond tick 1000 is
    an unpushed robot inside the first launch.  In every precision, with and without the plant, and on the checker build that fills
    every robot's LDS with NaNs first (a fresh child process; lmh_debug_build_flags bit 0 says which library ran).  The rollout kernel
    has no single-wave schedule, so there is no such case.
    With the plant the 64 robots stand on the compliant contact instead of walking (push_cases.scenario_controller says why); in
    every case no robot may be non-finite anywhere."""
    if build == "shipped":
        res = in_kernel_against_split(precision=precision, plant=plant)
    else:
        from linearmpchumanoid_amd import build as hipbuild
        assert os.path.exists(hipbuild.build_variant("poison", ["-DLMH_POISON"]))
        res = run_probe(_CHILD, "poison", timeout=900, args=(str(precision), str(plant)))
        assert res["build_flags"] & 1 == 1, res
    check_in_kernel_result(res, precision, plant)


# ------------------------------------------------------------------------------- 2. launch splitting
def test_split_launch_with_pushes_is_the_whole_launch():
    """rollout(400) followed by rollout(600) equals rollout(1000) with the same schedule, bit for bit: the push cursor is rebuilt from the
    robot's clock, and the second launch ignores what lies in its past."""
    ticks, dv = walking_pushes()
    ticks[12] = (399, 400, 401)                                     # around the split
    ctl, q0 = walking_controller()
    ctl.set_pushes(ticks, dv)
    whole = Run(ctl, q0)
    whole.launch(WALK_NT)
    parts = Run(ctl, q0)
    parts.launch(400)
    parts.launch(WALK_NT - 400)
    ctl.close()
    a, b = whole.result(), parts.result()
    assert np.isfinite(a["log"]).all()
    assert bits_differ(a, b) == []


# ------------------------------------------------------------------------------- 3. shared and per-robot schedules
def test_shared_schedule_is_that_schedule_per_robot_and_unused_records_push_nothing():
    ticks, dv = walking_pushes()
    res = {}
    for name in ("shared", "repeated", "mixed", "none"):
        ctl, q0 = walking_controller()
        if name == "shared":
            ctl.set_pushes(ticks[20], dv[20])
            assert not ctl.pushes_per_instance
        elif name == "repeated":
            ctl.set_pushes(np.tile(ticks[20], (WALK_B, 1)), np.tile(dv[20], (WALK_B, 1, 1)))
            assert ctl.pushes_per_instance
        elif name == "mixed":                                       # every third robot's records are all unused
            tk = ticks.copy(); tk[::3] = -1
            ctl.set_pushes(tk, dv)
        else:
            assert not ctl.pushes_per_instance and ctl.get_pushes(3)["ticks"].size == 0
        r = Run(ctl, q0)
        r.launch(600)
        res[name] = r.result()
        ctl.close()
    assert bits_differ(res["shared"], res["repeated"]) == []
    assert bits_differ(res["shared"], res["none"]) != []            # ... and it pushes
    rows = np.arange(0, WALK_B, 3)
    assert bits_differ(res["mixed"], res["none"], rows=rows) == []
    moved = np.abs(res["mixed"]["state"][:, :60] - res["none"]["state"][:, :60]).max(axis=1) > 0
    tk[::3] = 5000                                                  # (unused = never)
    assert np.array_equal(moved, (tk < 600).any(axis=1)) and moved.sum() > WALK_B // 2      # exactly the robots with a push inside the launch


# ------------------------------------------------------------------------------- 4. setters
def test_push_setters_refuse_whole_and_clear_exactly():
    """A refused lmh_set_pushes leaves the previous schedule in place (read back with lmh_get_pushes, and the rollout repeats bit for
    bit); every refusal names its reason and the first offending robot; clearing restores the unpushed result; get_pushes round-trips."""
    from linearmpchumanoid_amd import capi, trajectories
    from linearmpchumanoid_amd.capi import LmhError
    ticks, dv = walking_pushes()
    ctl, q0 = walking_controller()

    def run600():
        r = Run(ctl, q0)
        r.launch(600)
        return r.result()

    unpushed = run600()
    ctl.set_pushes(ticks, dv)
    assert ctl.pushes_per_instance and capi.lib().lmh_num_pushes(ctl._h) == 3
    rec = trajectories.push_schedule(ticks, dv)
    for i in (0, 7, 31, WALK_B - 1):                                # round trip: sorted by tick, dv bit for bit
        g = ctl.get_pushes(i)
        assert np.array_equal(g["ticks"], rec[i, :, 0].astype(np.int64)) and g["dv"].tobytes() == rec[i, :, 1:31].tobytes(), i
    pushed = run600()
    assert bits_differ(pushed, unpushed) != []

    def raw(records, n_push=None, n_sets=None):
        r = np.ascontiguousarray(records, dtype=np.float64)
        return capi.lib().lmh_set_pushes(ctl._h, r.ctypes.data_as(capi.C.c_void_p), r.shape[1] if n_push is None else n_push,
                                         r.shape[0] if n_sets is None else n_sets)

    cases = []
    bad = rec.copy(); bad[7, 1, 0] += 0.5; cases.append((bad, {}, "robot 7: " + trajectories.PUSH_ERR_TICK))
    bad = rec.copy(); bad[9, 0, 0] = -3.0; cases.append((bad, {}, "robot 9: " + trajectories.PUSH_ERR_TICK))
    bad = rec.copy(); bad[5, 2, 0] = bad[5, 1, 0]; cases.append((bad, {}, "robot 5: " + trajectories.PUSH_ERR_INCREASING))
    bad = rec.copy(); bad[6, 1, 0] = -1.0; cases.append((bad, {}, "robot 6: " + trajectories.PUSH_ERR_ORDER))
    bad = rec.copy(); bad[63, 2, 30] = np.nan; cases.append((bad, {}, "robot 63: " + trajectories.PUSH_ERR_DV))
    bad = rec.copy(); bad[2, 0, 1] = np.inf; bad[40, 0, 0] = 0.25; cases.append((bad, {}, "robot 2: " + trajectories.PUSH_ERR_DV))   # the FIRST offender
    cases.append((np.zeros((1, capi.MAX_PUSHES + 1, capi.PUSH_STRIDE)), {}, trajectories.PUSH_ERR_COUNT))
    cases.append((rec[:5], {}, trajectories.PUSH_ERR_SETS))
    for records, kw, msg in cases:
        assert raw(records, **kw) == -2
        assert capi.lib().lmh_last_error().decode() == msg, msg
        with pytest.raises(ValueError) as e:                       # the host statement refuses the same table in the same words
            trajectories.check_push_records(records, n_instances=WALK_B)
        assert str(e.value) == msg
        assert ctl.pushes_per_instance and capi.lib().lmh_num_pushes(ctl._h) == 3
        for i in (0, 7, WALK_B - 1):
            assert ctl.get_pushes(i)["dv"].tobytes() == rec[i, :, 1:31].tobytes()
    with pytest.raises(LmhError):
        ctl.get_pushes(WALK_B)
    assert bits_differ(run600(), pushed) == []                      # the schedule in place is still the one that runs
    ctl.set_pushes(None)
    assert not ctl.pushes_per_instance and capi.lib().lmh_num_pushes(ctl._h) == 0 and ctl.get_pushes(0)["ticks"].size == 0
    assert bits_differ(run600(), unpushed) == []
    ctl.set_pushes(ticks[3], dv[3])                                 # shared; every robot reads the one set
    assert not ctl.pushes_per_instance
    assert np.array_equal(ctl.get_pushes(17)["ticks"], np.sort(ticks[3]))
    # plain evaluations do not integrate and ignore the schedule (ticks[0] holds tick 0)
    ctl.set_pushes(ticks, dv)
    st = ctl.new_state(q0, np.zeros(30), t=0.0)
    o1, _ = ctl.stand_step(st.clone())
    ctl.set_pushes(None)
    o2, _ = ctl.stand_step(st.clone())
    torch.cuda.synchronize()
    assert o1.cpu().numpy().tobytes() == o2.cpu().numpy().tobytes()
    ctl.close()


# ------------------------------------------------------------------------------- 5. oracle parity
ORC_B, ORC_NT, ORC_SEED, ORC_AMP = 32, 500, 20261018, 0.1
ORC_DT, ORC_MPC_DT, ORC_N = 1e-3, 2e-2, 16                        # bench.py's config 2: 1 kHz control, 16 x 20 ms preview, stance references
BAND_TILT, BAND_Z = 0.2, 0.03                                      # upright band: |roll|, |pitch| [rad], |base z - start| [m]


def balance_pushes():
    from linearmpchumanoid_amd import trajectories
    return trajectories.draw_pushes(ORC_B, 2, (20, 200), ORC_AMP, ORC_SEED)


class _StandStep:
    """Oracle.eval under the name restatement_np.rk4_tick calls (Controller::standStep; it keeps Robot::v_ like the reference)."""

    def __init__(self, o):
        self.o = o

    def stand_step(self, q, dq, t):
        return self.o.eval(q, dq, t)


def oracle_pushed(q0, ticks, dv, nt=ORC_NT):
    """One robot in the CPU oracle, tick by tick: Oracle.rollout of one tick at a time with dv added to the state between the ticks, the
    posture and the QP status looked at after every tick.  The LAST tick is taken by hand -- rk4Step over Oracle.eval
    (oracle/restatement_np.rk4_tick) -- so that the fourth stage's evaluation, which is what lmh_rollout leaves in d_out, is at hand
    with its accelerations.  -> dict(log [nt,36], k [nt], state [60], qpp [30] of that evaluation, worst_tilt, worst_dz, qp_status_seen)."""
    from oracle.pyoracle import Oracle
    from oracle.restatement_np import rk4_tick
    o = Oracle(sim_time=nt * ORC_DT + 1.0, dt=ORC_MPC_DT, horizon_time=ORC_N * ORC_MPC_DT + 1e-9, do_ik=True)
    state, t = np.concatenate([q0, np.zeros(30)]), 0.0
    log, ks, tilt, dz, bad, qpp = np.zeros((nt, 36)), np.zeros(nt, np.int64), 0.0, 0.0, 0, None
    for n in range(nt):
        for j in np.flatnonzero(np.asarray(ticks) == n):
            state = state.copy(); state[30:60] += dv[j]
        if n < nt - 1:
            r = o.rollout(state, t, 1, dt=ORC_DT, log=True)
            state, t, log[n], ks[n] = r["state"], r["t"], r["log"][0], r["k"][0]
            bad |= int(r["info"][3] != 0)
        else:
            state, e = rk4_tick(_StandStep(o), state, t, ORC_DT)
            log[n, :24], log[n, 24:], ks[n], qpp = e["tau"], e["f"], e["k"], e["qpp"].copy()
            bad |= int(e["qp_status"] != 0)
            t += ORC_DT
        tilt = max(tilt, float(np.abs(state[3:5]).max())); dz = max(dz, float(abs(state[2] - q0[2])))
    o.close()
    return dict(log=log, k=ks, state=state, qpp=qpp, worst_tilt=tilt, worst_dz=dz, qp_status_seen=bad)


def test_pushed_balance_against_the_oracle():
    """Balance task on bench.py's config-2 settings (dt = 1 ms, N = 16 x mpc_dt = 20 ms, stance references, warm start, zero initial
    velocity), 32 robots, two planar pushes each of at most 0.1 m/s per axis at ticks of [20, 200) (trajectories.draw_pushes, seed
    20261018), 500 ticks: at least 300 after the last push.  The oracle is Oracle.rollout tick by tick with dv added between the ticks
    (oracle_pushed).  tau and f of EVERY tick through the log, the accelerations of the last tick (out[:, 36:66], the fourth stage's
    evaluation) and the final state within helpers.close's 1e-6 relative, k of the launch's last evaluation bit-exact, no flag.  The log
    record is tau | f, so the accelerations of the other ticks have no record of their own; they are what the state integrates.
    Condition on the inputs, asserted here on the oracle alone before anything runs on the GPU: no robot of the draw reports a QP
    failure after any tick or leaves the upright band |roll|, |pitch| <= 0.2 rad, |base z - start| <= 0.03 m after any tick (this draw:
    0.067 rad and 3.7 mm at worst).  No case is skipped."""
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    from concurrent.futures import ThreadPoolExecutor
    from oracle.pyoracle import Oracle
    o = Oracle(sim_time=1.0, dt=ORC_MPC_DT, horizon_time=ORC_N * ORC_MPC_DT + 1e-9, do_ik=True)
    q0, zcom = o.robot()["q"].copy(), o.zcom                        # the IK start posture and its CoM height, as apps/offline/main.cpp:24-39
    o.close()
    ticks, dv = balance_pushes()
    assert np.abs(dv).max() <= ORC_AMP and ticks.max() < ORC_NT - 300
    with ThreadPoolExecutor(max_workers=8) as ex:
        refs = list(ex.map(lambda i: oracle_pushed(q0, ticks[i], dv[i]), range(ORC_B)))
    for i, r in enumerate(refs):
        assert r["qp_status_seen"] == 0 and r["worst_tilt"] <= BAND_TILT and r["worst_dz"] <= BAND_Z, (i, r["worst_tilt"], r["worst_dz"])
    ctl = BatchedController(ORC_B, default_config(dt=ORC_DT, time_horizon=ORC_N * ORC_MPC_DT + 1e-9, z_com=zcom, mpc_dt=ORC_MPC_DT, warm_start=1))
    ctl.set_refs_stance(ORC_NT * ORC_DT + 1.0, 2)
    ctl.set_pushes(ticks, dv)
    run = Run(ctl, q0)
    run.launch(ORC_NT)
    ctl.close()
    g = run.result()
    assert (g["status"][:, 2] == 0).all(), g["status"][:, 2]
    worst = dict(tau=0.0, f=0.0, state=0.0, qdd=0.0)
    for i, r in enumerate(refs):
        assert g["status"][i, 0] == r["k"][-1], i
        worst["state"] = max(worst["state"], vec_err(g["state"][i, :60], r["state"]))
        worst["qdd"] = max(worst["qdd"], vec_err(g["out"][i, 36:66], r["qpp"]))
        for tk in range(ORC_NT):
            worst["tau"] = max(worst["tau"], vec_err(g["log"][tk, i, :24], r["log"][tk, :24]))
            worst["f"] = max(worst["f"], float(np.abs(g["log"][tk, i, 24:] - r["log"][tk, 24:]).max() / WEIGHT))
    print("pushed balance against the oracle, worst relative errors:", worst)
    for i, r in enumerate(refs):
        assert close(g["state"][i, :60], r["state"]), (i, vec_err(g["state"][i, :60], r["state"]))
        assert close(g["out"][i, 36:66], r["qpp"]), (i, vec_err(g["out"][i, 36:66], r["qpp"]))
        for tk in range(ORC_NT):
            assert close(g["log"][tk, i, :24], r["log"][tk, :24]), (i, tk)
            assert close(g["log"][tk, i, 24:], r["log"][tk, 24:], scale=WEIGHT), (i, tk)
