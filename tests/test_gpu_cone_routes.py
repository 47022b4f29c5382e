"""The push-through cone solve's multipliers and qv come from row-broadcast chains in registers.  These runs drive the routes of the
cone QP that those chains feed and compare every logged tick with the CPU oracle: the all-free solve (standing), the push-through
solve with one foot unused (single support), the edge-contact push-through after a touch-down (double support on a sole edge), and
the register / general routes (qv read from LDS) that pushed robots fall into."""
import numpy as np
import pytest
import torch

from helpers import TOL_REL, WEIGHT, close, oracle_system, start_posture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def consts():
    return start_posture(oracle_system(1e-3, 0.032))


def _check_against_oracle(stn, log, status, nt, make_oracle, v0):
    for i in range(stn.shape[0]):
        o = make_oracle(i)
        r = o.rollout(np.concatenate([v0[i][0], v0[i][1]]), 0.0, nt, log=True)
        assert status[i, 0] == r["k"][-1]
        assert close(stn[i, :60], r["state"], 1e-7), i
        for tk in range(0, nt, 5):
            ref = r["log"][tk]
            assert close(log[tk, i, :24], ref[:24], TOL_REL), (i, tk)
            assert close(log[tk, i, 24:], ref[24:], TOL_REL, scale=WEIGHT), (i, tk)


def test_walking_through_two_touch_downs_against_oracle(consts):
    """Single support (one foot unused) and the double support after each touch-down (edge contact), 4 step lengths, 900 ticks."""
    from linearmpchumanoid_amd import trajectories
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    from oracle.pyoracle import Oracle
    dt, N, nt = 1e-3, 32, 900
    th = N * dt
    plan = trajectories.walk_plan(2.0, dt, num_steps=3, time_per_step=0.4, ds_time=0.1, step_height=0.02, settle_time=0.15)
    xs = np.array([0.02, 0.03, 0.04, 0.05])
    B = len(xs)
    ctl = BatchedController(B, default_config(dt=dt, time_horizon=th, z_com=consts["zcom"], warm_start=1))
    ctl.set_refs(plan["zmp_x"], plan["zmp_y"], plan["phase"])
    ctl.set_segments(plan["segs"], plan["seg_of_sample"])
    ctl.set_xscale(xs)
    st = ctl.new_state(consts["q0"], np.zeros(30), t=0.0)
    out, status, log = ctl.rollout(st, nt, log=True)
    torch.cuda.synchronize()
    stn, log, status = st.cpu().numpy(), log.cpu().numpy(), status.cpu().numpy()
    assert (status[:, 2] == 0).all()

    def make_oracle(i):
        o = Oracle(sim_time=2.0, dt=dt, horizon_time=th, do_ik=True)
        o.set_zcom(consts["zcom"])
        o.set_refs(plan["zmp_x"], plan["zmp_y"], plan["phase"])
        o.set_segments(plan["segs"], plan["seg_of_sample"], xscale=float(xs[i]))
        return o

    _check_against_oracle(stn, log, status, nt, make_oracle, [(consts["q0"], np.zeros(30))] * B)
    single = np.abs(log[:, :, 24 + 6:24 + 12]).max(axis=2) == 0.0
    assert single.any() and (~single).any()                      # both support phases were met


@pytest.mark.parametrize("push", [(0.15, 0.0), (-0.15, 0.0), (0.0, 0.15), (0.0, -0.15)], ids=["x+", "x-", "y+", "y-"])
def test_pushed_standing_robot_against_oracle(consts, push):
    """Standing on both feet, cold start, pushed forward, backward and to either side: the all-free solve, then whichever of the
    push-through, edge-contact and register routes the centre of pressure moving over the soles leads to."""
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    from oracle.pyoracle import Oracle
    dt, th, nt = 1e-3, 0.016, 300
    zcom = Oracle(sim_time=1.0, dt=dt, horizon_time=th, do_ik=True).zcom
    ctl = BatchedController(1, default_config(dt=dt, time_horizon=th, z_com=zcom))
    ctl.set_refs_stance(1.0, 2)
    v = np.zeros(30); v[0:2] = push
    st = ctl.new_state(consts["q0"], v[None, :], t=0.0)
    out, status, log = ctl.rollout(st, nt, log=True)
    torch.cuda.synchronize()
    stn, log, status = st.cpu().numpy(), log.cpu().numpy(), status.cpu().numpy()
    assert status[0, 2] == 0

    def make_oracle(i):
        return Oracle(sim_time=1.0, dt=dt, horizon_time=th, do_ik=True)

    _check_against_oracle(stn, log, status, nt, make_oracle, [(consts["q0"], v)])
