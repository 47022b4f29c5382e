"""The scenarios of tests/test_gpu_qp_tiles.py, importable by the test process and by the child process that runs the NaN-filled-LDS
checker build.  Both drive the matrix-core tiles of the 15-row QP set-up (qp_setup15: V, Cm, Z | Mb bp', Y, S | d, S^-1, [W | h]), whose
epilogues form their guards, selected constants and redirected addresses once per lane:

  weights   three robots whose base-position, base-angle and joint weights are three clearly different numbers, another triple per
            robot, so that a tile that takes the wrong one of 1 / w_base_pos, 1 / w_base_ang, 1 / w_joints for a row of D^-1 cannot hide
            behind two equal values; two timed velocity pushes per robot inside 8 ticks.
  walking   four robots on a walking plan compressed so that 64 ticks at dt = 1 ms pass through double support, both single supports
            and two touch-downs (settle 5 ms, steps of 20 ms with 5 ms of double support, swing apex 1 mm, steps of 1 to 4 mm: at this
            pace a longer or higher step asks for foot accelerations no contact force can supply).
"""
import numpy as np

DT, TH = 1e-3, 0.016                                               # BASELINE config 2 constants (helpers.cfg2)

# ---------------------------------------------------------------------------------------------------------------- weights
WEIGHT_SETS = [
    dict(w_base_pos=3.0, w_base_ang=17.0, w_joints=0.6),
    dict(w_base_pos=40.0, w_base_ang=2.5, w_joints=7.0),
    dict(w_base_pos=0.8, w_base_ang=6.0, w_joints=25.0),
]
WEIGHT_NT = 8
PUSH_SEED, PUSH_AMP = 20261021, 0.1


def weight_pushes():
    """-> (ticks [3,2], dv [3,2,30]): two planar base kicks per robot at distinct ticks of [0, 7)"""
    from linearmpchumanoid_amd import trajectories
    return trajectories.draw_pushes(len(WEIGHT_SETS), 2, (0, WEIGHT_NT - 1), PUSH_AMP, PUSH_SEED)


class _StandStep:
    """Oracle.eval under the name restatement_np.rk4_tick calls"""

    def __init__(self, o):
        self.o = o

    def stand_step(self, q, dq, t):
        return self.o.eval(q, dq, t)


def weight_oracle(q0, over, ticks, dv, nt=WEIGHT_NT):
    """One robot in the CPU oracle with the weights `over`, tick by tick with dv added to the velocities in front of its tick; the last tick
    through rk4_tick over Oracle.eval, whose fourth evaluation is what lmh_rollout leaves in d_out, accelerations included.
    -> dict(log [nt,36], k [nt], qpp [30], state [60], qp_status_seen)"""
    from helpers import oracle_system
    from oracle.restatement_np import rk4_tick
    o = oracle_system(DT, TH)
    o.set_gains(**over)
    state, t = np.concatenate([q0, np.zeros(30)]), 0.0
    log, ks, bad, qpp = np.zeros((nt, 36)), np.zeros(nt, np.int64), 0, None
    for n in range(nt):
        for j in np.flatnonzero(np.asarray(ticks) == n):
            state = state.copy(); state[30:60] += dv[j]
        if n < nt - 1:
            r = o.rollout(state, t, 1, log=True)
            state, t, log[n], ks[n] = r["state"], r["t"], r["log"][0], r["k"][0]
            bad |= int(r["info"][3] != 0)
        else:
            state, e = rk4_tick(_StandStep(o), state, t, DT)
            log[n, :24], log[n, 24:], ks[n], qpp = e["tau"], e["f"], e["k"], e["qpp"].copy()
            bad |= int(e["qp_status"] != 0)
    o.close()
    return dict(log=log, k=ks, qpp=qpp, state=state, qp_status_seen=bad)


# ---------------------------------------------------------------------------------------------------------------- walking
WALK_NT, WALK_SIM = 64, 1.0
WALK_SPEC = dict(num_steps=3, time_per_step=0.02, ds_time=0.005, step_height=0.001, settle_time=0.005)
WALK_XS = np.array([0.001, 0.002, 0.003, 0.004])
WALK_SPLIT = (20, 20, 24)


def walk_plan():
    from linearmpchumanoid_amd import trajectories
    return trajectories.walk_plan(WALK_SIM, DT, **WALK_SPEC)


def walk_oracle(q0, zcom, plan, xscale, nt=WALK_NT):
    from oracle.pyoracle import Oracle
    o = Oracle(sim_time=WALK_SIM, dt=DT, horizon_time=TH, do_ik=True)
    o.set_zcom(zcom)
    o.set_refs(plan["zmp_x"], plan["zmp_y"], plan["phase"])
    o.set_segments(plan["segs"], plan["seg_of_sample"], xscale=float(xscale))
    r = o.rollout(np.concatenate([q0, np.zeros(30)]), 0.0, nt, log=True)
    o.close()
    return r


def walk_run(q0, zcom, split=(WALK_NT,)):
    """The 64 ticks of the four walkers as the launches `split`, merged as push_cases.Run merges them.
    -> dict(state, out, status, log) of host arrays"""
    from helpers import make_controller
    from push_cases import Run
    plan = walk_plan()
    ctl = make_controller(len(WALK_XS), DT, TH, zcom, warm_start=1)
    ctl.set_refs(plan["zmp_x"], plan["zmp_y"], plan["phase"])
    ctl.set_segments(plan["segs"], plan["seg_of_sample"])
    ctl.set_xscale(WALK_XS)
    run = Run(ctl, q0)
    for nt in split:
        run.launch(nt)
    ctl.close()
    return run.result()
