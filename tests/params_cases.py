"""Shared pieces of the per-robot parameter tests (tests/test_gpu_params.py and its child process tests/params_reuse_child.py): the
parameter sets, the handles and the one comparison rule -- robot i of a handle with per-robot parameters equals robot i of a handle created
with parameter set i in its config and given the same states, with np.array_equal."""
import numpy as np

from helpers import make_controller, perturbed_velocities  # noqa: F401

# six sets: the defaults, the 18-row QP set-up (w_com_ang > 0), another friction coefficient, the full override of
# test_gpu_round2.test_non_default_gains_and_weights, and two more on the 15-row set-up (w_com_ang = 0)
SIX_SETS = [
    dict(),
    dict(w_com_ang=50.0),
    dict(mu=0.4),
    dict(w_com_ang=20.0, mu=0.5, kp_joints=250.0, kd_joints=30.0, kp_mom=12.0, kd_mom=7.0, kp_feet=450.0, kd_feet=40.0,
         w_com_lin=3000.0, w_base_pos=8.0, w_base_ang=12.0, w_joints=2.0, w_force=1.5, w_foot=50000.0, eps_coeff=2e-8),
    dict(kp_joints=350.0, kd_joints=36.0, w_joints=1.5, w_base_pos=12.0),
    dict(mu=0.55, w_force=2.0, eps_coeff=5e-9, kp_feet=550.0, kd_feet=46.0),
]
# workgroup reuse: the defaults next to a robot that differs in the friction table AND in the QP set-up size
REUSE_SETS = [dict(), dict(mu=0.4, w_com_ang=50.0)]
# four grounds of the compliant-contact plant (the first two are those of test_gpu_round2.test_plant_rollout_parity_and_physics)
PLANT_SETS = [
    dict(contact_k=2.0e4, contact_d=3.0, contact_dt=3.0, contact_mu=0.7),
    dict(contact_k=8.0e3, contact_d=2.0, contact_dt=4.0, contact_mu=0.5),
    dict(contact_k=1.5e4, contact_d=2.5, contact_dt=3.5, contact_mu=0.6),
    dict(contact_k=1.2e4, contact_d=3.0, contact_dt=2.0, contact_mu=0.8),
]


def columns(sets, cfg):
    """set_params keyword arguments from one dict per robot: a length-B array per field that any robot overrides, the config's value
    where a robot does not name it."""
    names = sorted({k for s in sets for k in s})
    return {n: np.array([s.get(n, getattr(cfg, n)) for s in sets], dtype=np.float64) for n in names}


def states(B, seed):
    """velocities and previous velocities of the B robots (the draw of test_non_default_gains_and_weights)"""
    return perturbed_velocities(B, seed=seed) * 1.5, perturbed_velocities(B, seed=seed + 1)


def run(ctl, q0, v, vprev, phases=(0, 1), ticks=30, log=True):
    """What the bit-equality tests compare, as host arrays: one stand_step (plain and debug schedule) per support phase on a fresh state,
    then a rollout of `ticks` on stance references.  ctl must have as many robots as v has rows."""
    import torch
    res = {}
    n = 2500
    for ph in phases:
        ctl.set_refs(np.zeros(n), np.zeros(n), np.full(n, ph, dtype=np.uint8))
        st = ctl.new_state(q0, v, t=0.0, v_prev=vprev)
        out, status = ctl.stand_step(st)
        st2 = ctl.new_state(q0, v, t=0.0, v_prev=vprev)
        out2, status2, _ = ctl.stand_step(st2, debug=True)
        torch.cuda.synchronize()
        res["eval%d" % ph] = dict(out=out.cpu().numpy()[:, :78], state=st.cpu().numpy(), status=status.cpu().numpy(),
                                  out_dbg=out2.cpu().numpy()[:, :78], state_dbg=st2.cpu().numpy(), status_dbg=status2.cpu().numpy())
    if ticks:
        ctl.set_refs_stance(2.0, 2)
        st = ctl.new_state(q0, v, t=0.0)
        out, status, lg = ctl.rollout(st, ticks, log=log)
        torch.cuda.synchronize()
        res["rollout"] = dict(out=out.cpu().numpy()[:, :78], state=st.cpu().numpy(), status=status.cpu().numpy())
        if log:
            res["rollout"]["log"] = lg.cpu().numpy()
    return res


def assert_robot_equal(per_robot, shared, i, what=""):
    """robot i of the two result sets of run(), bit for bit"""
    assert per_robot.keys() == shared.keys()
    for part, a in per_robot.items():
        for name, arr in a.items():
            x, y = (arr[:, i], shared[part][name][:, i]) if name == "log" else (arr[i], shared[part][name][i])
            assert np.array_equal(x, y), (what, i, part, name, float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))))
