"""Shared cases of the lmh_rollout_zoh_box tests (test_zoh_box.py on the CPU, test_gpu_zoh_box.py on the GPU).  Nothing here imports the HIP
library; everything is computed once per process and never written by a test.

The call is DEFINED by a host loop of calls that exist (include/lmh.h): lmh_rollout_zoh_ex's loop with the reference of every evaluation
formed by lmh_mpc_box_step at the CoM state that evaluation measures.  The GPU tests hold the kernel to that loop bit for bit; what is stated
here is the input: six robots, their plans, their boxes, and the push of the behaviour test.

Robots (B = 6, all at the IK start posture, whose CoM sits at about (-0.02, 0), with a base velocity of a few cm/s of their own):
    0  stands in double support; an all-infinite box in the per-robot sets: no bound can be active
    1  stands on its left foot for the whole run (plan ZMP y = +0.05); zmp_box of its plan with a margin of 15 mm: y in [0.04, 0.06]
    2, 3  robot 1's plan; robot 1's box moved by +2 cm in y and -3 cm in x: y in [0.06, 0.08]
    4, 5  walking plans of their own that change phase inside the preview window, zmp_boxes with a margin of 5 / 8 mm
Robots 2 and 3 are what makes a bound bind by construction: the plan's own ZMP, +0.05, lies below their box's lower edge 0.06, and the
unconstrained preview step puts the ZMP between the CoM (y = 0) and the plan's ZMP, so every single-support sample of the window is below it.
binding() confirms it with the numpy statement (trajectories.lip_box_step) at the reduced states the start posture gives, with the velocity a
fifth smaller and larger than the base's; the GPU tests assert it on the samples of every tick.
The shared set (n_sets = 1) is the moved box for every robot; robot 0 then has it too, so "no active bound on robot 0" belongs to the
per-robot sets alone."""
import functools

import numpy as np

from helpers import horizon_time, oracle_system
from linearmpchumanoid_amd import trajectories as tj

B = 6
DT = 1e-3
N_TICKS = 12
# N -> mpc_dt: the default, the largest horizon (lane 0 owns row 64, the LDS at its largest), the small strides
HORIZONS = {32: 1e-2, 64: 5e-3, 8: 1e-2}
SIM_TIME = 5.5
T_MID = 0.2                       # a clock mid-plan (a whole number of substeps: 200)
GRAVITY, ALPHA, BETA = 9.81, 1e-3, 1.0                             # lmh_config_default's
SHIFT_X, SHIFT_Y = -0.03, 0.02
XS = np.array([0.02, 0.02, 0.02, 0.02, 0.02, 0.03])
BASE_V = np.array([[0.02, -0.01], [-0.03, 0.02], [0.10, -0.08], [0.12, -0.05], [0.05, 0.02], [-0.04, -0.03]])
WALK = dict(num_steps=4, time_per_step=np.array([0.5, 1.3, 1.3, 1.3, 0.08, 0.1]), ds_time=np.array([0.1, 0.01, 0.01, 0.01, 0.03, 0.02]), step_height=0.002,
            settle_time=np.array([2.0, 0.0, 0.0, 0.0, 0.05, 0.26]), first_support=np.array([1, 2, 2, 2, 1, 2]))
MARGINS = np.array([0.0, 0.015, 0.015, 0.015, 0.005, 0.008])
EMPTY_ROBOT = 4                   # the robot whose window gets an empty sample in the empty-box test

# the behaviour test: one robot standing on a shared stance plan is pushed sideways at the start of control tick PUSH_TICK.
# PUSH_DV is the push's base velocity increment (m/s, y): behaviour_check() holds it to the oracle -- the unconstrained preview step at the pushed
# state commands a ZMP outside the stance box (zmp = CoM + D u, D = -z_com / g, from the oracle's CoM and Mpc3dLip reference).
PUSH_TICK = 2
PUSH_DV_Y = 1.0
STANCE_BOX = dict(lo_x=-0.05, hi_x=0.1, lo_y=-0.075, hi_y=0.075)


@functools.lru_cache(maxsize=None)
def start():
    """-> dict(q0 [30], zcom, com [3]: the CoM of the start posture)."""
    o = oracle_system(DT, 0.016)
    q0 = o.robot()["q"].copy()
    o.eval(q0, np.zeros(30), 0.0)
    return dict(q0=q0, zcom=o.zcom, com=o.robot()["CoM"].copy())


def velocities():
    v = np.zeros((B, 30))
    v[:, 0:2] = BASE_V
    v[:, 6:] = np.random.default_rng(20261201).normal(0.0, 0.05, (B, 24))
    return v


@functools.lru_cache(maxsize=None)
def draw(N):
    """-> dict(mpc_dt, th, plans (walk_plans, one per robot), xs, box [B,4,n] (the per-robot sets), shared [4,n], n)."""
    mpc_dt = HORIZONS[N]
    plans = tj.walk_plans(SIM_TIME, mpc_dt, WALK, B)
    box = tj.zmp_boxes(plans, XS, margin=MARGINS)
    box[0, 0::2] = -np.inf
    box[0, 1::2] = np.inf
    moved = box[1].copy()
    moved[0:2] += SHIFT_X
    moved[2:4] += SHIFT_Y
    box[2] = moved
    box[3] = moved
    for a in (box, moved):
        a.setflags(write=False)
    return dict(mpc_dt=mpc_dt, th=horizon_time(N, mpc_dt), plans=plans, xs=XS, box=box, shared=moved, n=plans["zmp_x"].shape[1])


def with_empty_sample(box, k):
    """A copy of per-robot sets with sample k of EMPTY_ROBOT's x rows empty (lo > hi)."""
    b = np.array(box)
    b[EMPTY_ROBOT, 0, k], b[EMPTY_ROBOT, 1, k] = 0.05, -0.05
    return b


def binding(N, t=0.0):
    """The numpy statement at the reduced states of the start (CoM of the start posture, the base's velocity times 0.8, 1 and 1.2):
    -> active [3, B] of the per-robot sets, active [3, B] of the shared set, flags OR-ed."""
    d, s = draw(N), start()
    res, flags = [], 0
    for sets in (d["box"], None):
        rows = []
        for f in (0.8, 1.0, 1.2):
            act = []
            for i in range(B):
                lip = np.array([s["com"][0], f * BASE_V[i, 0], s["com"][1], f * BASE_V[i, 1], t, 0, 0, 0])
                rec, pv = tj.lip_box_step(d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i], d["shared"] if sets is None else sets[i], lip, N, d["mpc_dt"],
                                          s["zcom"], ALPHA, BETA, GRAVITY, d["xs"][i])
                act.append(int(rec[15]))
                flags |= int(rec[14])
            rows.append(act)
        res.append(np.array(rows))
    return res[0], res[1], flags


def behaviour_check(N=32):
    """The oracle's unconstrained preview step at the start posture pushed by PUSH_DV_Y: -> (zmp [2], inside the stance box?)."""
    s = start()
    o = oracle_system(HORIZONS[N], horizon_time(N, HORIZONS[N]))
    v = np.zeros(30)
    v[1] = PUSH_DV_Y
    o.set_prev_velocity(v)
    o.eval(s["q0"], v, 0.0)
    com, ref = o.robot()["CoM"], o.qp()["mpcRef"]
    D = -o.zcom / GRAVITY
    zmp = np.array([com[0] + D * ref[2], com[1] + D * ref[5]])
    inside = STANCE_BOX["lo_x"] <= zmp[0] <= STANCE_BOX["hi_x"] and STANCE_BOX["lo_y"] <= zmp[1] <= STANCE_BOX["hi_y"]
    return zmp, bool(inside)
