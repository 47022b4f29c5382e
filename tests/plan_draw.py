"""The gait draw of the per-robot plan tests (CPU and GPU): one walking spec and one step length per robot.

Ranges (walking at control dt = 1e-3, mpc_dt = 1e-2, N = 32, simulation_time = 2.6, nominal model, IK posture, zero initial velocity;
sixteen CPU oracle robots drawn from them stayed finite with qp_status = 0 through 2400 ticks):
    time_per_step U(0.35, 0.65) s | ds_time U(0.2, 0.4) x time_per_step | step_height U(0.01, 0.03) m | settle_time U(0.05, 0.4) s |
    num_steps 2, 3 or 4 | first_support PHASE_RIGHT or PHASE_LEFT | xscale U(0.02, 0.05) m | foot_y 0.05 (the IK stance).
One generator, numpy.random.default_rng(seed), is consumed robot by robot in the order time_per_step, num_steps (integers(2, 5)),
ds_time factor, step_height, settle_time, first_support (integers(1, 3)), xscale: robot i of a batch of 16 is robot i of a batch of 256.
"""
import numpy as np

SEED = 20261016
SIM_TIME = 2.6
DT, MPC_DT, N_PREVIEW = 1e-3, 1e-2, 32
FOOT_Y = 0.05


def draw_walk_specs(B, seed=SEED):
    """-> (specs: dict of [B] arrays with walk_plan's keyword arguments, xscale [B])."""
    rng = np.random.default_rng(seed)
    sp = dict(time_per_step=np.zeros(B), ds_time=np.zeros(B), step_height=np.zeros(B), settle_time=np.zeros(B),
              num_steps=np.zeros(B, dtype=np.int64), first_support=np.zeros(B, dtype=np.int64), foot_y=np.full(B, FOOT_Y))
    xs = np.zeros(B)
    for i in range(B):
        sp["time_per_step"][i] = rng.uniform(0.35, 0.65)
        sp["num_steps"][i] = rng.integers(2, 5)
        sp["ds_time"][i] = rng.uniform(0.2, 0.4) * sp["time_per_step"][i]
        sp["step_height"][i] = rng.uniform(0.01, 0.03)
        sp["settle_time"][i] = rng.uniform(0.05, 0.4)
        sp["first_support"][i] = rng.integers(1, 3)
        xs[i] = rng.uniform(0.02, 0.05)
    return sp, xs


def spec_i(sp, i):
    """Robot i's keyword arguments of trajectories.walk_plan / BatchedController.gen_walk."""
    return {k: (int(v[i]) if v.dtype.kind == "i" else float(v[i])) for k, v in sp.items()}


JUMP_SEED = 20261017


def draw_jump_specs(B, seed=JUMP_SEED):
    """stance_time U(0.3, 0.5) s, flight_time U(0.08, 0.16) s, drawn robot by robot in that order."""
    rng = np.random.default_rng(seed)
    sp = dict(stance_time=np.zeros(B), flight_time=np.zeros(B))
    for i in range(B):
        sp["stance_time"][i] = rng.uniform(0.3, 0.5)
        sp["flight_time"][i] = rng.uniform(0.08, 0.16)
    return sp
