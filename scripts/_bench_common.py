"""What the timing scripts of this directory share (a private module, not a tool): the import path, bench.py's config-3 walkers, the
HIP-event timer with its median / min / max, and the --out writer.  Importing it puts the repository root and tests/ on sys.path."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

DT, MPC_DT, N_PREVIEW = 1e-3, 1e-2, 32                              # config 3: dt = 1 ms, N = 32 x mpc_dt = 10 ms


def config3_gait(n_ticks):
    """-> (simulation time, gen_walk keywords) of bench.py's config-3 gait for launches of n_ticks."""
    sim = n_ticks * DT + 1.0
    return sim, dict(num_steps=max(2, int((sim - 0.3) / 0.5)), time_per_step=0.5, ds_time=0.2, step_height=0.02, settle_time=0.3)


def config3_walkers(B, n_ticks):
    """bench.py's config-3 workload on one handle: B warm-started walkers from the IK start posture on the config-3 gait.
    -> (ctl, q0, out, status, log [n_ticks,B,36])."""
    from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture
    q0, zcom = ik_start_posture(0)
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT, warm_start=1))
    ctl.set_xscale(np.array([np.random.default_rng(20260003 + i).uniform(0.02, 0.05) for i in range(B)]))     # bench.py's step lengths
    sim, gait = config3_gait(n_ticks)
    ctl.gen_walk(sim, **gait)
    log = torch.zeros((n_ticks, B, 36), dtype=torch.float64, device=ctl.device)
    return ctl, q0, ctl.new_out(), ctl.new_status(), log


def time_launches(launch, steps, warmup=1, reps=1, before=None):
    """Milliseconds per launch of `steps` timed groups after `warmup` untimed ones, from a HIP-event pair around `reps` launches back to
    back.  before() runs outside the pair, and what it returns (a fresh state) is handed to every launch of the group."""
    times = []
    for it in range(warmup + steps):
        fresh = (before(),) if before else ()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch(*fresh)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1) / reps)
    return times


def summary(times):
    """-> (median, min, max)"""
    return float(np.median(times)), min(times), max(times)


def write_lines(path, lines):
    """The --out file; no path, no file."""
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").write("\n".join(lines) + "\n")
