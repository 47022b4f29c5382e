#!/usr/bin/env python3
"""Timed velocity pushes inside the rollout kernel against no schedule, on one handle, one box, one visit (reported, no threshold;
bench.py's headline line has no schedule and stays so).  Config-3 settings: 4096 robots, dt = 1 ms, N = 32 x mpc_dt = 10 ms, warm start,
log on, bench.py's config-3 gait and per-robot step lengths U(0.02, 0.05) m, 4000-tick launches from t = 0.  Three schedules, in this
order on the same handle:
  none    : no schedule (lmh_set_pushes(NULL): the tick loop compares against a tick that never comes)
  unused  : 8 records per robot, all unused (tick -1): the table is read at every chunk load, nothing is ever due
  pushed  : 8 planar base kicks per robot, trajectories.draw_pushes(B, 8, (0, ticks), amplitude, seed): every robot kicked at instants of
            its own.  Pushed walkers who fall take other cone routes (general-route solves, iteration caps), so this line is the cost of
            the experiment, not of the mechanism alone; `flagged robots` says how many left the flag-free regime
  none    : again, the drift of the visit
Usage: python scripts/push_bench.py [--instances 4096] [--ticks 4000] [--steps 3] [--amplitude 0.05] [--seed 20261019] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from linearmpchumanoid_amd import trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--amplitude", type=float, default=0.05)
ap.add_argument("--seed", type=int, default=20261019)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
dt, mpc_dt, N = 1e-3, 1e-2, 32
sim = nt * dt + 1.0
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=dt, time_horizon=N * mpc_dt + 1e-9, z_com=zcom, mpc_dt=mpc_dt, warm_start=1))
ctl.set_xscale(np.array([np.random.default_rng(20260003 + i).uniform(0.02, 0.05) for i in range(B)]))     # bench.py's step lengths
ctl.gen_walk(sim, num_steps=max(2, int((sim - 0.3) / 0.5)), time_per_step=0.5, ds_time=0.2, step_height=0.02, settle_time=0.3)
out, status = ctl.new_out(), ctl.new_status()
log = torch.zeros((nt, B, 36), dtype=torch.float64, device=ctl.device)


def measure(name):
    times, flagged = [], 0
    for it in range(args.steps + 1):                                # the first launch warms up
        st = ctl.new_state(q0, np.zeros(30), t=0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctl.rollout(st, nt, out, status, log)
        e1.record()
        torch.cuda.synchronize()
        if it:
            times.append(e0.elapsed_time(e1))
        flagged = int((status[:, 2] != 0).sum().item())
    ms = float(np.median(times))
    line = "%-8s records per robot %2d  per-robot=%d  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d" % (
        name, ctl.get_pushes(0)["ticks"].size, int(ctl.pushes_per_instance), ms, len(times), min(times), max(times), B * nt / ms / 1e3, flagged, B)
    print(line, flush=True)
    return line


lines = ["velocity pushes inside the rollout: %d robots, %d-tick launches, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); pushed: 8 kicks "
         "per robot, U(-%g, %g) m/s per axis, seed %d" % (B, nt, dt, N, mpc_dt, torch.cuda.get_device_name(0), args.amplitude, args.amplitude, args.seed)]
ctl.set_pushes(None)
lines.append(measure("none"))
ctl.set_pushes(np.full((B, 8), -1), np.zeros((B, 8, 30)))
lines.append(measure("unused"))
ctl.set_pushes(*trajectories.draw_pushes(B, 8, (0, nt), args.amplitude, args.seed))
lines.append(measure("pushed"))
ctl.set_pushes(None)
lines.append(measure("none"))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
