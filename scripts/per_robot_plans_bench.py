#!/usr/bin/env python3
"""Per-robot plans against the shared plan on one handle, one box, one visit (reported, no threshold; bench.py's headline line is the
shared plan and stays so).  Config-3 settings: 4096 robots, dt = 1 ms, N = 32 x mpc_dt = 10 ms, warm start, log on, per-robot step length
U(0.02, 0.05) m, 4000-tick launches from t = 0.  Three reference sets, in this order on the same handle:
  shared    : lmh_gen_walk with bench.py's config-3 gait (0.5 s steps, 0.2 s double support, 0.3 s settle, steps to the end of the run)
  equal     : lmh_gen_walk_batch with that gait repeated 4096 times (the cost of reading a slice of one's own, nothing else changes)
  per-robot : lmh_gen_walk_batch on the draw of the per-robot tests (time_per_step U(0.35, 0.65), ds U(0.2, 0.4) x, step height
              U(0.01, 0.03), settle U(0.05, 0.4), 2-4 steps, either first support; seed 20261016): desynchronised touch-downs; these
              gaits end after at most 3 s and the robots stand for the rest of the 4 s
Usage: python scripts/per_robot_plans_bench.py [--instances 4096] [--ticks 4000] [--steps 3] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture
from plan_draw import SEED, draw_walk_specs

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
dt, mpc_dt, N = 1e-3, 1e-2, 32
sim = nt * dt + 1.0
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=dt, time_horizon=N * mpc_dt + 1e-9, z_com=zcom, mpc_dt=mpc_dt, warm_start=1))
ctl.set_xscale(np.array([np.random.default_rng(20260003 + i).uniform(0.02, 0.05) for i in range(B)]))     # bench.py's step lengths
gait = dict(num_steps=max(2, int((sim - 0.3) / 0.5)), time_per_step=0.5, ds_time=0.2, step_height=0.02, settle_time=0.3)
out, status = ctl.new_out(), ctl.new_status()
log = torch.zeros((nt, B, 36), dtype=torch.float64, device=ctl.device)


def measure(name):
    best, flagged = [], 0
    for it in range(args.steps + 1):                                # the first launch warms up
        st = ctl.new_state(q0, np.zeros(30), t=0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctl.rollout(st, nt, out, status, log)
        e1.record()
        torch.cuda.synchronize()
        if it:
            best.append(e0.elapsed_time(e1))
        flagged = int((status[:, 2] != 0).sum().item())
    ms = float(np.median(best))
    mem = ctl.get_plan(0)
    per_robot_bytes = sum(mem[k].nbytes for k in mem)
    line = "%-10s per-robot=%d  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d  plan bytes per robot %d" % (
        name, int(ctl.plans_per_instance), ms, len(best), min(best), max(best), B * nt / ms / 1e3, flagged, B, per_robot_bytes)
    print(line, flush=True)
    return line


lines = ["per-robot plans against the shared plan: %d robots, %d-tick launches, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s)" % (
    B, nt, dt, N, mpc_dt, torch.cuda.get_device_name(0))]
ctl.gen_walk(sim, **gait)
lines.append(measure("shared"))
ctl.gen_walk_batch(sim, gait)
lines.append(measure("equal"))
sp, _ = draw_walk_specs(B, SEED)
ctl.gen_walk_batch(sim, sp)
lines.append(measure("per-robot"))
ctl.gen_walk(sim, **gait)
lines.append(measure("shared"))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
