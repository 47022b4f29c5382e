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

import numpy as np
import torch

from _bench_common import DT, MPC_DT, N_PREVIEW, config3_gait, config3_walkers, summary, time_launches, write_lines
from plan_draw import SEED, draw_walk_specs

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
ctl, q0, out, status, log = config3_walkers(B, nt)
sim, gait = config3_gait(nt)


def measure(name):
    times = time_launches(lambda st: ctl.rollout(st, nt, out, status, log), args.steps,                 # the first launch warms up
                          before=lambda: ctl.new_state(q0, np.zeros(30), t=0.0))
    flagged = int((status[:, 2] != 0).sum().item())
    ms, lo, hi = summary(times)
    mem = ctl.get_plan(0)
    per_robot_bytes = sum(mem[k].nbytes for k in mem)
    line = "%-10s per-robot=%d  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d  plan bytes per robot %d" % (
        name, int(ctl.plans_per_instance), ms, len(times), lo, hi, B * nt / ms / 1e3, flagged, B, per_robot_bytes)
    print(line, flush=True)
    return line


lines = ["per-robot plans against the shared plan: %d robots, %d-tick launches, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s)" % (
    B, nt, DT, N_PREVIEW, MPC_DT, torch.cuda.get_device_name(0))]
ctl.gen_walk(sim, **gait)
lines.append(measure("shared"))
ctl.gen_walk_batch(sim, gait)
lines.append(measure("equal"))
sp, _ = draw_walk_specs(B, SEED)
ctl.gen_walk_batch(sim, sp)
lines.append(measure("per-robot"))
ctl.gen_walk(sim, **gait)
lines.append(measure("shared"))
write_lines(args.out, lines)
