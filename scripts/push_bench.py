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

import numpy as np
import torch

from _bench_common import DT, MPC_DT, N_PREVIEW, config3_walkers, summary, time_launches, write_lines

from linearmpchumanoid_amd import trajectories

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--amplitude", type=float, default=0.05)
ap.add_argument("--seed", type=int, default=20261019)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
ctl, q0, out, status, log = config3_walkers(B, nt)


def measure(name):
    times = time_launches(lambda st: ctl.rollout(st, nt, out, status, log), args.steps,                 # the first launch warms up
                          before=lambda: ctl.new_state(q0, np.zeros(30), t=0.0))
    flagged = int((status[:, 2] != 0).sum().item())
    ms, lo, hi = summary(times)
    line = "%-8s records per robot %2d  per-robot=%d  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d" % (
        name, ctl.get_pushes(0)["ticks"].size, int(ctl.pushes_per_instance), ms, len(times), lo, hi, B * nt / ms / 1e3, flagged, B)
    print(line, flush=True)
    return line


lines = ["velocity pushes inside the rollout: %d robots, %d-tick launches, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); pushed: 8 kicks "
         "per robot, U(-%g, %g) m/s per axis, seed %d" % (B, nt, DT, N_PREVIEW, MPC_DT, torch.cuda.get_device_name(0), args.amplitude, args.amplitude, args.seed)]
ctl.set_pushes(None)
lines.append(measure("none"))
ctl.set_pushes(np.full((B, 8), -1), np.zeros((B, 8, 30)))
lines.append(measure("unused"))
ctl.set_pushes(*trajectories.draw_pushes(B, 8, (0, nt), args.amplitude, args.seed))
lines.append(measure("pushed"))
ctl.set_pushes(None)
lines.append(measure("none"))
write_lines(args.out, lines)
