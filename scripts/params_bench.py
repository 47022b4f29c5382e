#!/usr/bin/env python3
"""Per-robot controller parameters (lmh_set_params) against the config's one set, on one handle, one box, one visit (reported, no
threshold; bench.py's headline line runs the shared set and stays so).  Config-3 settings: 4096 robots, dt = 1 ms, N = 32 x mpc_dt = 10 ms,
warm start, log on, bench.py's config-3 gait and per-robot step lengths U(0.02, 0.05) m, 4000-tick launches from t = 0, HIP events.
Three settings, in this order on the same handle:
  shared  : no per-robot parameters (lmh_set_params(NULL)): the rollout instantiation every earlier round ran
  same    : one record per robot, every record the config's values: the cost of the mechanism alone (the other instantiation, one block
            and one friction table per robot behind the scalar cache)
  drawn   : every one of the 19 fields drawn per robot within +/- `spread` of its default (w_com_ang's default is 0 and stays 0).
            Other gains and weights take other active-set routes, so this line is the cost of the experiment, not of the mechanism
  shared  : again, the drift of the visit
Usage: python scripts/params_bench.py [--instances 4096] [--ticks 4000] [--steps 3] [--spread 0.2] [--seed 20261020] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--spread", type=float, default=0.2)
ap.add_argument("--seed", type=int, default=20261020)
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
    line = "%-7s per-robot=%d  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d" % (
        name, int(ctl.params_per_instance()), ms, len(times), min(times), max(times), B * nt / ms / 1e3, flagged, B)
    print(line, flush=True)
    return line


rng = np.random.default_rng(args.seed)
drawn = {n: getattr(ctl.cfg, n) * rng.uniform(1.0 - args.spread, 1.0 + args.spread, B) for n in capi.PARAM_FIELDS}
lines = ["per-robot controller parameters in the rollout: %d robots, %d-tick launches, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); "
         "drawn: all 19 fields U(1 - %g, 1 + %g) x default per robot, seed %d" % (B, nt, dt, N, mpc_dt, torch.cuda.get_device_name(0), args.spread, args.spread, args.seed)]
ctl.set_params()
lines.append(measure("shared"))
ctl.set_params(**{n: np.full(B, getattr(ctl.cfg, n)) for n in capi.PARAM_FIELDS})
lines.append(measure("same"))
ctl.set_params(**drawn)
lines.append(measure("drawn"))
ctl.set_params()
lines.append(measure("shared"))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
