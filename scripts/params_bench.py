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

import numpy as np
import torch

from _bench_common import DT, MPC_DT, N_PREVIEW, config3_walkers, summary, time_launches, write_lines

from linearmpchumanoid_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--spread", type=float, default=0.2)
ap.add_argument("--seed", type=int, default=20261020)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
ctl, q0, out, status, log = config3_walkers(B, nt)


def measure(name):
    times = time_launches(lambda st: ctl.rollout(st, nt, out, status, log), args.steps,                 # the first launch warms up
                          before=lambda: ctl.new_state(q0, np.zeros(30), t=0.0))
    flagged = int((status[:, 2] != 0).sum().item())
    ms, lo, hi = summary(times)
    line = "%-7s per-robot=%d  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d" % (
        name, int(ctl.params_per_instance()), ms, len(times), lo, hi, B * nt / ms / 1e3, flagged, B)
    print(line, flush=True)
    return line


rng = np.random.default_rng(args.seed)
drawn = {n: getattr(ctl.cfg, n) * rng.uniform(1.0 - args.spread, 1.0 + args.spread, B) for n in capi.PARAM_FIELDS}
lines = ["per-robot controller parameters in the rollout: %d robots, %d-tick launches, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); "
         "drawn: all 19 fields U(1 - %g, 1 + %g) x default per robot, seed %d" % (B, nt, DT, N_PREVIEW, MPC_DT, torch.cuda.get_device_name(0), args.spread, args.spread, args.seed)]
ctl.set_params()
lines.append(measure("shared"))
ctl.set_params(**{n: np.full(B, getattr(ctl.cfg, n)) for n in capi.PARAM_FIELDS})
lines.append(measure("same"))
ctl.set_params(**drawn)
lines.append(measure("drawn"))
ctl.set_params()
lines.append(measure("shared"))
write_lines(args.out, lines)
