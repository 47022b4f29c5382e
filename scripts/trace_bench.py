#!/usr/bin/env python3
"""Cost of the rollout trace (lmh_rollout_trace) against no trace, on one handle, one box, one visit (reported, no threshold; bench.py's
headline line has no trace and stays so).  Config-3 settings: 4096 robots, dt = 1 ms, N = 32 x mpc_dt = 10 ms, warm start, log on,
bench.py's config-3 gait and per-robot step lengths U(0.02, 0.05) m, launches from t = 0, the median of three after one warm-up.
Lines, in this order on the same handle:
  none      : no trace, 4000 ticks (NULL, 0: the tick loop tests one pointer per tick and wave)
  every=10  : 4000 ticks, 400 samples per robot
  none      : no trace, 1000 ticks (the line every = 1 is read against)
  every=1   : 1000 ticks, not 4000: a sample is 1440 B per robot, so 4000 of them for 4096 robots would be a 23.6 GB buffer
  none      : 4000 ticks again, the drift of the visit
Usage: python scripts/trace_bench.py [--instances 4096] [--ticks 4000] [--short-ticks 1000] [--steps 3] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import DT, MPC_DT, N_PREVIEW, config3_walkers, summary, time_launches, write_lines
from linearmpchumanoid_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--short-ticks", type=int, default=1000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
ctl, q0, out, status, log = config3_walkers(B, nt)


def measure(name, ticks, every):
    ns = capi.lib().lmh_trace_samples(ticks, every)
    trace = torch.zeros((ns, B, capi.TRACE_STRIDE), dtype=torch.float64, device=ctl.device) if every else None
    st = None                                                       # the state of the last launch

    def fresh():
        nonlocal st
        st = ctl.new_state(q0, np.zeros(30), t=0.0)
        return st

    def launch(s):
        if every:
            ctl.rollout_trace(s, ticks, every, out, status, log[:ticks], trace)
        else:
            ctl.rollout(s, ticks, out, status, log[:ticks])

    times = time_launches(launch, args.steps, before=fresh)         # the first launch warms up
    flagged = int((status[:, 2] != 0).sum().item())
    if every:                                                       # the last sample is the launch's own final record
        assert torch.equal(trace[-1, :, :96], st) and torch.equal(trace[-1, :, 96:176], out)
    ms, lo, hi = summary(times)
    gb = ns * B * capi.TRACE_STRIDE * 8 / 1e9
    line = "%-9s %5d ticks  %5d samples  %7.3f GB written  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d" % (
        name, ticks, ns, gb, ms, len(times), lo, hi, B * ticks / ms / 1e3, flagged, B)
    print(line, flush=True)
    del trace
    torch.cuda.empty_cache()
    return line


lines = ["rollout trace: %d robots, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); a sample is %d B per robot"
         % (B, DT, N_PREVIEW, MPC_DT, torch.cuda.get_device_name(0), capi.TRACE_STRIDE * 8)]
lines.append(measure("none", nt, 0))
lines.append(measure("every=10", nt, 10))
lines.append(measure("none", args.short_ticks, 0))
lines.append(measure("every=1", args.short_ticks, 1))
lines.append(measure("none", nt, 0))
write_lines(args.out, lines)
