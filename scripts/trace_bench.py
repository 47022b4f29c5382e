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
ap.add_argument("--short-ticks", type=int, default=1000)
ap.add_argument("--steps", type=int, default=3)
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


def measure(name, ticks, every):
    ns = capi.lib().lmh_trace_samples(ticks, every)
    trace = torch.zeros((ns, B, capi.TRACE_STRIDE), dtype=torch.float64, device=ctl.device) if every else None
    times, flagged = [], 0
    for it in range(args.steps + 1):                                # the first launch warms up
        st = ctl.new_state(q0, np.zeros(30), t=0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if every:
            ctl.rollout_trace(st, ticks, every, out, status, log[:ticks], trace)
        else:
            ctl.rollout(st, ticks, out, status, log[:ticks])
        e1.record()
        torch.cuda.synchronize()
        if it:
            times.append(e0.elapsed_time(e1))
        flagged = int((status[:, 2] != 0).sum().item())
    if every:                                                       # the last sample is the launch's own final record
        assert torch.equal(trace[-1, :, :96], st) and torch.equal(trace[-1, :, 96:176], out)
    ms = float(np.median(times))
    gb = ns * B * capi.TRACE_STRIDE * 8 / 1e9
    line = "%-9s %5d ticks  %5d samples  %7.3f GB written  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  flagged robots %d of %d" % (
        name, ticks, ns, gb, ms, len(times), min(times), max(times), B * ticks / ms / 1e3, flagged, B)
    print(line, flush=True)
    del trace
    torch.cuda.empty_cache()
    return line


lines = ["rollout trace: %d robots, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); a sample is %d B per robot"
         % (B, dt, N, mpc_dt, torch.cuda.get_device_name(0), capi.TRACE_STRIDE * 8)]
lines.append(measure("none", nt, 0))
lines.append(measure("every=10", nt, 10))
lines.append(measure("none", args.short_ticks, 0))
lines.append(measure("every=1", args.short_ticks, 1))
lines.append(measure("none", nt, 0))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
