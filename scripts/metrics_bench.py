#!/usr/bin/env python3
"""Cost of the rollout metrics (lmh_rollout_metrics) against a plain launch and against the every-tick trace it replaces, on one handle,
one box, one visit (reported, no threshold; bench.py's headline line has neither and stays so).  Config-3 settings: 4096 robots, dt = 1 ms,
N = 32 x mpc_dt = 10 ms, warm start, log on, bench.py's config-3 gait and per-robot step lengths U(0.02, 0.05) m, launches of 1000 ticks
from t = 0 (an every-tick trace of 4000 would be a 23.6 GB buffer), the median of three after one warm-up.
Lines, in this order on the same handle: plain | metrics | trace every = 1 | plain again (the drift of the visit), each with its ratio to
the first plain line.  The metrics line also checks its record against the trace's fold for the first robots.
Usage: python scripts/metrics_bench.py [--instances 4096] [--ticks 1000] [--steps 3] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import DT, MPC_DT, N_PREVIEW, config3_walkers, summary, time_launches, write_lines
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd import metrics as hm

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=1000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, nt = args.instances, args.ticks
ctl, q0, out, status, log = config3_walkers(B, nt)
record = ctl.new_metrics(0.8 * q0[2], 0.5)
trace = None
base = None
CHECK = min(B, 32)                                                  # robots whose record is held against the folded trace


def measure(name, mode):
    global trace, base
    if mode == "trace":
        trace = torch.zeros((nt, B, capi.TRACE_STRIDE), dtype=torch.float64, device=ctl.device)

    def fresh():
        if mode == "metrics":
            ctl.metrics_reset(record, 0.8 * q0[2], 0.5)
        return ctl.new_state(q0, np.zeros(30), t=0.0)

    def launch(s):
        if mode == "metrics":
            ctl.rollout_metrics(s, nt, record, out, status, log)
        elif mode == "trace":
            ctl.rollout_trace(s, nt, 1, out, status, log, trace)
        else:
            ctl.rollout(s, nt, out, status, log)

    times = time_launches(launch, args.steps, before=fresh)         # the first launch warms up
    flagged = int((status[:, 2] != 0).sum().item())
    ms, lo, hi = summary(times)
    base = ms if base is None else base
    extra = ""
    if mode == "trace":
        ref = hm.fold_trace(hm.identity(CHECK, 0.8 * q0[2], 0.5), trace[:, :CHECK].cpu().numpy())
        got = record[:CHECK].cpu().numpy()
        same = bool(((got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))).all())
        extra = "  record of the first %d robots == fold of this trace: %s" % (CHECK, same)
        trace = None
        torch.cuda.empty_cache()
    line = "%-8s %5d ticks  %9.2f ms / launch (median of %d; min %.2f max %.2f)  %8.3f M ticks/s  x%.4f of plain  flagged robots %d of %d%s" % (
        name, nt, ms, len(times), lo, hi, B * nt / ms / 1e3, ms / base, flagged, B, extra)
    print(line, flush=True)
    return line


lines = ["rollout metrics: %d robots, dt=%g, N=%d x mpc_dt=%g, log on, same handle (%s); a record is %d B per robot, a trace sample %d B per robot and tick"
         % (B, DT, N_PREVIEW, MPC_DT, torch.cuda.get_device_name(0), capi.METRICS_STRIDE * 8, capi.TRACE_STRIDE * 8)]
lines.append(measure("plain", "plain"))
lines.append(measure("metrics", "metrics"))
lines.append(measure("every=1", "trace"))
lines.append(measure("plain", "plain"))
s = hm.summarise(record.cpu().numpy(), DT)
lines.append("summary of the records: effort median %.4g, peak torque max %.4g, min base height min %.4g, RMS CoM error x | y median %.3g | %.3g, robots flagged %d, fallen %d"
             % (np.median(s["effort"]), s["peak_torque"].max(), s["min_base_height"].min(), np.median(s["rms_error"][:, 0]), np.median(s["rms_error"][:, 1]),
                int(np.isfinite(s["t_first_flag"]).sum()), int(np.isfinite(s["t_first_fall"]).sum())))
print(lines[-1])
write_lines(args.out, lines)
