#!/usr/bin/env python3
"""Throughput of the three rigid-body calls (lmh_terms, lmh_inverse_dynamics, lmh_forward_dynamics) at 4096 robots, timed with HIP events
on one handle (reported, no threshold: none of them is on the rollout's path, and bench.py's headline line does not run them).  States:
the posture sweep's draw around the IK start posture (joints +-1 rad) with velocities; qdd ~ N(0, 10^2), w ~ N(0, (m g / 2)^2).  Each call
is launched `--reps` times back to back between two events, the median of `--steps` such groups after one warm-up group is reported.
Usage: python scripts/terms_bench.py [--instances 4096] [--reps 20] [--steps 5] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import summary, time_launches, write_lines
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B = args.instances
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
rng = np.random.default_rng(20261103)
qn = np.tile(q0, (B, 1))
qn[:, 3:] += rng.uniform(-1.0, 1.0, (B, 27))
dev = lambda a: torch.as_tensor(a).to(ctl.device)
q, v = dev(qn), dev(rng.normal(0.0, 0.2, (B, 30)))
qdd, w = dev(rng.normal(0.0, 10.0, (B, 30))), dev(rng.normal(0.0, 5.305 * 9.81 / 2, (B, 12)))
tau = ctl.inverse_dynamics(q, v, qdd, w)
calls = [("terms", lambda: ctl.terms(q, v), capi.TERMS_STRIDE * 8),
         ("inverse_dynamics", lambda: ctl.inverse_dynamics(q, v, qdd, w), 240),
         ("forward_dynamics", lambda: ctl.forward_dynamics(q, v, tau, w), 244)]
lines = ["rigid-body calls: %d robots, fp64, one wave per robot (%s)" % (B, torch.cuda.get_device_name(0))]
for name, fn, nbytes in calls:
    times = time_launches(fn, args.steps, reps=args.reps)           # the first group warms up
    ms, lo, hi = summary(times)
    line = "%-17s %8.3f ms / call (median of %d groups of %d; min %.3f max %.3f)  %8.3f M robots/s  %6.2f GB/s written" % (
        name, ms, len(times), args.reps, lo, hi, B / ms / 1e3, B * nbytes / ms / 1e6)
    print(line, flush=True)
    lines.append(line)
x, flags = ctl.forward_dynamics(q, v, tau, w)
torch.cuda.synchronize()
lines.append("forward_dynamics(inverse_dynamics(qdd)) - qdd: max %.3e; flagged robots %d of %d" % (float((x - qdd).abs().max()), int((flags != 0).sum()), B))
print(lines[-1])
write_lines(args.out, lines)
