#!/usr/bin/env python3
"""Throughput of lmh_plant_step: 4096 robots x 100 substeps of 1 ms per launch, timed with HIP events on one handle (reported, no
threshold: the call is not on the rollout's path and bench.py's headline line does not run it).  The robots start standing half a
millimetre into the default ground with small random velocities and are driven by the torques of one stand_step held over the launch
(zero-order hold), so the feet are in contact throughout.  Every timed launch starts from the same state; the median, minimum and
maximum of `--steps` launches after `--warmup` warm-up launches are reported, in robot-substeps per second.
Usage: python scripts/plant_step_bench.py [--instances 4096] [--substeps 100] [--steps 7] [--warmup 2] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import summary, time_launches, write_lines
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--substeps", type=int, default=100)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, n = args.instances, args.substeps
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(2.0, 2)
rng = np.random.default_rng(20261104)
q = np.tile(q0, (B, 1)); q[:, 2] -= 5.0e-4
v = np.zeros((B, 30)); v[:, 0:2] = rng.uniform(-0.05, 0.05, (B, 2)); v[:, 6:] = rng.normal(0.0, 0.01, (B, 24))
st0 = ctl.new_state(q, v, t=0.0)
out, _ = ctl.stand_step(st0.clone())
tau = torch.cat([torch.zeros((B, 6), dtype=torch.float64, device=ctl.device), out[:, 0:24]], dim=1).contiguous()


def launch(s):
    global st, flags                                                # of the last launch
    st, flags = ctl.plant_step(s, tau, n)


times = time_launches(launch, args.steps, warmup=args.warmup, before=st0.clone)
flagged = int((flags != 0).sum())
ms, lo, hi = summary(times)
rate = lambda t: B * n / t / 1e3
lines = ["lmh_plant_step: %d robots x %d substeps, fp64, one wave per robot (%s)" % (B, n, torch.cuda.get_device_name(0)),
         "%.3f ms / launch (median of %d after %d warm-up; min %.3f max %.3f)" % (ms, len(times), args.warmup, lo, hi),
         "%.3f M robot-substeps/s (median; %.3f .. %.3f over the launches, spread %.1f %%)" % (
             rate(ms), rate(hi), rate(lo), 100.0 * (hi - lo) / ms),
         "flagged robots %d of %d; finite %s" % (flagged, B, bool(torch.isfinite(st[:, 0:60]).all()))]
print("\n".join(lines))
write_lines(args.out, lines)
