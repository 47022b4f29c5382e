#!/usr/bin/env python3
"""A slope sweep in one launch (a demonstration of lmh_set_ground, not a test): 64 standing robots, each on its own slope between 0 and 10
degrees -- 32 slopes that rise ahead of the robot (+x), the same 32 rising to its left (+y) --, 2 s of the zero-order-hold loop at the
default gains in ONE rollout_zoh_ex launch with the metrics record.  The plane turns about the point under the base, so every robot starts
with its soles in (or a few millimetres off) its ground; the controller is not told about the slope.  A robot is "down" when its base is
below Z_MIN or rolled / pitched beyond TILT_MAX at the end of a control tick (FIRST_FALL of the metrics record).
Reported: the same launch on a handle without a table (the control: what the loop does on the plane z = 0 by itself), then per direction
every slope with its FIRST_FALL and FIRST_FLAG (control ticks), and the steepest slope up to which no robot fell.
Usage: python scripts/ground_sweep.py [--seconds 2.0] [--substeps 1] [--z-min 0.2] [--tilt-max 0.5] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import lines, say, standing, write_lines

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0)
ap.add_argument("--substeps", type=int, default=1)
ap.add_argument("--z-min", type=float, default=0.2)
ap.add_argument("--tilt-max", type=float, default=0.5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "ground_sweep.py runs on the GPU only"
from linearmpchumanoid_amd import trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, DT = 64, 1e-3
nt = int(round(args.seconds / (DT * args.substeps)))
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(args.seconds + 1.0, 2)
q, _ = standing(B, q0)
v = np.zeros((B, 30))
slopes = np.tile(np.linspace(0.0, 10.0, B // 2), 2)
az = np.repeat([0.0, 0.5 * np.pi], B // 2)
rec = trajectories.ground_planes(np.deg2rad(slopes), az)
rec[:, 3] = rec[:, 7] = rec[:, 0] * q[:, 0] + rec[:, 1] * q[:, 1]
ctl.set_ground(rec)
st = ctl.new_state(q, v, t=0.0, v_prev=v)
m = ctl.new_metrics(args.z_min, args.tilt_max)
ctl.rollout_zoh_ex(st, nt, args.substeps, metrics=m)
torch.cuda.synchronize()
f = ctl.split_metrics(m.cpu().numpy())
say("slope sweep on %s: %d robots, %d control ticks x %d substeps of %g s (%.1f s), default gains, Z_MIN %.2f m, TILT_MAX %.2f rad; base height at the start %.3f m"
    % (torch.cuda.get_device_name(0), B, nt, args.substeps, DT, nt * args.substeps * DT, args.z_min, args.tilt_max, q[0, 2]))
plain = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
plain.set_refs_stance(args.seconds + 1.0, 2)
st0, m0 = plain.new_state(q, v, t=0.0, v_prev=v), plain.new_metrics(args.z_min, args.tilt_max)
plain.rollout_zoh_ex(st0, nt, args.substeps, metrics=m0)
torch.cuda.synchronize()
f0 = plain.split_metrics(m0.cpu().numpy())
say("control, no table (z = 0): FIRST_FALL %d  FIRST_FLAG %d  base height min %.3f m (all %d robots alike: %s)"
    % (f0["first_fall"][0], f0["first_flag"][0], f0["xmin"][0, 2], B, bool((f0["first_fall"] == f0["first_fall"][0]).all())))
for name, rows in (("rising ahead (+x)", range(0, B // 2)), ("rising to the left (+y)", range(B // 2, B))):
    say(name + ":")
    best = None
    fell = False
    for i in rows:
        ff, fl = int(f["first_fall"][i]), int(f["first_flag"][i])
        say("  %5.2f deg: FIRST_FALL %5d  FIRST_FLAG %5d  base height min %.3g m  |roll|, |pitch| max %.3g, %.3g rad"
            % (slopes[i], ff, fl, f["xmin"][i, 2], max(-f["xmin"][i, 3], f["xmax"][i, 3]), max(-f["xmin"][i, 4], f["xmax"][i, 4])))
        fell = fell or ff >= 0
        if not fell:
            best = slopes[i]
    say("  steepest slope with no FIRST_FALL on it or on any milder one: %s" % ("none" if best is None else "%.2f deg" % best))
write_lines(args.out, lines)
