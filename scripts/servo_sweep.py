#!/usr/bin/env python3
"""A gain sweep of the joint servo in one launch per setting (a measurement of lmh_rollout_zoh_servo, not a test): does the zero-order-hold
loop stand on flat ground once a joint-level servo runs inside the hold?  256 robots at rest on the plane z = 0 (ground_sweep.py's start),
one per cell of a 16 x 16 grid of servo records, LMH_SERVO_INTEGRATE, the metrics record on (Z_MIN, TILT_MAX as ground_sweep.py), 2000
control ticks at n_substeps = 1 and 2000 at n_substeps = 10, each ONE rollout_zoh_servo launch.
The grid is dimensionless, on every joint's own inertia at the start posture, m_j = 1 / (M^-1)_jj from terms():
    kp_j = a m_j / dt^2,   kd_j = b m_j / dt        a in {0} + 15 log-spaced values,  b in {0} + 15 log-spaced values
(dt is the plant's substep: the servo acts at every RK4 stage).  Its upper end is bounded by the stability of explicit RK4: on the real axis
|lambda dt| <= 2.78, so kd_j <= 2.78 m_j / dt, that is b <= 2.78; the grid's last b lies beyond the bound and its cells are printed as
skipped (those robots run with zero gains and are not read).  Cell (0, 0) is the control: zero gains, which must reproduce the loop without
a servo (the same launch through rollout_zoh_ex is printed beside it).
Reported per n_substeps: FIRST_FALL (control ticks; -1 = the robot stood for the whole run) of every cell, the cells that stand, and the
latest fall.
Usage: python scripts/servo_sweep.py [--ticks 2000] [--substeps 1 10] [--z-min 0.2] [--tilt-max 0.5] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import lines, say, standing, write_lines

ap = argparse.ArgumentParser()
ap.add_argument("--ticks", type=int, default=2000)
ap.add_argument("--substeps", type=int, nargs="+", default=[1, 10])
ap.add_argument("--z-min", type=float, default=0.2)
ap.add_argument("--tilt-max", type=float, default=0.5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "servo_sweep.py runs on the GPU only"
from linearmpchumanoid_amd import trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

G, DT, RK4_REAL = 16, 1e-3, 2.78
B = G * G
A = np.concatenate([[0.0], np.logspace(-4.0, 0.0, G - 1)])          # kp dt^2 / m
Bd = np.concatenate([[0.0], np.logspace(-3.0, np.log10(2.5), G - 2), [4.0]])       # kd dt / m: the last one is beyond RK4's real-axis bound
q0, zcom = ik_start_posture(0)
q, _ = standing(B, q0)
v = np.zeros((B, 30))
sim = args.ticks * max(args.substeps) * DT + 1.0


def handle():
    c = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
    c.set_refs_stance(sim, 2)
    return c


ctl = handle()
M = ctl.split_terms(ctl.terms(torch.as_tensor(q).to(ctl.device)).cpu().numpy())["M"][0]
m = 1.0 / np.diag(np.linalg.inv(M))[6:30]
ia, ib = np.divmod(np.arange(B), G)                                 # robot i: row ia (kp), column ib (kd)
skipped = Bd[ib] > RK4_REAL
kp = np.where(skipped[:, None], 0.0, A[ia][:, None] * m[None, :] / DT ** 2)
kd = np.where(skipped[:, None], 0.0, Bd[ib][:, None] * m[None, :] / DT)
ctl.set_servo(kp, kd)
say("servo gain sweep on %s: %d robots at rest on z = 0, LMH_SERVO_INTEGRATE, default controller gains, Z_MIN %.2f m, TILT_MAX %.2f rad; base height at the start %.3f m"
    % (torch.cuda.get_device_name(0), B, args.z_min, args.tilt_max, q[0, 2]))
say("joint inertias m_j = 1 / (M^-1)_jj at the start posture: %.3g .. %.3g kg m^2; kp_j = a m_j / dt^2, kd_j = b m_j / dt, dt = %g s; RK4 real-axis bound b <= %.2f" % (m.min(), m.max(), DT, RK4_REAL))
say("largest gains run: kp %.3g .. %.3g N m/rad (a = %.3g), kd %.3g .. %.3g N m s/rad (b = %.3g)"
    % (A[-1] * m.min() / DT ** 2, A[-1] * m.max() / DT ** 2, A[-1], Bd[-2] * m.min() / DT, Bd[-2] * m.max() / DT, Bd[-2]))
plain = handle()
for n_sub in args.substeps:
    st, met = ctl.new_state(q, v, t=0.0, v_prev=v), ctl.new_metrics(args.z_min, args.tilt_max)
    r = ctl.rollout_zoh_servo(st, args.ticks, n_sub, servo="integrate", metrics=met)
    st0, met0 = plain.new_state(q, v, t=0.0, v_prev=v), plain.new_metrics(args.z_min, args.tilt_max)
    plain.rollout_zoh_ex(st0, args.ticks, n_sub, metrics=met0)
    torch.cuda.synchronize()
    f, f0 = ctl.split_metrics(met.cpu().numpy()), plain.split_metrics(met0.cpu().numpy())
    ff, fl = f["first_fall"].astype(int), f["first_flag"].astype(int)
    nonfinite = ~np.isfinite(st[:, :60].cpu().numpy()).all(axis=1)
    say("")
    say("n_substeps %d: %d control ticks of %g s = %.1f s in one launch" % (n_sub, args.ticks, n_sub * DT, args.ticks * n_sub * DT))
    say("  control without a servo (rollout_zoh_ex): FIRST_FALL %d  FIRST_FLAG %d (all %d robots alike: %s) | cell (0, 0), zero gains: FIRST_FALL %d  FIRST_FLAG %d | the same: %s"
        % (f0["first_fall"][0], f0["first_flag"][0], B, bool((f0["first_fall"] == f0["first_fall"][0]).all()), ff[0], fl[0],
           "yes" if (ff[0], fl[0]) == (int(f0["first_fall"][0]), int(f0["first_flag"][0])) else "NO"))
    say("  FIRST_FALL per cell (rows a = kp dt^2 / m, columns b = kd dt / m; -1 = stood for the whole run; * = the end state is not finite):")
    say("  %9s |" % "a \\ b" + "".join(" %8.2g" % b for b in Bd))
    for i in range(G):
        say("  %9.3g |" % A[i] + "".join("  skipped" if skipped[i * G + j] else " %7d%s" % (ff[i * G + j], "*" if nonfinite[i * G + j] else " ") for j in range(G)))
    run = ~skipped
    stood = [(A[ia[i]], Bd[ib[i]]) for i in range(B) if run[i] and ff[i] < 0 and not nonfinite[i]]
    best = max((i for i in range(B) if run[i]), key=lambda i: (args.ticks if ff[i] < 0 else ff[i]))
    say("  cells that stand for the whole run: %d of %d run%s" % (len(stood), int(run.sum()), "" if not stood else ": " + ", ".join("(a %.3g, b %.3g)" % c for c in stood)))
    say("  latest fall: cell (a %.3g, b %.3g) at control tick %s; cells whose end state is not finite: %d"
        % (A[ia[best]], Bd[ib[best]], "none" if ff[best] < 0 else str(ff[best]), int((nonfinite & run).sum())))
write_lines(args.out, lines)
