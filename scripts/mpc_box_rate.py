#!/usr/bin/env python3
"""What the box-constrained MPC calls cost.  `--instances` robots (4096) on per-robot walking plans (tests/plan_draw.py's draw: 64 plans,
repeated), mpc_dt = 10 ms, at N = 32 and N = 64:
  step      lmh_mpc_box_step in robots/s with none, a few and all samples of an axis active (the whole sole on the reference | a 1 cm push
            in a sole shrunk by 15 mm | a 3 cm, 0.2 m/s push in a +-2 mm box), beside lmh_mpc_step and lmh_mpc_preview on the same states;
            the mean and maximum rounds and the mean active samples come from lmh_mpc_box_preview's header at the same states
  rollout   lmh_mpc_box_rollout in robot-ticks/s beside lmh_mpc_rollout on the same plans, `--ticks` ticks from a 1 cm push in a sole shrunk
            by 10 mm, with the share of ticks that had an active bound
The parent of these calls has no constrained solve: the numbers are information, not a pass mark.  Everything is warmed up, then timed
`--steps` times, host clock around work that ends in a device synchronise; medians and the min..max spread are reported.
Usage: python scripts/mpc_box_rate.py [--instances 4096] [--ticks 200] [--steps 5] [--warmup 2] [--out FILE]"""
import argparse
import time

import numpy as np
import torch

from _bench_common import MPC_DT, DT, lines, say, write_lines
import plan_draw
from linearmpchumanoid_amd import trajectories as tj
from linearmpchumanoid_amd.controller import BatchedController, default_config

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "mpc_box_rate.py measures on the GPU only"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stat(fn):
    t = [timed(fn) for _ in range(args.warmup + args.steps)][args.warmup:]
    m = float(np.median(t))
    return m, "%.3f ms (%.3f .. %.3f)" % (m * 1e3, min(t) * 1e3, max(t) * 1e3)


B, nt, DISTINCT = args.instances, args.ticks, 64
reps = -(-B // DISTINCT)
sp, xs64 = plan_draw.draw_walk_specs(DISTINCT)
sim_time = nt * MPC_DT + 2.0
plans64 = tj.walk_plans(sim_time, MPC_DT, sp)
plans = {k: np.concatenate([v] * reps)[:B] for k, v in plans64.items()}
xs = np.concatenate([xs64] * reps)[:B]
zcoms = np.linspace(0.24, 0.275, B)
n = plans["zmp_x"].shape[1]
REGIMES = (("none active", 0.0, (0.0, 0.0, 0.0, 0.0)), ("a few active", 0.015, (0.01, 0.05, 0.01, 0.05)), ("all active", 0.023, (0.005, 0.0, 0.03, 0.2)))
say("box-constrained LIPM preview MPC, %d robots on per-robot walking plans (%d distinct), mpc_dt = %g ms, fp64 (%s); %d timed repeats after %d warm-up"
    % (B, DISTINCT, MPC_DT * 1e3, torch.cuda.get_device_name(0), args.steps, args.warmup))
for N in (32, 64):
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N * MPC_DT + 1e-9, z_com=0.26, mpc_dt=MPC_DT))
    ctl.set_plans(plans["zmp_x"], plans["zmp_y"], plans["phase"], plans["segs"], plans["seg_of_sample"])
    ctl.set_xscale(xs)
    ctl.set_zcom(zcoms)
    k0 = np.array([int(np.flatnonzero(plans["phase"][i] != 0)[0]) + 1 for i in range(B)])      # inside the first single support
    on_ref = np.stack([xs * plans["zmp_x"][np.arange(B), k0], np.zeros(B), plans["zmp_y"][np.arange(B), k0], np.zeros(B)], axis=1)
    for name, margin, off in REGIMES:
        lipn = np.zeros((B, 8))
        lipn[:, 0:4] = on_ref + np.array(off)
        lipn[:, 4] = (k0 + 0.5) * MPC_DT
        lip = torch.as_tensor(lipn).to(ctl.device)
        box = torch.as_tensor(tj.zmp_boxes(plans64, xs64, margin=margin)).to(ctl.device).repeat(reps, 1, 1)[:B].contiguous()
        f = ctl.split_box_preview(ctl.mpc_box_preview(lip, box), N)
        rounds = torch.stack([f["rounds_x"], f["rounds_y"]]).double()
        active = (f["active_x"] + f["active_y"]).double()
        flagged = int((f["flags"] != 0).sum())
        ms, ss = stat(lambda: ctl.mpc_box_step(lip, box))
        say("N = %2d  box step, %-12s %s = %.3f M robots/s | rounds mean %.2f max %d, active samples mean %.1f of %d, flagged %d"
            % (N, name, ss, B / ms / 1e6, float(rounds.mean()), int(rounds.max()), float(active.mean()), 2 * (N + 1), flagged))
    mp, s_pv = stat(lambda: ctl.mpc_preview(lip))
    mu, s_st = stat(lambda: ctl.mpc_step(lip))
    say("N = %2d  lmh_mpc_preview        %s = %.3f M robots/s | lmh_mpc_step %s = %.1f M robots/s" % (N, s_pv, B / mp / 1e6, s_st, B / mu / 1e6))
    lipn[:, 0:4] = on_ref + np.array((0.01, 0.05, 0.01, 0.05))
    lip0 = torch.as_tensor(lipn).to(ctl.device)
    box = torch.as_tensor(tj.zmp_boxes(plans64, xs64, margin=0.01)).to(ctl.device).repeat(reps, 1, 1)[:B].contiguous()
    traj = torch.zeros((nt, B, 16), dtype=torch.float64, device=ctl.device)
    mb, s_b = stat(lambda: ctl.mpc_box_rollout(lip0.clone(), box, nt, traj=traj))
    busy = float((traj[:, :, 15] > 0).double().mean())
    flagged = int((traj[:, :, 14] != 0).sum())
    mf, s_f = stat(lambda: ctl.mpc_rollout(lip0.clone(), nt, traj=traj))
    say("N = %2d  box rollout, %d ticks  %s = %.3f M robot-ticks/s (%.0f %% of the ticks with an active bound, %d samples flagged) | lmh_mpc_rollout %s = "
        "%.1f M robot-ticks/s" % (N, nt, s_b, B * nt / mb / 1e6, 100 * busy, flagged, s_f, B * nt / mf / 1e6))
    ctl.close()
write_lines(args.out, lines)
