#!/usr/bin/env python3
"""What the public MPC calls cost: lmh_mpc_rollout against the two other routes to the same CoM trajectory, and lmh_mpc_preview.
4096 robots on per-robot walking plans (tests/plan_draw.py's draw), N = 32, mpc_dt = 10 ms, 4000 ticks:
  rollout      one lmh_mpc_rollout launch, with the trajectory [ticks, B, 16] and without it
  host loop    the `--ticks` lmh_mpc_step launches the rollout is defined as, the state moved on by torch between them (reported, no threshold;
               launch-bound: that is part of what it costs)
  whole body   the only route a library without these calls has: one controller evaluation (stand_step) per tick.  The evaluation is timed
               here on the same handle, `--eval-launches` launches per repeat, and the route's cost is ticks x that time (running all 4000
               would integrate nothing anyway: the evaluation does not move the state)
  preview      one lmh_mpc_preview launch at N = 16 and N = 64
Everything is warmed up, then timed `--steps` times with the routes alternating, host clock around work that ends in a device
synchronise.  Medians and the min..max spread of each are reported; the rollout and the host loop are compared bit for bit.
Usage: python scripts/mpc_rate.py [--instances 4096] [--ticks 4000] [--steps 5] [--warmup 2] [--eval-launches 20] [--out FILE]"""
import argparse
import time

import numpy as np
import torch

from _bench_common import MPC_DT, N_PREVIEW, DT, lines, say, write_lines
import plan_draw
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=4000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--eval-launches", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "mpc_rate.py measures on the GPU only"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stat(t):
    m = float(np.median(t))
    return m, "%.3f ms (%.3f .. %.3f, spread %.1f %%)" % (m * 1e3, min(t) * 1e3, max(t) * 1e3, 100.0 * (max(t) - min(t)) / m)


def host_loop(ctl, lip, n_ticks, traj):
    for j in range(n_ticks):
        rec = ctl.mpc_step(lip)
        if traj is not None:
            traj[j].copy_(rec)
        lip[:, 0:2].copy_(rec[:, 0:2]); lip[:, 2:4].copy_(rec[:, 3:5])
        lip[:, 4] += MPC_DT


B, nt = args.instances, args.ticks
q0, zcom = ik_start_posture(0)
sp, xs = plan_draw.draw_walk_specs(B)
ctl = BatchedController(B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT))
ctl.gen_walk_batch(nt * MPC_DT + 1.0, sp)
ctl.set_xscale(xs)
ctl.set_zcom(np.linspace(0.24, 0.275, B))
lip0 = ctl.new_lip((-0.02, 0.0), (0.0, 0.0), t=0.0)
st = ctl.new_state(q0, np.zeros(30), t=0.0)
out, status = ctl.new_out(), ctl.new_status()
traj = torch.zeros((nt, B, 16), dtype=torch.float64, device=ctl.device)
traj_h = torch.zeros_like(traj)
say("LIPM preview MPC, %d robots on per-robot walking plans, N = %d, mpc_dt = %g ms, %d ticks, fp64 (%s); %d timed repeats after %d warm-up, "
    "the routes alternating" % (B, ctl.N, MPC_DT * 1e3, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
t_roll, t_quiet, t_host, t_eval = [], [], [], []
for it in range(args.warmup + args.steps):
    a, b, c = lip0.clone(), lip0.clone(), lip0.clone()
    r = (timed(lambda: ctl.mpc_rollout(a, nt, traj=traj)), timed(lambda: ctl.mpc_rollout(b, nt, traj=False)),
         timed(lambda: host_loop(ctl, c, nt, traj_h)),
         timed(lambda: [ctl.stand_step(st, out, status) for _ in range(args.eval_launches)]) / args.eval_launches)
    if it >= args.warmup:
        for lst, v in zip((t_roll, t_quiet, t_host, t_eval), r):
            lst.append(v)
same = bool(torch.equal(a.view(torch.int64), c.view(torch.int64)) and torch.equal(traj.view(torch.int64), traj_h.view(torch.int64))
            and torch.equal(a.view(torch.int64), b.view(torch.int64)))
flags = traj[:, :, 14].to(torch.int64)
(mr, sr), (mq, sq), (mh, sh), (me, se) = stat(t_roll), stat(t_quiet), stat(t_host), stat(t_eval)
say("rollout, trajectory stored  %s = %.1f M robot-ticks/s" % (sr, B * nt / mr / 1e6))
say("rollout, no trajectory      %s = %.1f M robot-ticks/s" % (sq, B * nt / mq / 1e6))
say("host loop of mpc_step       %s = %.2f M robot-ticks/s | host loop / rollout %.1f | same bits %s" % (sh, B * nt / mh / 1e6, mh / mr, same))
say("one controller evaluation   %s = %.3f M evaluations/s; %d ticks of it: %.1f ms = %.0f x the rollout with its trajectory "
    "(slowest rollout %.3f ms against %d x the fastest evaluation %.1f ms)" % (
        se, B / me / 1e6, nt, nt * me * 1e3, nt * me / mr, max(t_roll) * 1e3, nt, nt * min(t_eval) * 1e3))
say("samples flagged (the plans cover every window): %d; finite: %s; CoM x after %d ticks %.4f .. %.4f m" % (
    int((flags != 0).sum()), bool(torch.isfinite(traj[:, :, 0:8]).all()), nt, float(a[:, 0].min()), float(a[:, 0].max())))
ctl.close()
for N in (16, 64):
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT))
    ctl.gen_walk_batch(6.0, sp)
    ctl.set_xscale(xs)
    ctl.set_zcom(np.linspace(0.24, 0.275, B))
    lip = ctl.new_lip((-0.02, 0.0), (0.05, 0.02), t=np.linspace(0.0, 2.0, B))
    tp = [timed(lambda: ctl.mpc_preview(lip)) for _ in range(args.warmup + args.steps)][args.warmup:]
    pv = ctl.mpc_preview(lip)
    mp, s = stat(tp)
    say("preview N = %2d              %s = %.3f M robots/s | flagged not SPD %d, finite %s" % (
        N, s, B / mp / 1e6, int((pv[:, 1].to(torch.int64) & 8 != 0).sum()), bool(torch.isfinite(pv).all())))
    ctl.close()
write_lines(args.out, lines)
