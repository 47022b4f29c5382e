#!/usr/bin/env python3
"""What fusing the zero-order-hold loop buys: one lmh_rollout_zoh launch against the host loop of lmh_eval + lmh_plant_step it is defined
as, 4096 robots from a standing start, 200 control ticks, n_substeps in {1, 4, 10} (reported, no threshold; the host loop is built from
calls older than lmh_rollout_zoh, so it stands for the library without it).
Per n_substeps: both versions are warmed up, then timed alternately `--steps` times from the same state, host clock around work that ends
in a device synchronise (the host loop is launch-bound at small n_substeps: that is part of what it costs).  Medians, the min..max spread
of each, control ticks/s, plant substeps/s and the ratio are reported; the two results are compared bit for bit at the timed size.
The host loop forms tau30 = [base wrench | out.tau] with one device copy per tick into a buffer allocated once.
--stand: instead, what the loop does physically -- `--stand-ticks` control ticks of four standing robots (robot 0 at rest, the others with
small random velocities) at n_substeps = 1 and 10, base height, tilt and flags every tenth of the run.  An observation, not a check.
Usage: python scripts/zoh_rate.py [--instances 4096] [--ticks 200] [--steps 5] [--warmup 2] [--stand] [--out FILE]"""
import argparse
import time

import numpy as np
import torch

from _bench_common import lines, say, write_lines
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--substeps", type=int, nargs="+", default=[1, 4, 10])
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--stand", action="store_true")
ap.add_argument("--stand-ticks", type=int, default=2000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "zoh_rate.py measures on the GPU only"
q0, zcom = ik_start_posture(0)


def standing(B, seed, rest_first=False):
    rng = np.random.default_rng(seed)
    q = np.tile(q0, (B, 1)); q[:, 2] -= 5.0e-4                  # every sole vertex half a millimetre into the default ground
    v = np.zeros((B, 30)); v[:, 0:2] = rng.uniform(-0.05, 0.05, (B, 2)); v[:, 6:] = rng.normal(0.0, 0.01, (B, 24))
    if rest_first:
        v[0] = 0.0
    return q, v


def host_loop(ctl, st, out, status, tau30, n_ticks, n_sub):
    for _ in range(n_ticks):
        ctl.stand_step(st, out, status)
        tau30[:, 6:30].copy_(out[:, 0:24])
        ctl.plant_step(st, tau30, n_sub)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


if args.stand:
    B = 4
    for n_sub in (1, 10):
        sim = args.stand_ticks * n_sub * 1e-3 + 1.0
        ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
        ctl.set_refs_stance(sim, 2)
        q, v = standing(B, 20261105, rest_first=True)
        st = ctl.new_state(q, v, t=0.0, v_prev=v)
        status = ctl.new_status()
        chunk = max(1, args.stand_ticks // 10)
        say("standing, n_substeps = %d (control period %d ms), %d control ticks:" % (n_sub, n_sub, args.stand_ticks))
        flags = np.zeros(B, dtype=np.int64)
        for done in range(chunk, args.stand_ticks + 1, chunk):
            out, status = ctl.rollout_zoh(st, chunk, n_sub, status=status)
            torch.cuda.synchronize()
            a = st.cpu().numpy()
            flags |= status.cpu().numpy()[:, 2]
            say("  tick %5d  t %6.3f s  base z %s  max |roll|,|pitch| %.4f rad  flags %s  finite %s" % (
                done, a[0, 90], np.array2string(a[:, 2], precision=4), float(np.abs(a[:, 3:5]).max()), flags.tolist(), bool(np.isfinite(a[:, :60]).all())))
        ctl.close()
else:
    B, nt = args.instances, args.ticks
    ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
    ctl.set_refs_stance(nt * max(args.substeps) * 1e-3 + 1.0, 2)
    q, v = standing(B, 20261104)
    st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
    tau30 = torch.zeros((B, 30), dtype=torch.float64, device=ctl.device)
    say("zero-order-hold loop, %d robots x %d control ticks, fp64 (%s); %d timed repeats after %d warm-up, the two versions alternating" % (
        B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
    for n_sub in args.substeps:
        tf, th = [], []
        for it in range(args.warmup + args.steps):
            sa, sb = st0.clone(), st0.clone()
            oa, ob, xa, xb = ctl.new_out(), ctl.new_out(), ctl.new_status(), ctl.new_status()
            a = timed(lambda: ctl.rollout_zoh(sa, nt, n_sub, out=oa, status=xa))
            b = timed(lambda: host_loop(ctl, sb, ob, xb, tau30, nt, n_sub))
            if it >= args.warmup:
                tf.append(a); th.append(b)
        same = bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)) and torch.equal(oa.view(torch.int64), ob.view(torch.int64)))
        mf, mh = float(np.median(tf)), float(np.median(th))
        spread = lambda t, m: 100.0 * (max(t) - min(t)) / m
        say("n_substeps %2d: fused %8.2f ms (%.2f .. %.2f, spread %.1f %%) = %.3f M ticks/s, %.3f M substeps/s | host loop %8.2f ms (%.2f .. %.2f, "
            "spread %.1f %%) = %.3f M ticks/s, %.3f M substeps/s | host / fused %.2f | same bits %s, flagged %d, finite %s" % (
                n_sub, mf * 1e3, min(tf) * 1e3, max(tf) * 1e3, spread(tf, mf), B * nt / mf / 1e6, B * nt * n_sub / mf / 1e6,
                mh * 1e3, min(th) * 1e3, max(th) * 1e3, spread(th, mh), B * nt / mh / 1e6, B * nt * n_sub / mh / 1e6, mh / mf,
                same, int((xa[:, 2] != 0).sum()), bool(torch.isfinite(sa[:, 0:60]).all())))
write_lines(args.out, lines)
