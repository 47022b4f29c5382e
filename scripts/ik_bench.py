#!/usr/bin/env python3
"""Cost of the inverse-kinematics launches at 4096 robots from initial_configuration() (reported, no threshold: set-up code, not on the
rollout's path).  Host clock around `--reps` launches that end in a device synchronise; `--steps` such groups after `--warmup` untimed
ones; median, min and max per launch.  Every launch starts from its own copy of the start postures, made before the clock starts.

  ik          lmh_ik, default target (4 Newton steps per robot)
  batch1      lmh_ik_batch, n_targets = 1, the same target as device records
  batch8      lmh_ik_batch, n_targets = 8: a squat, CoM height 0.25 / 0.26 alternating from the default posture's
  chain8      the same eight targets as eight chained n_targets = 1 launches

--ik-only times lmh_ik alone and loads a library that has no lmh_ik_batch (a build of an earlier tree, LMH_VARIANT=<name>): the number to
set this tree's lmh_ik against, from alternating runs of the two.
Usage: python scripts/ik_bench.py [--instances 4096] [--reps 10] [--steps 15] [--warmup 3] [--ik-only] [--out FILE]"""
import argparse
import json
import time

import numpy as np
import torch

from _bench_common import summary, write_lines
from linearmpchumanoid_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--ik-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.ik_only:
    capi.PROTOTYPES.pop("lmh_ik_batch", None)

from linearmpchumanoid_amd.controller import BatchedController, default_config, initial_configuration  # noqa: E402

B = args.instances
ctl = BatchedController(B, default_config())
start = torch.as_tensor(np.tile(initial_configuration(), (B, 1))).to(ctl.device)


def timed(launch):
    """ms per launch: [steps] groups of `reps` launches, each on a fresh copy of the start postures."""
    times = []
    for it in range(args.warmup + args.steps):
        qs = [start.clone() for _ in range(args.reps)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for q in qs:
            launch(q)
        torch.cuda.synchronize()
        if it >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3 / args.reps)
    return times


cases = [("ik", lambda q: ctl.ik(q))]
if not args.ik_only:
    from linearmpchumanoid_amd.trajectories import ik_targets, start_targets
    one = torch.as_tensor(ik_targets(B=B)[0]).to(ctl.device)
    squat = torch.as_tensor(np.stack([start_targets(z_com=0.25 if k % 2 == 0 else 0.26, B=B) for k in range(8)])).to(ctl.device)

    def chain8(q):
        for k in range(8):
            q = ctl.ik_batch(q, squat[k])[0]

    cases += [("batch1", lambda q: ctl.ik_batch(q, one)), ("batch8", lambda q: ctl.ik_batch(q, squat)), ("chain8", chain8)]
    # what is timed is what the contract says: the same bits
    q_ik, it_ik = ctl.ik(start.clone())
    q_b1, it_b1, _ = ctl.ik_batch(start, one)
    q_b8, it_b8, _ = ctl.ik_batch(start, squat)
    q_c = start
    for k in range(8):
        q_c, it_c, _ = ctl.ik_batch(q_c, squat[k])
        assert torch.equal(q_c, q_b8[k]) and torch.equal(it_c, it_b8[k]), k
    assert torch.equal(q_ik, q_b1) and torch.equal(it_ik, it_b1)
    steps8 = [int(x) for x in it_b8[:, 0].cpu()]
result = dict(library=capi.SO_PATH.split("/")[-1], instances=B, reps=args.reps, steps=args.steps, device=torch.cuda.get_device_name(0))
lines = ["inverse kinematics: %d robots from initial_configuration(), %s (%s)" % (B, result["library"], result["device"])]
for name, fn in cases:
    ms, lo, hi = summary(timed(fn))
    result[name] = dict(median_ms=ms, min_ms=lo, max_ms=hi)
    lines.append("%-7s %8.3f ms / launch (median of %d groups of %d; min %.3f max %.3f)" % (name, ms, args.steps, args.reps, lo, hi))
    print(lines[-1], flush=True)
if not args.ik_only:
    result["newton_steps_batch8"] = steps8
    lines.append("batch1 / ik %.3f; batch8 / chain8 %.3f; Newton steps of the eight targets %s" % (
        result["batch1"]["median_ms"] / result["ik"]["median_ms"], result["batch8"]["median_ms"] / result["chain8"]["median_ms"], steps8))
    print(lines[-1])
print(json.dumps(result))
write_lines(args.out, lines + [json.dumps(result)])
ctl.close()
