#!/usr/bin/env python3
"""Host time per call of rollout_zoh_io and rollout_zoh_rigid: what the Python argument handling and the C host layer cost around a launch
that is as short as the family has one -- 64 standing robots (zoh_rate.py's start), ONE control tick of ONE substep, fp64.  Timed on the
host: time.perf_counter around { the call ; torch.cuda.synchronize() }, microseconds, medians with min..max over --steps calls after
--warmup untimed ones, each call with what exercises the argument handling (io: meas, actuators with act_mem, applied and log allocated;
rigid: a mode per tick, kv, lam allocated, meas).
Every series is one child process of this script (_bench_common.parent_pass), three per side and call, alternating:
  parent   the library built from the parent commit (--parent-variant NAME loads linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py)
           driven by the parent commit's controller.py (the file LMH_PARENT_CONTROLLER names, loaded in the place of this tree's)
  tree     this build and this tree's controller.py, in a child of the same kind
Verdict per call: the median of the tree's series medians against the parent's, PASS when it is no more than the parent's own spread (largest
minus smallest series median of this session) above the parent's median of medians.  No ratio is fixed in advance: nobody has measured the host
time per call here before.  Without a parent library only this tree is measured, and the output says so.
Usage: [LMH_PARENT_CONTROLLER=FILE] python scripts/zoh_call_overhead.py --instances 64 --ticks 1 --substeps 1 --steps 300 --warmup 30
                                        [--parent-variant NAME] [--out FILE]"""
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

from _bench_common import have_parent, lines, parent_pass, say, standing, summary, write_lines, zoh_rate_args

CALLS = ("rollout_zoh_io", "rollout_zoh_rigid")
REPEATS = 3                                                         # series per side and call
args = zoh_rate_args("rollout_zoh_io or rollout_zoh_rigid (--call) on the host clock", (), calls=CALLS)


def child():
    """One series: --steps timed calls of args.call on the library LMH_VARIANT selects; the parent's library with the parent's controller."""
    if os.environ.get("LMH_VARIANT") and os.environ.get("LMH_PARENT_CONTROLLER"):
        import linearmpchumanoid_amd
        spec = importlib.util.spec_from_file_location("linearmpchumanoid_amd.controller_of_parent", os.environ["LMH_PARENT_CONTROLLER"])
        C = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(C)
    else:
        from linearmpchumanoid_amd import controller as C
    B, nt, ns = args.instances, args.ticks, args.substeps[0]
    q0, zcom = C.ik_start_posture(0)
    q, v = standing(B, q0)
    ctl = C.BatchedController(B, C.default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
    ctl.set_refs_stance((args.steps + args.warmup) * nt * ns * 1e-3 + 1.0, 2)
    ctl.set_actuators(tau_max=100.0, alpha=0.5, delay=1)
    st = ctl.new_state(q, v, t=0.0, v_prev=v)
    out, status = ctl.new_out(), ctl.new_status()
    out0, _ = ctl.stand_step(st.clone())
    mem = ctl.new_act_mem(out0[:, 0:24].contiguous())
    meas = torch.zeros((nt, B, 60), dtype=torch.float64, device=ctl.device)
    mode = torch.zeros((nt, B), dtype=torch.int32, device=ctl.device)
    if args.call == "rollout_zoh_io":
        call = lambda: ctl.rollout_zoh_io(st, nt, ns, meas=meas, actuators=True, act_mem=mem, applied=True, log=True, out=out, status=status)
    else:
        call = lambda: ctl.rollout_zoh_rigid(st, nt, ns, mode=mode, kv=50.0, lam=True, meas=meas, out=out, status=status)
    times = []
    for it in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if it >= args.warmup:
            times.append(1e6 * (time.perf_counter() - t0))
    print(json.dumps({"times": {str(ns): times}, "controller": C.__file__}))
    sys.exit(0)


if args.child:
    child()
n_sub = str(args.substeps[0])
say("host time per call, rollout_zoh_io and rollout_zoh_rigid, %d robots x %d control tick(s) x %d substep(s), fp64 (%s); per series %d timed calls after %d warm-up, "
    "perf_counter around the call and the synchronize" % (args.instances, args.ticks, args.substeps[0], torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent(args):
    say("no parent library (--parent-variant): this tree only, nothing is compared with the parent")
elif not os.environ.get("LMH_PARENT_CONTROLLER"):
    say("LMH_PARENT_CONTROLLER is not set: the parent's LIBRARY under this tree's controller.py (the C host layer alone is compared)")
series = {(side, call): [] for side in ("parent", "tree") for call in CALLS}
for rep in range(REPEATS):
    for call in CALLS:
        args.call = call
        if have_parent(args):
            series["parent", call].append(parent_pass(args)[n_sub])
        series["tree", call].append(parent_pass(args, "")[n_sub])
for call in CALLS:
    say("%s:" % call)
    meds = {}
    for side in ("parent", "tree"):
        for i, t in enumerate(series[side, call]):
            m, lo, hi = summary(t)
            say("  %-6s series %d: %8.1f us (%.1f .. %.1f)" % (side, i + 1, m, lo, hi))
        meds[side] = [summary(t)[0] for t in series[side, call]]
    if meds["parent"]:
        p, t, spread = float(np.median(meds["parent"])), float(np.median(meds["tree"])), max(meds["parent"]) - min(meds["parent"])
        say("  parent median of medians %.1f us, its own spread %.1f us (%.2f %%); tree %.1f us = parent x %.4f | no more than the parent's spread above it: %s"
            % (p, spread, 100.0 * spread / p, t, t / p, "PASS" if t <= p + spread else "FAIL"))
write_lines(args.out, lines)
