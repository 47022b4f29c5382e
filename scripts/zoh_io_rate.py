#!/usr/bin/env python3
"""What the options of lmh_rollout_zoh_io cost in the zero-order-hold loop: 4096 standing robots (zoh_rate.py's start), 200 control ticks,
n_substeps 1 and 10, fp64.
Timed per n_substeps, HIP events around one launch, medians with min..max, the rows of this build interleaved launch by launch:
  ex, nothing set        lmh_rollout_zoh_ex without an option on this build (judged: inside the parent's spread, its code object is unchanged)
  io, nothing set        lmh_rollout_zoh_io without an option: the same kernel (judged the same way)
  io, meas               a measurement error per control tick and robot
  io, actuators          per-robot records: delay i % 4 control ticks, alpha 0.8, a limit of 15 N m on every joint (mild: the robots keep
                         standing, so the rows time the same controller work)
  io, applied            the applied torques stored
  io, all three          the measurement, the actuator and the applied torques together
  ex, everything         pushes, a wrench sequence, metrics and the every-tick trace of lmh_rollout_zoh_ex (zoh_ex_rate.py's row), and
  io, all + everything   the same with all three options of lmh_rollout_zoh_io on top: reported relative to the row above it
  parent                 rollout_zoh_ex, nothing set, from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), in two child processes of this one, one before and one
                         after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
The option rows are reported relative to "ex, nothing set", not judged.  Without a parent library only this build is measured, and the output says so.
Usage: python scripts/zoh_io_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                     [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

from _bench_common import ROOT, summary, time_launches, write_lines

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--substeps", type=int, nargs="+", default=[1, 10])
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--parent-variant", default=None)
ap.add_argument("--child", action="store_true", help="(internal) time rollout_zoh_ex on the library LMH_VARIANT selects and print one JSON line")
ap.add_argument("--out", default=None)
args = ap.parse_args()

from linearmpchumanoid_amd import capi

if args.child:                                                     # a library of the parent tree has not got the new entry points
    for name in ("lmh_rollout_zoh_io", "lmh_set_actuators", "lmh_actuators_per_instance", "lmh_get_actuators"):
        capi.PROTOTYPES.pop(name, None)
from linearmpchumanoid_amd import trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

assert torch.cuda.is_available(), "zoh_io_rate.py measures on the GPU only"
B, nt = args.instances, args.ticks
q0, zcom = ik_start_posture(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def standing(seed=20261104):                                       # zoh_rate.py's start
    rng = np.random.default_rng(seed)
    q = np.tile(q0, (B, 1)); q[:, 2] -= 5.0e-4
    v = np.zeros((B, 30)); v[:, 0:2] = rng.uniform(-0.05, 0.05, (B, 2)); v[:, 6:] = rng.normal(0.0, 0.01, (B, 24))
    return q, v


ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * 1e-3 + 1.0, 2)
q, v = standing()
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()

if args.child:
    print(json.dumps({"times": {str(n): time_launches(lambda st: ctl.rollout_zoh_ex(st, nt, n, out=out, status=status), args.steps, args.warmup, before=st0.clone)
                                for n in args.substeps}}))
    sys.exit(0)


def parent_pass():
    env = {k: val for k, val in os.environ.items() if k != "LMH_DIAG"}
    env["LMH_VARIANT"] = args.parent_variant
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--instances", str(B), "--ticks", str(nt), "--steps", str(args.steps),
                        "--warmup", str(args.warmup), "--substeps", *map(str, args.substeps)], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["times"]


have_parent = bool(args.parent_variant) and os.path.exists(os.path.join(ROOT, "linearmpchumanoid_amd", "liblmh_hip_var_%s.so" % args.parent_variant))
say("zero-order-hold loop and the options of lmh_rollout_zoh_io, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
    % (B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent:
    say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
parent = [parent_pass()] if have_parent else []
dev = ctl.device
rng = np.random.default_rng(20261220)
meas = torch.zeros((nt, B, 60), dtype=torch.float64, device=dev)
meas[:, :, 0:30] = torch.as_tensor(rng.normal(0.0, 1.0e-4, (nt, B, 30))).to(dev)
meas[:, :, 30:60] = torch.as_tensor(rng.normal(0.0, 1.0e-3, (nt, B, 30))).to(dev)
applied = torch.zeros((nt, B, 24), dtype=torch.float64, device=dev)
ctl.set_actuators(tau_max=15.0, alpha=0.8, delay=np.arange(B) % 4)
mem0 = ctl.new_act_mem()
bw = torch.as_tensor(np.random.default_rng(20261105).normal(0.0, 0.5, (nt, B, 6))).to(dev)
metrics = ctl.new_metrics(0.2, 0.5)
mine = {}
for n_sub in args.substeps:
    ticks, dv = trajectories.draw_pushes(B, 16, (1, nt * n_sub), 0.02, 20261106)         # 16 records per robot, all inside the run
    ctl.set_pushes(ticks, dv)
    tr1 = torch.zeros((nt, B, capi.TRACE_STRIDE), dtype=torch.float64, device=dev)
    mem = mem0.clone()                                             # (handed on from launch to launch: what it holds does not change the work)
    io = lambda **kw: (lambda s: ctl.rollout_zoh_io(s, nt, n_sub, out=out, status=status, **kw))
    every = dict(pushes=True, base_wrench=bw, metrics=metrics, trace_every=1, trace=tr1)
    three = dict(meas=meas, actuators=True, act_mem=mem, applied=applied)
    rows = [("ex, nothing set", lambda s: ctl.rollout_zoh_ex(s, nt, n_sub, out=out, status=status)),
            ("io, nothing set", io()),
            ("io, meas", io(meas=meas)),
            ("io, actuators", io(actuators=True, act_mem=mem)),
            ("io, applied", io(applied=applied)),
            ("io, all three", io(**three)),
            ("ex, everything", lambda s: ctl.rollout_zoh_ex(s, nt, n_sub, out=out, status=status, **every)),
            ("io, all + everything", io(**three, **every))]
    # what the launches leave: rollout_zoh_ex's bytes without an option; how many robots a limit cut and how many carry a counted flag with all three on
    sa, sb, sc = st0.clone(), st0.clone(), st0.clone()
    ra = ctl.rollout_zoh_ex(sa, nt, n_sub)
    rb = ctl.rollout_zoh_io(sb, nt, n_sub)
    rc = ctl.rollout_zoh_io(sc, nt, n_sub, meas=meas, actuators=True, act_mem=mem0.clone(), applied=applied)
    torch.cuda.synchronize()
    same = bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)) and torch.equal(ra["out"].view(torch.int64), rb["out"].view(torch.int64))
                and torch.equal(ra["status"], rb["status"]))
    times = {name: [] for name, _ in rows}
    for it in range(args.steps):                                   # interleaved, one timed launch each (the first round also warms up)
        for name, fn in rows:
            times[name] += time_launches(fn, 1, args.warmup if it == 0 else 0, before=st0.clone)
    mine[n_sub] = (times, same, int(((rc["status"][:, 2] & capi.FLAG_TAU_LIMIT) != 0).sum()), int(((rc["status"][:, 2] & 15) != 0).sum()), [name for name, _ in rows])
    ctl.set_pushes(None)
if have_parent:
    parent.append(parent_pass())
fmt = lambda t: "%8.2f ms (%.2f .. %.2f, spread %.1f %%) = %.3f M ticks/s" % (summary(t)[0], summary(t)[1], summary(t)[2],
                                                                             100.0 * (max(t) - min(t)) / summary(t)[0], B * nt / summary(t)[0] / 1e3)
for n_sub in args.substeps:
    times, same, cut, flagged, names = mine[n_sub]
    base = summary(times["ex, nothing set"])[0]
    say("n_substeps %2d: (io with nothing set leaves rollout_zoh_ex's bytes: %s; with all three on, robots a limit cut: %d, robots with a counted flag: %d)"
        % (n_sub, same, cut, flagged))
    for name in names:
        say("  %-21s %s | / ex, nothing set %.4f" % (name, fmt(times[name]), summary(times[name])[0] / base))
    say("  io, all + everything / ex, everything %.4f" % (summary(times["io, all + everything"])[0] / summary(times["ex, everything"])[0]))
    if have_parent:
        allp = []
        for i, p in enumerate(parent):
            say("  parent, pass %d        %s" % (i + 1, fmt(p[str(n_sub)])))
            allp += p[str(n_sub)]
        meds = [summary(p[str(n_sub)])[0] for p in parent]
        say("  parent pass-to-pass: medians %.2f / %.2f ms (%.2f %%), range of all timings %.2f .. %.2f ms" % (meds[0], meds[1], 100.0 * abs(meds[0] - meds[1]) / min(meds), min(allp), max(allp)))
        for name in ("ex, nothing set", "io, nothing set"):
            m = summary(times[name])[0]
            say("  %-21s / parent median %.4f | inside the parent's own spread (or faster): %s" % (name, m / float(np.median(allp)), "PASS" if m <= max(allp) else "FAIL"))
write_lines(args.out, lines)
