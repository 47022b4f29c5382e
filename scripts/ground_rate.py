#!/usr/bin/env python3
"""What a ground table (lmh_set_ground) costs in the torque-driven plant and the zero-order-hold loop: 4096 standing robots (zoh_rate.py's
start), 200 control ticks, n_substeps 1 and 10, fp64.
Timed per n_substeps, HIP events around one launch, medians with min..max, the rows of this build interleaved launch by launch:
  step, no table         lmh_plant_step of ticks x n_substeps substeps under the torques of one evaluation, on a handle without a table
                         (judged: inside the parent's spread, the kernel is unchanged)
  zoh, no table          lmh_rollout_zoh on that handle (judged the same way)
  step, per-robot table  lmh_plant_step on a handle with one record per robot: slopes of 0 .. 3 degrees in random directions through the
                         start's contact patch (how many robots end a launch with a counted flag, with and without the table, is reported: the
                         loop does not keep a robot up for long on either ground, DESIGN round 16)
  zoh, per-robot table   lmh_rollout_zoh on that handle: lmh_rollout_zoh_ground_kernel instead of lmh_rollout_zoh_ex_kernel
  parent                 the two calls without a table from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), each in two child processes of this one, one before
                         and one after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
  this build, child      the same two calls on this build in a child process of the same kind between the parent's two (judged too: a
                         child runs one call back to back, the interleaved rows above run it behind three other kernels)
The table rows are reported relative to this build's own no-table rows, not judged.  Without a parent library only this build is measured, and
the output says so.
Usage: python scripts/ground_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                     [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, have_parent, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

CALLS = ("plant_step", "rollout_zoh")
args = zoh_rate_args("plant_step or rollout_zoh (--call)", ("lmh_set_ground", "lmh_ground_per_instance", "lmh_get_ground"), calls=CALLS)
from linearmpchumanoid_amd import trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt = args.instances, args.ticks
q0, zcom = ik_start_posture(0)
q, v = standing(B, q0)


def handle():
    c = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
    c.set_refs_stance(nt * max(args.substeps) * 1e-3 + 1.0, 2)
    return c


ctl = handle()
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
out0, _ = ctl.stand_step(st0.clone())
tau = torch.cat([torch.zeros((B, 6), dtype=torch.float64, device=ctl.device), out0[:, 0:24]], dim=1).contiguous()   # the torques a hold would see
step_of = lambda c: (lambda n: (lambda st: c.plant_step(st, tau, nt * n)))
zoh_of = lambda c: (lambda n: (lambda st: c.rollout_zoh(st, nt, n, out=out, status=status)))
child_branch(args, step_of(ctl) if args.call == "plant_step" else zoh_of(ctl), st0.clone)


def parent_passes(variant=None):
    res = {}
    for call in CALLS:
        args.call = call
        res[call] = parent_pass(args, variant)
    return res


say("plant step and zero-order-hold loop with and without a ground table, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
    % (B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent(args):
    say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
parent = [parent_passes()] if have_parent(args) else []
ground = handle()
rng = np.random.default_rng(20261026)
slope, az = np.deg2rad(rng.uniform(0.0, 3.0, B)), rng.uniform(-np.pi, np.pi, B)
rec = trajectories.ground_planes(slope, az)
# through the point under the base on the flat ground: the plane turns about the middle of the contact patch
rec[:, 3] = rec[:, 7] = rec[:, 0] * q[:, 0] + rec[:, 1] * q[:, 1]
ground.set_ground(rec)
mine = {}
for n_sub in args.substeps:
    rows = [("step, no table", step_of(ctl)(n_sub)), ("zoh, no table", zoh_of(ctl)(n_sub)),
            ("step, per-robot table", step_of(ground)(n_sub)), ("zoh, per-robot table", zoh_of(ground)(n_sub))]
    _, sa = ctl.rollout_zoh(st0.clone(), nt, n_sub)
    _, sb = ground.rollout_zoh(st0.clone(), nt, n_sub)
    torch.cuda.synchronize()
    times = time_rows(args, rows, st0.clone)
    mine[n_sub] = (times, int(((sa[:, 2] & 15) != 0).sum()), int(((sb[:, 2] & 15) != 0).sum()), [name for name, _ in rows])
child = parent_passes("") if parent else None
if parent:
    parent.append(parent_passes())
for n_sub in args.substeps:
    times, flagged0, flagged, names = mine[n_sub]
    say("n_substeps %2d: (robots that end rollout_zoh with a counted flag: %d without a table, %d with it)" % (n_sub, flagged0, flagged))
    for name in names:
        base = summary(times[name.split(",")[0] + ", no table"])[0]
        say("  %-22s %s | / its no-table row %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    for call, row in (("plant_step", "step, no table"), ("rollout_zoh", "zoh, no table")):
        if parent:
            say("  parent, %s:" % call)
            say("  %-22s %s" % ("this build, child", fmt(args, child[call][str(n_sub)])))
            parent_report(args, [p[call] for p in parent], n_sub, 22, [("%-22s" % row, summary(times[row])[0]), ("%-22s" % "this build, child", summary(child[call][str(n_sub)])[0])])
write_lines(args.out, lines)
