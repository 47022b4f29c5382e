#!/usr/bin/env python3
"""What the rigid-contact plant inside the zero-order-hold loop (lmh_rollout_zoh_rigid) costs beside the host loop it replaces and beside
the compliant loop: 4096 standing robots (zoh_rate.py's start), 200 control ticks, n_substeps 1 and 10, fp64, both soles held, kv = 50.
Timed per n_substeps, HIP events around one launch (the host loop: around its 2 x ticks launches), medians with min..max, the rows of this
build interleaved launch by launch:
  host loop              ticks x { stand_step ; plant_step_rigid([0 | out.tau], DOUBLE, kv, n_substeps) }: what the call replaces
  zoh_rigid              lmh_rollout_zoh_rigid, LMH_RIGID_FIXED, nothing else set
  zoh_rigid, lam         the same with the multipliers of every control tick stored
  zoh_rigid, per tick    LMH_RIGID_PER_TICK, mode[j][i] = (i + j) % 3: a mode word read per control tick, RIGHT / LEFT / DOUBLE mixed
  zoh_io                 lmh_rollout_zoh_io with nothing set: the compliant loop (judged: inside the parent's spread, the kernel is unchanged)
  step, rigid            lmh_plant_step_rigid of ticks x n_substeps substeps under the torques of one evaluation (judged the same way)
  parent                 rollout_zoh_io and plant_step_rigid from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), each in two child processes of this one, one before
                         and one after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
  this build, child      the same two calls on this build in a child process of the same kind between the parent's two (judged too)
The zoh_rigid rows are reported relative to the host loop and to zoh_io, not judged: no ratio is fixed in advance.  Without a parent library
only this build is measured, and the output says so.
Usage: python scripts/zoh_rigid_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                        [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, have_parent, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

CALLS = ("rollout_zoh_io", "plant_step_rigid")
args = zoh_rate_args("rollout_zoh_io or plant_step_rigid (--call)", ("lmh_rollout_zoh_rigid",), calls=CALLS)
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt, DT, KV = args.instances, args.ticks, 1e-3, 50.0
q0, zcom = ik_start_posture(0)
q, v = standing(B, q0)
ctl = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * DT + 1.0, 2)
dev = ctl.device
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
out0, _ = ctl.stand_step(st0.clone())
zero6 = torch.zeros((B, 6), dtype=torch.float64, device=dev)
tau = torch.cat([zero6, out0[:, 0:24]], dim=1).contiguous()          # the torques a hold would see
io_of = lambda n: (lambda st: ctl.rollout_zoh_io(st, nt, n, out=out, status=status))
step_of = lambda n: (lambda st: ctl.plant_step_rigid(st, tau, None, KV, nt * n))
child_branch(args, io_of if args.call == "rollout_zoh_io" else step_of, st0.clone)


def parent_passes(variant=None):
    res = {}
    for call in CALLS:
        args.call = call
        res[call] = parent_pass(args, variant)
    return res


def host_loop_of(n, out=out, status=status):
    def loop(st):
        for _ in range(nt):
            ctl.stand_step(st, out, status)
            ctl.plant_step_rigid(st, torch.cat([zero6, out[:, 0:24]], dim=1), None, KV, n)
    return loop


say("zero-order-hold loop on the rigid-contact plant, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
    % (B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent(args):
    say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
parent = [parent_passes()] if have_parent(args) else []
lam = torch.zeros((nt, B, 12), dtype=torch.float64, device=dev)
per_tick = torch.as_tensor(((np.arange(B)[None, :] + np.arange(nt)[:, None]) % 3).astype(np.int32)).to(dev).contiguous()
mine = {}
for n_sub in args.substeps:
    zr = lambda **kw: (lambda st: ctl.rollout_zoh_rigid(st, nt, n_sub, kv=KV, out=out, status=status, **kw))
    rows = [("host loop", host_loop_of(n_sub)), ("zoh_rigid", zr()), ("zoh_rigid, lam", zr(lam=lam)), ("zoh_rigid, per tick", zr(mode=per_tick)),
            ("zoh_io", io_of(n_sub)), ("step, rigid", step_of(n_sub))]
    # the call against its host loop once, outside the timing, both from a fresh status record (the timed rows hand theirs on, warm start
    # included): the same bytes, and how many robots end with a counted flag
    sa, sb = st0.clone(), st0.clone()
    r = ctl.rollout_zoh_rigid(sa, nt, n_sub, kv=KV)
    host_loop_of(n_sub, ctl.new_out(), ctl.new_status())(sb)
    torch.cuda.synchronize()
    same = bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)))
    mine[n_sub] = (time_rows(args, rows, st0.clone), same, int(((r["status"][:, 2] & 15) != 0).sum()), [name for name, _ in rows])
child = parent_passes("") if parent else None
if parent:
    parent.append(parent_passes())
for n_sub in args.substeps:
    times, same, flagged, names = mine[n_sub]
    say("n_substeps %2d: (the call leaves the host loop's state bit for bit: %s; robots that end the loop with a counted flag: %d)" % (n_sub, same, flagged))
    host, io = summary(times["host loop"])[0], summary(times["zoh_io"])[0]
    for name in names:
        m = summary(times[name])[0]
        say("  %-22s %s | / host loop %.4f | / zoh_io %.4f" % (name, fmt(args, times[name]), m / host, m / io))
    zm = summary(times["zoh_rigid"])[0]
    say("  lmh_rollout_zoh_rigid is %s than the host loop it replaces (x %.3f)" % ("FASTER" if zm < host else "SLOWER", zm / host))
    for call, row in (("rollout_zoh_io", "zoh_io"), ("plant_step_rigid", "step, rigid")):
        if parent:
            say("  parent, %s:" % call)
            say("  %-22s %s" % ("this build, child", fmt(args, child[call][str(n_sub)])))
            parent_report(args, [p[call] for p in parent], n_sub, 22, [("%-22s" % row, summary(times[row])[0]), ("%-22s" % "this build, child", summary(child[call][str(n_sub)])[0])])
write_lines(args.out, lines)
