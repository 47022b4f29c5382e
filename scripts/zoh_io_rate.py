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
import numpy as np
import torch

from _bench_common import child_branch, fmt, head, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

args = zoh_rate_args("rollout_zoh_ex", ("lmh_rollout_zoh_io", "lmh_set_actuators", "lmh_actuators_per_instance", "lmh_get_actuators"))
from linearmpchumanoid_amd import capi, trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt = args.instances, args.ticks
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * 1e-3 + 1.0, 2)
q, v = standing(B, q0)
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
child_branch(args, lambda n: (lambda st: ctl.rollout_zoh_ex(st, nt, n, out=out, status=status)), st0.clone)

parent = head(args, "zero-order-hold loop and the options of lmh_rollout_zoh_io")
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
    times = time_rows(args, rows, st0.clone)
    mine[n_sub] = (times, same, int(((rc["status"][:, 2] & capi.FLAG_TAU_LIMIT) != 0).sum()), int(((rc["status"][:, 2] & 15) != 0).sum()), [name for name, _ in rows])
    ctl.set_pushes(None)
if parent:
    parent.append(parent_pass(args))
for n_sub in args.substeps:
    times, same, cut, flagged, names = mine[n_sub]
    base = summary(times["ex, nothing set"])[0]
    say("n_substeps %2d: (io with nothing set leaves rollout_zoh_ex's bytes: %s; with all three on, robots a limit cut: %d, robots with a counted flag: %d)"
        % (n_sub, same, cut, flagged))
    for name in names:
        say("  %-21s %s | / ex, nothing set %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    say("  io, all + everything / ex, everything %.4f" % (summary(times["io, all + everything"])[0] / summary(times["ex, everything"])[0]))
    if parent:
        parent_report(args, parent, n_sub, 21, [("%-21s" % name, summary(times[name])[0]) for name in ("ex, nothing set", "io, nothing set")])
write_lines(args.out, lines)
