#!/usr/bin/env python3
"""What the options of lmh_rollout_zoh_ex cost in the zero-order-hold loop, and that adding them cost the loop without one nothing:
4096 standing robots (zoh_rate.py's start), 200 control ticks, n_substeps 1 and 10, fp64.
Timed per n_substeps, HIP events around one launch, medians with min..max, the rows of this build interleaved launch by launch:
  rollout_zoh            lmh_rollout_zoh on this build (judged: inside the parent's spread, its code object is unchanged)
  ex, nothing set        rollout_zoh_ex without an option: the same kernel (judged the same way)
  ex, pushes             16 push records per robot inside the run (trajectories.draw_pushes: planar base kicks of up to 2 cm/s)
  ex, wrench sequence    a base wrench per control tick
  ex, metrics            the per-robot record
  ex, trace every 1 | every 10
  ex, everything         pushes, wrench sequence, metrics and the every-tick trace together
  parent                 rollout_zoh from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), in two child processes of this one, one before and one
                         after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
The option rows are reported relative to rollout_zoh, not judged.  Without a parent library only this build is measured, and the output says so.
Usage: python scripts/zoh_ex_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                     [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, head, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

args = zoh_rate_args("rollout_zoh", ("lmh_rollout_zoh_ex",))
from linearmpchumanoid_amd import capi, trajectories
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt = args.instances, args.ticks
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * 1e-3 + 1.0, 2)
q, v = standing(B, q0)
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
child_branch(args, lambda n: (lambda st: ctl.rollout_zoh(st, nt, n, out=out, status=status)), st0.clone)

parent = head(args, "zero-order-hold loop and the options of lmh_rollout_zoh_ex")
bw = torch.as_tensor(np.random.default_rng(20261105).normal(0.0, 0.5, (nt, B, 6))).to(ctl.device)
metrics = ctl.new_metrics(0.2, 0.5)
mine = {}
for n_sub in args.substeps:
    ticks, dv = trajectories.draw_pushes(B, 16, (1, nt * n_sub), 0.02, 20261106)         # 16 records per robot, all inside the run
    ctl.set_pushes(ticks, dv)
    tr1 = torch.zeros((nt, B, capi.TRACE_STRIDE), dtype=torch.float64, device=ctl.device)
    tr10 = torch.zeros((nt // 10, B, capi.TRACE_STRIDE), dtype=torch.float64, device=ctl.device)
    ex = lambda **kw: (lambda s: ctl.rollout_zoh_ex(s, nt, n_sub, out=out, status=status, **kw))
    rows = [("rollout_zoh", lambda s: ctl.rollout_zoh(s, nt, n_sub, out=out, status=status)),
            ("ex, nothing set", ex()),
            ("ex, pushes", ex(pushes=True)),
            ("ex, wrench sequence", ex(base_wrench=bw)),
            ("ex, metrics", ex(metrics=metrics)),
            ("ex, trace every 1", ex(trace_every=1, trace=tr1)),
            ("ex, trace every 10", ex(trace_every=10, trace=tr10)),
            ("ex, everything", ex(pushes=True, base_wrench=bw, metrics=metrics, trace_every=1, trace=tr1))]
    # what the launches leave: the plain call's bytes without an option, flag-free robots with everything on
    sa, sb, sc = st0.clone(), st0.clone(), st0.clone()
    oa, xa = ctl.rollout_zoh(sa, nt, n_sub)
    rb = ctl.rollout_zoh_ex(sb, nt, n_sub)
    rc = ctl.rollout_zoh_ex(sc, nt, n_sub, pushes=True, base_wrench=bw, metrics=ctl.new_metrics(0.2, 0.5), trace_every=1, trace=tr1)
    torch.cuda.synchronize()
    same = bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)) and torch.equal(oa.view(torch.int64), rb["out"].view(torch.int64)) and torch.equal(xa, rb["status"]))
    times = time_rows(args, rows, st0.clone)
    mine[n_sub] = (times, same, int(((rc["status"][:, 2] & 15) != 0).sum()), [name for name, _ in rows])
    ctl.set_pushes(None)
if parent:
    parent.append(parent_pass(args))
for n_sub in args.substeps:
    times, same, flagged, names = mine[n_sub]
    base = summary(times["rollout_zoh"])[0]
    say("n_substeps %2d: (ex with nothing set leaves rollout_zoh's bytes: %s; robots with a counted flag with everything on: %d)" % (n_sub, same, flagged))
    for name in names:
        say("  %-20s %s | / rollout_zoh %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    if parent:
        parent_report(args, parent, n_sub, 20, [("%-20s" % name, summary(times[name])[0]) for name in ("rollout_zoh", "ex, nothing set")])
write_lines(args.out, lines)
