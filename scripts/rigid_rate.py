#!/usr/bin/env python3
"""What the rigid-contact plant (lmh_plant_step_rigid) costs beside the compliant one (lmh_plant_step): 4096 standing robots (zoh_rate.py's
start), 200 control ticks, n_substeps 1 and 10, fp64.
Timed per n_substeps, HIP events around one launch, medians with min..max, the rows of this build interleaved launch by launch:
  step                   lmh_plant_step of ticks x n_substeps substeps under the torques of one evaluation (judged: inside the parent's
                         spread, the kernel is unchanged)
  step, rigid DOUBLE     lmh_plant_step_rigid of as many substeps under the same torques, both soles of every robot held, kv = 50
  step, rigid mix        the same with mode[i] = i % 3: RIGHT / LEFT / DOUBLE mixed over the batch
  parent                 plant_step from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py) in two child processes of this one, one before and one
                         after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
  this build, child      the same call on this build in a child process of the same kind between the parent's two (judged too)
The rigid rows are reported relative to this build's own `step` row, not judged: the rigid derivative does strictly more work.  Without a
parent library only this build is measured, and the output says so.
Usage: python scripts/rigid_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                    [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, head, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

args = zoh_rate_args("plant_step", ("lmh_plant_derivative_rigid", "lmh_plant_step_rigid"))
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt, DT, KV = args.instances, args.ticks, 1e-3, 50.0
q0, zcom = ik_start_posture(0)
q, v = standing(B, q0)
ctl = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * DT + 1.0, 2)
dev = ctl.device
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out0, _ = ctl.stand_step(st0.clone())
tau = torch.cat([torch.zeros((B, 6), dtype=torch.float64, device=dev), out0[:, 0:24]], dim=1).contiguous()   # the torques a hold would see
step_of = lambda n: (lambda st: ctl.plant_step(st, tau, nt * n))
child_branch(args, step_of, st0.clone)

parent = head(args, "plant step, compliant and rigid contact")
mix = torch.as_tensor((np.arange(B) % 3 + 1) % 3, dtype=torch.int32).to(dev)       # RIGHT, LEFT, DOUBLE, ...
mine = {}
for n_sub in args.substeps:
    rows = [("step", step_of(n_sub)),
            ("step, rigid DOUBLE", (lambda st: ctl.plant_step_rigid(st, tau, None, KV, nt * n_sub))),
            ("step, rigid mix", (lambda st: ctl.plant_step_rigid(st, tau, mix, KV, nt * n_sub)))]
    flagged = []
    for m in (None, mix):
        _, _, f = ctl.plant_step_rigid(st0.clone(), tau, m, KV, nt * n_sub)
        torch.cuda.synchronize()
        flagged.append(int(((f & 10) != 0).sum()))
    mine[n_sub] = (time_rows(args, rows, st0.clone), flagged, [name for name, _ in rows])
child = parent_pass(args, "") if parent else None
if parent:
    parent.append(parent_pass(args))
for n_sub in args.substeps:
    times, flagged, names = mine[n_sub]
    say("n_substeps %2d: (robots that end the rigid hold non-finite or with a rejected pivot: %d DOUBLE, %d mix)" % (n_sub, *flagged))
    base = summary(times["step"])[0]
    for name in names:
        say("  %-22s %s | / step %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    if parent:
        say("  %-22s %s" % ("this build, child", fmt(args, child[str(n_sub)])))
        parent_report(args, parent, n_sub, 22, [("%-22s" % "step", base), ("%-22s" % "this build, child", summary(child[str(n_sub)])[0])])
write_lines(args.out, lines)
