#!/usr/bin/env python3
"""What the joint servo (lmh_set_servo, lmh_plant_step_servo, lmh_rollout_zoh_servo) costs in the torque-driven plant and the
zero-order-hold loop: 4096 standing robots (zoh_rate.py's start), 200 control ticks, n_substeps 1 and 10, fp64.
Timed per n_substeps, HIP events around one launch, medians with min..max, the rows of this build interleaved launch by launch:
  step                   lmh_plant_step of ticks x n_substeps substeps under the torques of one evaluation (judged: inside the parent's
                         spread, the kernel is unchanged)
  zoh_io                 lmh_rollout_zoh_io with the applied torques stored, so that lmh_rollout_zoh_io_kernel runs (judged the same way)
  step, servo            lmh_plant_step_servo on a handle with one record per robot (kp_j = 0.01 m_j / dt^2, kd_j = 0.1 m_j / dt on the joints'
                         own inertias at the start posture), setpoint = the start posture at rest
  zoh servo, mode 0      lmh_rollout_zoh_servo with mode 0 on that handle: lmh_rollout_zoh_io's launch, what the two rows below are held against
  zoh servo, integrate   LMH_SERVO_INTEGRATE: lmh_rollout_zoh_servo_kernel
  zoh servo, caller      LMH_SERVO_CALLER with a setpoint record per control tick and robot
  parent                 plant_step and rollout_zoh_io from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), each in two child processes of this one, one before
                         and one after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
  this build, child      the same two calls on this build in a child process of the same kind between the parent's two (judged too)
The servo rows are reported relative to this build's own rows without a servo, not judged.  Without a parent library only this build is
measured, and the output says so.
Usage: python scripts/servo_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                    [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, have_parent, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

CALLS = ("plant_step", "rollout_zoh_io")
args = zoh_rate_args("plant_step or rollout_zoh_io (--call)", ("lmh_set_servo", "lmh_servo_per_instance", "lmh_get_servo", "lmh_plant_step_servo", "lmh_rollout_zoh_servo"), calls=CALLS)
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt, DT = args.instances, args.ticks, 1e-3
q0, zcom = ik_start_posture(0)
q, v = standing(B, q0)


def handle():
    c = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
    c.set_refs_stance(nt * max(args.substeps) * DT + 1.0, 2)
    return c


ctl = handle()
dev = ctl.device
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
applied = torch.zeros((nt, B, 24), dtype=torch.float64, device=dev)
out0, _ = ctl.stand_step(st0.clone())
tau = torch.cat([torch.zeros((B, 6), dtype=torch.float64, device=dev), out0[:, 0:24]], dim=1).contiguous()   # the torques a hold would see
step_of = lambda c: (lambda n: (lambda st: c.plant_step(st, tau, nt * n)))
io_of = lambda c: (lambda n: (lambda st: c.rollout_zoh_io(st, nt, n, applied=applied, out=out, status=status)))
child_branch(args, step_of(ctl) if args.call == "plant_step" else io_of(ctl), st0.clone)


def parent_passes(variant=None):
    res = {}
    for call in CALLS:
        args.call = call
        res[call] = parent_pass(args, variant)
    return res


say("plant step and zero-order-hold loop with and without the joint servo, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
    % (B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent(args):
    say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
parent = [parent_passes()] if have_parent(args) else []
servo = handle()
M = servo.split_terms(servo.terms(torch.as_tensor(q[:B]).to(dev)).cpu().numpy())["M"][0]
m = 1.0 / np.diag(np.linalg.inv(M))[6:30]
servo.set_servo(np.tile(0.01 * m / DT ** 2, (B, 1)), np.tile(0.1 * m / DT, (B, 1)))
assert servo.servo_per_instance
sp = torch.as_tensor(np.concatenate([q[:, 6:30], np.zeros((B, 24))], axis=1)).to(dev).contiguous()
sp_seq = sp[None].repeat(nt, 1, 1).contiguous()
mine = {}
for n_sub in args.substeps:
    zsv = lambda sv: (lambda st: servo.rollout_zoh_servo(st, nt, n_sub, servo=sv, applied=applied, out=out, status=status))
    rows = [("step", step_of(ctl)(n_sub)), ("zoh_io", io_of(ctl)(n_sub)),
            ("step, servo", (lambda st: servo.plant_step_servo(st, sp, tau, nt * n_sub))),
            ("zoh servo, mode 0", zsv(None)), ("zoh servo, integrate", zsv("integrate")), ("zoh servo, caller", zsv(sp_seq))]
    flagged = []
    for sv in (None, "integrate"):
        r = servo.rollout_zoh_servo(st0.clone(), nt, n_sub, servo=sv)
        torch.cuda.synchronize()
        flagged.append(int(((r["status"][:, 2] & 15) != 0).sum()))
    mine[n_sub] = (time_rows(args, rows, st0.clone), flagged, [name for name, _ in rows])
child = parent_passes("") if parent else None
if parent:
    parent.append(parent_passes())
for n_sub in args.substeps:
    times, flagged, names = mine[n_sub]
    say("n_substeps %2d: (robots that end the loop with a counted flag: %d without the servo, %d with LMH_SERVO_INTEGRATE)" % (n_sub, *flagged))
    for name in names:
        base = summary(times["step" if name.startswith("step") else ("zoh servo, mode 0" if name.startswith("zoh servo") else "zoh_io")])[0]
        say("  %-22s %s | / its row without a servo %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    for call, row in (("plant_step", "step"), ("rollout_zoh_io", "zoh_io")):
        if parent:
            say("  parent, %s:" % call)
            say("  %-22s %s" % ("this build, child", fmt(args, child[call][str(n_sub)])))
            parent_report(args, [p[call] for p in parent], n_sub, 22, [("%-22s" % row, summary(times[row])[0]), ("%-22s" % "this build, child", summary(child[call][str(n_sub)])[0])])
write_lines(args.out, lines)
