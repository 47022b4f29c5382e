#!/usr/bin/env python3
"""What the plastic touchdown impact costs: lmh_plant_impact_rigid beside lmh_plant_derivative_rigid, and lmh_rollout_zoh_rigid_impact
beside lmh_rollout_zoh_rigid.  4096 standing robots (zoh_rate.py's start), 200 control ticks, n_substeps 1 and 10, fp64, kv = 50.  Timed
per n_substeps, HIP events around one launch, medians with min..max, the rows of this build interleaved launch by launch:
  zoh_rigid                  lmh_rollout_zoh_rigid, LMH_RIGID_FIXED, both soles (judged: inside the parent's spread, the kernel is unchanged)
  impact, none lands         lmh_rollout_zoh_rigid_impact, enable = 1, the same modes, d_mode_prev = DOUBLE: no foot ever becomes held -- the
                             price of the check (a word loaded and stored per control tick, in another kernel); laid beside the parent's spread
  zoh_rigid, R/D per tick    lmh_rollout_zoh_rigid, LMH_RIGID_PER_TICK, mode[j] = RIGHT on even ticks and DOUBLE on odd ones
  impact, every 2nd tick     lmh_rollout_zoh_rigid_impact on those words: the left sole lands on every second control tick
  derivative | impact        (once, not per n_substeps) `ticks` launches back to back of plant_derivative_rigid and of plant_impact_rigid
  parent                     rollout_zoh_rigid from a library built from the parent commit (--parent-variant NAME loads
                             linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py) in two child processes of this one, one before and one
                             after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
  this build, child          the same call on this build in a child process of the same kind between the parent's two (judged too)
Without a parent library only this build is measured, and the output says so.
Usage: python scripts/rigid_impact_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                           [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, have_parent, lines, parent_pass, parent_report, say, standing, summary, time_launches, time_rows, write_lines, zoh_rate_args

args = zoh_rate_args("rollout_zoh_rigid", ("lmh_plant_impact_rigid", "lmh_rollout_zoh_rigid_impact"))
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt, DT, KV = args.instances, args.ticks, 1e-3, 50.0
q0, zcom = ik_start_posture(0)
q, v = standing(B, q0)
ctl = BatchedController(B, default_config(dt=DT, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * DT + 1.0, 2)
dev = ctl.device
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
rigid_of = lambda n, **kw: (lambda st: ctl.rollout_zoh_rigid(st, nt, n, kv=KV, out=out, status=status, **kw))
child_branch(args, rigid_of, st0.clone)

say("plastic impact of the rigid-contact plant, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
    % (B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent(args):
    say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
parent = [parent_pass(args)] if have_parent(args) else []
double = torch.zeros((B,), dtype=torch.int32, device=dev)
words = torch.as_tensor(np.tile(np.where(np.arange(nt) % 2 == 0, 1, 0).astype(np.int32)[:, None], (1, B))).to(dev).contiguous()
prev = torch.zeros((B,), dtype=torch.int32, device=dev)


def impact_of(n, mode, first):
    def launch(st):
        prev.fill_(first)
        return ctl.rollout_zoh_rigid(st, nt, n, mode=mode, kv=KV, out=out, status=status, impact=prev)
    return launch


mine = {}
for n_sub in args.substeps:
    rows = [("zoh_rigid", rigid_of(n_sub)), ("impact, none lands", impact_of(n_sub, None, 0)), ("zoh_rigid, R/D per tick", rigid_of(n_sub, mode=words)),
            ("impact, every 2nd tick", impact_of(n_sub, words, 1))]
    # once, outside the timing: no landing leaves the rigid call's bytes; how many robots meet an impulse that pulls
    sa, sb, sc = st0.clone(), st0.clone(), st0.clone()
    ctl.rollout_zoh_rigid(sa, nt, n_sub, kv=KV)
    prev.fill_(0)
    ctl.rollout_zoh_rigid(sb, nt, n_sub, kv=KV, impact=prev)
    prev.fill_(1)
    r = ctl.rollout_zoh_rigid(sc, nt, n_sub, mode=words, kv=KV, impact=prev, impulse=True)
    torch.cuda.synchronize()
    same = bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)))
    landed = int((r["impulse"].abs().amax(dim=2) > 0).sum(dim=0).min())
    mine[n_sub] = (time_rows(args, rows, st0.clone), same, landed, int(((r["status"][:, 2] & 1024) != 0).sum()), int(((r["status"][:, 2] & 15) != 0).sum()), [n for n, _ in rows])
child = parent_pass(args, "") if parent else None
if parent:
    parent.append(parent_pass(args))
for n_sub in args.substeps:
    times, same, landed, pulls, flagged, names = mine[n_sub]
    say("n_substeps %2d: (no landing leaves lmh_rollout_zoh_rigid's state bit for bit: %s; landings per robot in the R/D run: %d; robots with LMH_FLAG_IMPULSE_PULL: %d, with a "
        "counted flag: %d)" % (n_sub, same, landed, pulls, flagged))
    base = summary(times["zoh_rigid"])[0]
    for name in names:
        say("  %-24s %s | / zoh_rigid %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    a, b = summary(times["impact, every 2nd tick"])[0], summary(times["zoh_rigid, R/D per tick"])[0]
    say("  one landing costs %.4f ms per 4096-robot tick = %.2f %% of a control tick of the R/D run" % ((a - b) / (nt / 2), 100.0 * (a - b) / (nt / 2) / (b / nt)))
    if parent:
        say("  parent, rollout_zoh_rigid:")
        say("  %-24s %s" % ("this build, child", fmt(args, child[str(n_sub)])))
        parent_report(args, parent, n_sub, 24, [("%-24s" % "zoh_rigid", base), ("%-24s" % "this build, child", summary(child[str(n_sub)])[0]),
                                                ("%-24s" % "impact, none lands", summary(times["impact, none lands"])[0])])
# the two stand-alone calls, `ticks` launches back to back per timing, interleaved
qd, vd = st0[:, 0:30].contiguous(), st0[:, 30:60].contiguous()
tau = torch.zeros((B, 30), dtype=torch.float64, device=dev)
t = {"derivative": [], "impact": []}
for it in range(args.steps):
    t["derivative"] += time_launches(lambda: ctl.plant_derivative_rigid(qd, vd, tau, double, KV), 1, args.warmup if it == 0 else 0, reps=nt)
    t["impact"] += time_launches(lambda: ctl.plant_impact_rigid(qd, vd, double), 1, args.warmup if it == 0 else 0, reps=nt)
say("stand-alone calls, both soles held, ms per launch of %d robots (the wrapper's three allocations included in both):" % B)
for name in ("derivative", "impact"):
    m, lo, hi = summary(t[name])
    say("  plant_%s_rigid %8.4f ms (%.4f .. %.4f) | / derivative %.4f" % (name, m, lo, hi, m / summary(t["derivative"])[0]))
write_lines(args.out, lines)
