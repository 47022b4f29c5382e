#!/usr/bin/env python3
"""What a caller-supplied CoM reference costs in the zero-order-hold loop, and that adding it cost the loop without one nothing:
4096 standing robots (zoh_rate.py's start), 200 control ticks, n_substeps 1 and 10, fp64.
Timed per n_substeps, HIP events around one launch, medians with min..max:
  this build   rollout_zoh without ref and with ref, alternating.  The references are the launch's own -- out[:, 72:78] of every tick,
               collected by the built-in loop one tick per launch --, so both runs do the same physics and must leave the same bytes.
  parent       the same rollout_zoh without ref from a library built from the parent commit (--parent-variant NAME loads
               linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), in two child processes of this one, one before and one after
               this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
Judged: this build's no-ref median lies inside the range of the parent's timings (or below it).  Reported without a mark: the ref path
relative to the no-ref path.  Without a parent library only this build is measured, and the output says so.
Usage: python scripts/zoh_ref_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                      [--out FILE]"""
import torch

from _bench_common import child_branch, fmt, head, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

args = zoh_rate_args("the no-ref loop", ("lmh_eval_ref", "lmh_rollout_zoh_ref"))
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt = args.instances, args.ticks
q0, zcom = ik_start_posture(0)
ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.016, z_com=zcom))
ctl.set_refs_stance(nt * max(args.substeps) * 1e-3 + 1.0, 2)
q, v = standing(B, q0)
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
no_ref = lambda n_sub: (lambda st: ctl.rollout_zoh(st, nt, n_sub, out=out, status=status))
child_branch(args, no_ref, st0.clone)

parent = head(args, "zero-order-hold loop with and without a caller-supplied CoM reference")
mine = {}
for n_sub in args.substeps:
    # the launch's own references, collected one tick per launch
    st, x, seq = st0.clone(), ctl.new_status(), torch.zeros((nt, B, 16), dtype=torch.float64, device=ctl.device)
    for j in range(nt):
        o, x = ctl.rollout_zoh(st, 1, n_sub, status=x)
        seq[j, :, 0:6] = o[:, 72:78]
    sa, sb = st0.clone(), st0.clone()
    oa, xa = ctl.rollout_zoh(sa, nt, n_sub)
    ob, xb = ctl.rollout_zoh(sb, nt, n_sub, ref=seq)
    torch.cuda.synchronize()
    same = bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)) and torch.equal(oa.view(torch.int64), ob.view(torch.int64)) and torch.equal(xa, xb))
    times = time_rows(args, [("no ref", no_ref(n_sub)), ("ref", lambda s: ctl.rollout_zoh(s, nt, n_sub, out=out, status=status, ref=seq))], st0.clone)
    mine[n_sub] = (times["no ref"], times["ref"], same, int((xa[:, 2] != 0).sum()))
if parent:
    parent.append(parent_pass(args))
for n_sub in args.substeps:
    t_no, t_ref, same, flagged = mine[n_sub]
    m_no, m_ref = summary(t_no)[0], summary(t_ref)[0]
    say("n_substeps %2d:" % n_sub)
    say("  this build, no ref   %s" % fmt(args, t_no))
    say("  this build, ref      %s | ref / no ref %.4f (reported, not judged) | same bits as no ref %s, flagged robots %d" % (fmt(args, t_ref), m_ref / m_no, same, flagged))
    if parent:
        parent_report(args, parent, n_sub, 20, [("this build no ref", m_no)], one_line=True)
write_lines(args.out, lines)
