#!/usr/bin/env python3
"""What closing the box-constrained preview step inside the zero-order-hold loop costs (lmh_rollout_zoh_box), and that adding it cost the
loop without it nothing: 4096 standing robots (zoh_rate.py's start), 200 control ticks, n_substeps 1 and 10, fp64, dt = 1 ms, N = 32 samples
of mpc_dt = 10 ms.  Timed per n_substeps, HIP events around one launch (around the whole loop for the host loop), medians with min..max, the
rows of this build interleaved launch by launch:
  rollout_zoh            lmh_rollout_zoh on this build (judged: inside the parent's spread, its code object is unchanged)
  box, infinite          rollout_zoh_box with an all-infinite box: the factor and the solve of every tick, no working-set round
  box, binding           rollout_zoh_box on a left-foot stance plan with tests/zoh_box_cases.py's moved box (the plan's own ZMP lies outside it):
                         bounds active on every tick
  host loop, infinite | binding
                         the four launches per control tick the call replaces (lmh_eval on a scratch copy, lmh_mpc_box_step, lmh_eval_ref,
                         lmh_plant_step), with the copies between them
  box, N = 16 | N = 64   the two box rows on handles of those horizons (N = 64: mpc_dt = 5 ms)
  parent                 rollout_zoh from a library built from the parent commit (--parent-variant NAME loads
                         linearmpchumanoid_amd/liblmh_hip_var_NAME.so, see build.py), in two child processes of this one, one before and one
                         after this build's passes: their medians and ranges are the parent's own pass-to-pass spread in this session.
The box rows are reported relative to rollout_zoh and to the host loop, not judged.  Also reported: how far the loop under an infinite box is
from rollout_zoh after the run (the gain-row step and the factor solve agree to rounding only).
Usage: python scripts/zoh_box_rate.py [--instances 4096] [--ticks 200] [--substeps 1 10] [--steps 5] [--warmup 2] [--parent-variant NAME]
                                      [--out FILE]"""
import numpy as np
import torch

from _bench_common import child_branch, fmt, head, lines, parent_pass, parent_report, say, standing, summary, time_rows, write_lines, zoh_rate_args

args = zoh_rate_args("rollout_zoh", ("lmh_rollout_zoh_box",))
from linearmpchumanoid_amd import capi, trajectories as tj
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

B, nt = args.instances, args.ticks
DT = 1e-3
q0, zcom = ik_start_posture(0)
SIM = nt * max(args.substeps) * DT + 1.0


def handle(N, mpc_dt, support):
    c = BatchedController(B, default_config(dt=DT, time_horizon=N * mpc_dt + 1e-9, z_com=zcom, mpc_dt=mpc_dt))
    c.set_refs_stance(SIM, support)
    return c


def boxes(c, mpc_dt, support):
    """-> the all-infinite box (support 2) or the moved, always-binding box of a left-foot stance (support 1), [4, n_samples] on the device"""
    zx, zy = tj.stance_zmp(SIM, mpc_dt, support)
    n = capi.lib().lmh_num_ref_samples(c._h)
    assert n == len(zx)
    if support == 2:
        b = np.full((4, n), np.inf); b[0::2] = -np.inf
    else:
        b = tj.zmp_box(dict(zmp_x=zx, zmp_y=zy, phase=np.full(n, capi.PHASE_LEFT)), margin=0.015)
        b[0:2] -= 0.03; b[2:4] += 0.02
        assert (zy < b[2]).all()
    return torch.as_tensor(b).to(c.device)


q, v = standing(B, q0)
ctl = handle(32, 1e-2, 2)
st0 = ctl.new_state(q, v, t=0.0, v_prev=v)
out, status = ctl.new_out(), ctl.new_status()
child_branch(args, lambda n: (lambda st: ctl.rollout_zoh(st, nt, n, out=out, status=status)), st0.clone)


def host_loop(c, box, n_sub):
    """The loop the call replaces, on buffers made once."""
    scratch, o2, s2, lip = st0.clone(), c.new_out(), c.new_status(), torch.zeros((B, capi.LIP_STRIDE), dtype=torch.float64, device=c.device)
    zero = torch.zeros((B, 6), dtype=torch.float64, device=c.device)
    idx = torch.as_tensor([66, 69, 67, 70], device=c.device)

    def run(st):
        for _ in range(nt):
            scratch.copy_(st)
            c.stand_step(scratch, o2, s2)
            lip[:, 0:4] = o2[:, idx]
            lip[:, 4] = st[:, 90]
            m = c.mpc_box_step(lip, box)
            c.stand_step(st, out, status, ref=m)
            c.plant_step(st, torch.cat([zero, out[:, 0:24]], dim=1), n_sub)
    return run


parent = head(args, "zero-order-hold loop with the box-constrained preview step inside (lmh_rollout_zoh_box)")
left = handle(32, 1e-2, 1)
inf32, bind32 = boxes(ctl, 1e-2, 2), boxes(left, 1e-2, 1)
others = []
for N, mpc_dt in ((16, 1e-2), (64, 5e-3)):
    a, b = handle(N, mpc_dt, 2), handle(N, mpc_dt, 1)
    others.append((N, a, boxes(a, mpc_dt, 2), b, boxes(b, mpc_dt, 1)))
mine = {}
for n_sub in args.substeps:
    bx = lambda c, box: (lambda s: c.rollout_zoh_box(s, box, nt, n_sub, mpc=False, out=out, status=status))
    rows = [("rollout_zoh", lambda s: ctl.rollout_zoh(s, nt, n_sub, out=out, status=status)),
            ("box, infinite", bx(ctl, inf32)), ("box, binding", bx(left, bind32)),
            ("host loop, infinite", host_loop(ctl, inf32, n_sub)), ("host loop, binding", host_loop(left, bind32, n_sub))]
    for N, a, ia, b, bb in others:
        rows += [("box, infinite, N = %d" % N, bx(a, ia)), ("box, binding, N = %d" % N, bx(b, bb))]
    # what the launches leave: how far the infinite box is from the built-in step, whether bounds were active, flagged robots
    sa, sb, sc = st0.clone(), st0.clone(), st0.clone()
    ctl.rollout_zoh(sa, nt, n_sub)
    ri = ctl.rollout_zoh_box(sb, inf32, nt, n_sub)
    rb = left.rollout_zoh_box(sc, bind32, nt, n_sub)
    torch.cuda.synchronize()
    far = float((sa[:, 0:60] - sb[:, 0:60]).abs().max())
    info = dict(far=far, far_rel=far / float(sa[:, 0:60].abs().max()), active_inf=float(ri["mpc"][:, :, 15].max()), active_bind_min=float(rb["mpc"][:, :, 15].min()),
                flagged_inf=int(((ri["status"][:, 2] & 15) != 0).sum()), flagged_bind=int(((rb["status"][:, 2] & 15) != 0).sum()))
    del ri, rb
    times = time_rows(args, rows, st0.clone)
    mine[n_sub] = (times, info, [name for name, _ in rows])
if parent:
    parent.append(parent_pass(args))
for n_sub in args.substeps:
    times, info, names = mine[n_sub]
    base = summary(times["rollout_zoh"])[0]
    say("n_substeps %2d: infinite box against rollout_zoh after the run: max |q, v difference| %.3e (%.3e of max |q, v|); active samples under the infinite box: "
        "max %d, under the binding box: min %d; robots with a counted flag: %d (infinite), %d (binding)"
        % (n_sub, info["far"], info["far_rel"], info["active_inf"], info["active_bind_min"], info["flagged_inf"], info["flagged_bind"]))
    for name in names:
        say("  %-26s %s | / rollout_zoh %.4f" % (name, fmt(args, times[name]), summary(times[name])[0] / base))
    for kind in ("infinite", "binding"):
        say("  host loop / fused, %-9s %.3f" % (kind + ":", summary(times["host loop, " + kind])[0] / summary(times["box, " + kind])[0]))
    if parent:
        parent_report(args, parent, n_sub, 26, [("rollout_zoh", base)])
write_lines(args.out, lines)
