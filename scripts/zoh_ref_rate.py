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
ap.add_argument("--child", action="store_true", help="(internal) time the no-ref loop on the library LMH_VARIANT selects and print one JSON line")
ap.add_argument("--out", default=None)
args = ap.parse_args()

from linearmpchumanoid_amd import capi

if args.child:                                                     # a library of the parent tree has not got the new entry points
    for name in ("lmh_eval_ref", "lmh_rollout_zoh_ref"):
        capi.PROTOTYPES.pop(name, None)
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

assert torch.cuda.is_available(), "zoh_ref_rate.py measures on the GPU only"
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


def no_ref(n_sub):
    return time_launches(lambda st: ctl.rollout_zoh(st, nt, n_sub, out=out, status=status), args.steps, args.warmup, before=st0.clone)


if args.child:
    print(json.dumps({"times": {str(n): no_ref(n) for n in args.substeps}}))
    sys.exit(0)


def parent_pass():
    env = {k: val for k, val in os.environ.items() if k != "LMH_DIAG"}
    env["LMH_VARIANT"] = args.parent_variant
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--instances", str(B), "--ticks", str(nt), "--steps", str(args.steps),
                        "--warmup", str(args.warmup), "--substeps", *map(str, args.substeps)], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["times"]


have_parent = bool(args.parent_variant) and os.path.exists(os.path.join(ROOT, "linearmpchumanoid_amd", "liblmh_hip_var_%s.so" % args.parent_variant))
say("zero-order-hold loop with and without a caller-supplied CoM reference, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
    % (B, nt, torch.cuda.get_device_name(0), args.steps, args.warmup))
if not have_parent:
    say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
parent = [parent_pass()] if have_parent else []
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
    t_no, t_ref = [], []
    for _ in range(args.steps):                                    # alternating, one timed launch each (the first pair also warms up)
        t_no += time_launches(lambda s: ctl.rollout_zoh(s, nt, n_sub, out=out, status=status), 1, args.warmup if not t_no else 0, before=st0.clone)
        t_ref += time_launches(lambda s: ctl.rollout_zoh(s, nt, n_sub, out=out, status=status, ref=seq), 1, args.warmup if not t_ref else 0, before=st0.clone)
    mine[n_sub] = (t_no, t_ref, same, int((xa[:, 2] != 0).sum()))
if have_parent:
    parent.append(parent_pass())
fmt = lambda t: "%8.2f ms (%.2f .. %.2f, spread %.1f %%) = %.3f M ticks/s" % (summary(t)[0], summary(t)[1], summary(t)[2],
                                                                             100.0 * (max(t) - min(t)) / summary(t)[0], B * nt / summary(t)[0] / 1e3)
for n_sub in args.substeps:
    t_no, t_ref, same, flagged = mine[n_sub]
    m_no, m_ref = summary(t_no)[0], summary(t_ref)[0]
    say("n_substeps %2d:" % n_sub)
    say("  this build, no ref   %s" % fmt(t_no))
    say("  this build, ref      %s | ref / no ref %.4f (reported, not judged) | same bits as no ref %s, flagged robots %d" % (fmt(t_ref), m_ref / m_no, same, flagged))
    if have_parent:
        allp = []
        for i, p in enumerate(parent):
            say("  parent, pass %d       %s" % (i + 1, fmt(p[str(n_sub)])))
            allp += p[str(n_sub)]
        meds = [summary(p[str(n_sub)])[0] for p in parent]
        inside = m_no <= max(allp)
        say("  parent pass-to-pass: medians %.2f / %.2f ms (%.2f %%), range of all timings %.2f .. %.2f ms | this build no ref / parent median %.4f | "
            "inside the parent's own spread (or faster): %s" % (meds[0], meds[1], 100.0 * abs(meds[0] - meds[1]) / min(meds), min(allp), max(allp),
                                                              m_no / float(np.median(allp)), "PASS" if inside else "FAIL"))
write_lines(args.out, lines)
