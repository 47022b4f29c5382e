#!/usr/bin/env python3
"""Does the closed loop stand on the rigid-contact plant, where nothing but the controller is left in the loop?  (A measurement of
lmh_plant_step_rigid, not a test.)  256 robots from rest at the IK start posture, both soles held (LMH_PHASE_DOUBLE), the host loop
    stand_step ; plant_step_rigid([0 | out.tau], DOUBLE, kv, n_substeps = 1)
for 2000 control ticks of 1 ms.  Falls are scored on the device after every tick by the metrics record's rule: down = !(q[2] >= z_min) or
!(|roll| <= tilt_max) or !(|pitch| <= tilt_max).
Run 1, the control: every robot with the default gains -- all alike; its first fall is laid beside the CPU loop's (oracle evaluation +
numpy statement: control tick 728 by this rule, where the tilt trips first; 816 by the height alone), and the largest |lambda - out.f| of
the run is printed: how far the wrench the constraint needs is from the wrench the controller planned.
Run 2, the controller's own gains through set_params, one robot per cell of a 16 x 16 grid:
    rows 0..14   kp_mom = s kp_mom0, kd_mom = sqrt(s) kd_mom0 (the damping ratio kept), s = 10^-1.5 .. 10^1.5, row 7 is s = 1
    row 15       the default momentum gains with w_foot raised a hundredfold
    columns      kp_joints = c kp_joints0, kd_joints = sqrt(c) kd_joints0, c = 10^-1.5 .. 10^1.5 (column 7 is c = 1) and c = 100
Reported: the first-fall tick of every cell (-1 = stood for the whole run), the cells that stand, the latest fall; and, because the contact is
bilateral, for the cells that stand whether a held foot ever pulled or left its friction disc (LMH_FLAG_CONTACT_PULL / _SLIP OR-ed over
the run) and where they are at the end: a cell that stands only by pulling on the ground does not stand on a real one.
--zoh: the same two runs, each as ONE launch of rollout_zoh_rigid with a metrics record (FIRST_FALL is the host loop's first-fall tick, the
multipliers and the log give |lambda - out.f|), which must reproduce the host loop's table; then, with the call in hand, run 2 again at
n_substeps = 10 (a control period of 10 ms) and with mode="plan" on a walking plan (gen_walk's defaults, x scale 0.03 m: the plan decides
which soles are held; there is no impact model and the contact stays bilateral).
--impact (with --zoh): the walking-plan run once more as rollout_zoh_rigid_impact -- the plastic impact at every touchdown of the plan,
d_mode_prev = the plan's first mode -- laid beside the run without it, with the cells that raise LMH_FLAG_IMPULSE_PULL / _SLIP counted.
Usage: python scripts/rigid_stand.py [--ticks 2000] [--kv 50] [--z-min 0.2] [--tilt-max 0.5] [--zoh [--impact]] [--out FILE]"""
import argparse

import numpy as np
import torch

from _bench_common import lines, say, write_lines

ap = argparse.ArgumentParser()
ap.add_argument("--ticks", type=int, default=2000)
ap.add_argument("--kv", type=float, default=50.0)
ap.add_argument("--z-min", type=float, default=0.2)
ap.add_argument("--tilt-max", type=float, default=0.5)
ap.add_argument("--zoh", action="store_true", help="one rollout_zoh_rigid launch per run instead of the host loop; then n_substeps = 10 and a walking plan")
ap.add_argument("--impact", action="store_true", help="with --zoh: the walking-plan run again with the plastic impact at every touchdown")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "rigid_stand.py runs on the GPU only"
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

G, DT, CPU_FALL, CPU_FALL_Z = 16, 1e-3, 728, 816
B = G * G
q0, zcom = ik_start_posture(0)
q, v = np.tile(q0, (B, 1)), np.zeros((B, 30))
cfg = default_config(dt=DT, time_horizon=0.016, z_com=zcom)
S = np.logspace(-1.5, 1.5, G - 1)
Cj = np.concatenate([S, [100.0]])


def run(ctl, control):
    """The host loop -> (first fall per robot [B] (-1: none), largest |lambda - out.f| of robot `control` over the ticks it stood, the
    tick and row it occurred at, plant flags OR-ed)"""
    dev = ctl.device
    st = ctl.new_state(q, v, t=0.0, v_prev=v)
    out, status = ctl.new_out(), ctl.new_status()
    zero6 = torch.zeros((B, 6), dtype=torch.float64, device=dev)
    first = torch.full((B,), -1, dtype=torch.int64, device=dev)
    gap = torch.zeros((args.ticks, 12), dtype=torch.float64, device=dev)
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    for tick in range(args.ticks):
        ctl.stand_step(st, out, status)
        _, lam, pf = ctl.plant_step_rigid(st, torch.cat([zero6, out[:, 0:24]], dim=1), None, args.kv, 1)
        flags |= pf
        gap[tick] = (lam[control] - out[control, 24:36]).abs()
        down = ~(st[:, 2] >= args.z_min) | ~(st[:, 3].abs() <= args.tilt_max) | ~(st[:, 4].abs() <= args.tilt_max)
        first = torch.where((first < 0) & down, torch.full_like(first, tick), first)
    torch.cuda.synchronize()
    first = first.cpu().numpy()
    n = args.ticks if first[control] < 0 else int(first[control])
    g = gap[:max(n, 1)].cpu().numpy()
    at = np.unravel_index(int(np.argmax(g)), g.shape)
    return first, float(g.max()), at, flags.cpu().numpy(), st


def run_zoh(ctl, control, n_substeps=1, mode=None, impact=None):
    """run() as one launch of rollout_zoh_rigid with a metrics record -> the same tuple.  impact: None | d_mode_prev (int32 [B])"""
    st = ctl.new_state(q, v, t=0.0, v_prev=v)
    m = ctl.new_metrics(args.z_min, args.tilt_max)
    r = ctl.rollout_zoh_rigid(st, args.ticks, n_substeps, mode=mode, kv=args.kv, lam=True, log=True, metrics=m, impact=impact)
    torch.cuda.synchronize()
    first = ctl.split_metrics(m.cpu().numpy())["first_fall"].astype(np.int64)
    n = args.ticks if first[control] < 0 else int(first[control])
    g = (r["lam"][:max(n, 1), control] - r["log"][:max(n, 1), control, 24:36]).abs().cpu().numpy()
    at = np.unravel_index(int(np.argmax(g)), g.shape)
    return first, float(g.max()), at, (r["status"][:, 2] & ~255).cpu().numpy(), st      # (the plant's informational flags: the bits above the controller's)


if args.zoh:
    run = run_zoh
ctl = BatchedController(B, cfg)
ctl.set_refs_stance(args.ticks * DT + 1.0, 2)
if args.zoh:
    say("each run below is ONE launch of rollout_zoh_rigid with a metrics record; the host loop's table: profiles/r33_rigid_stand.txt")
say("closed loop on the rigid-contact plant on %s: %d robots from rest, both soles held, kv = %g /s, n_substeps = 1, %d control ticks of %g s; down: z < %.2f m or tilt > %.2f rad"
    % (torch.cuda.get_device_name(0), B, args.kv, args.ticks, DT, args.z_min, args.tilt_max))
first, gap, at, flags, st = run(ctl, 0)
alike = bool((first == first[0]).all())
say("run 1, default gains: first fall at control tick %d (all %d robots alike: %s); the CPU loop's: %d by the same rule (%d by the height alone)" % (first[0], B, alike, CPU_FALL, CPU_FALL_Z))
say("  largest |lambda - out.f| while the robot stood: %.4g (row %d of n_R f_R n_L f_L, control tick %d); plant flags OR-ed over the run: %d"
    % (gap, at[1], at[0], int(np.bitwise_or.reduce(flags))))

ia, ib = np.divmod(np.arange(B), G)
s_mom = np.where(ia < G - 1, S[np.minimum(ia, G - 2)], 1.0)
fields = dict(kp_mom=cfg.kp_mom * s_mom, kd_mom=cfg.kd_mom * np.sqrt(s_mom), kp_joints=cfg.kp_joints * Cj[ib], kd_joints=cfg.kd_joints * np.sqrt(Cj[ib]),
              w_foot=np.where(ia == G - 1, 100.0 * cfg.w_foot, cfg.w_foot))
grid = BatchedController(B, cfg)
grid.set_refs_stance(args.ticks * DT + 1.0, 2)
grid.set_params(**fields)
control = 7 * G + 7
from linearmpchumanoid_amd import capi


def report(title, first2, gap2, flags2, st2):
    nonfinite = ~np.isfinite(st2[:, :60].cpu().numpy()).all(axis=1)
    say("")
    say("%s, the controller's gains, one robot per cell; control cell (row 7, column 7): first fall %d (run 1: %d), largest |lambda - out.f| %.4g" % (title, first2[control], first[0], gap2))
    say("  first fall per cell (rows: s on kp_mom, sqrt(s) on kd_mom; last row: w_foot x 100; columns: c on kp_joints, sqrt(c) on kd_joints; -1 = stood; * = end state not finite):")
    say("  %9s |" % "s \\ c" + "".join(" %7.3g" % c for c in Cj))
    for i in range(G):
        say("  %9s |" % ("w_foot" if i == G - 1 else "%.3g" % S[i]) + "".join(" %6d%s" % (first2[i * G + j], "*" if nonfinite[i * G + j] else " ") for j in range(G)))
    stood = [i for i in range(B) if first2[i] < 0 and not nonfinite[i]]
    best = max(range(B), key=lambda i: (args.ticks if first2[i] < 0 else first2[i]))
    say("  cells that stand for the whole run: %d of %d%s" % (len(stood), B, "" if not stood else ": " + ", ".join("(row %d, column %d)" % divmod(i, G) for i in stood)))
    end = st2.cpu().numpy()
    pulled = [i for i in stood if flags2[i] & capi.FLAG_CONTACT_PULL]
    slipped = [i for i in stood if flags2[i] & capi.FLAG_CONTACT_SLIP]
    say("  of the cells that stand: %d pulled on the ground at some tick, %d left the friction disc at some tick, %d did neither" % (len(pulled), len(slipped), len([i for i in stood if i not in pulled and i not in slipped])))
    if stood:
        say("  their end states: base height %.4f .. %.4f m (start %.4f), |pitch| <= %.4f rad, |roll| <= %.2e rad, largest |v| %.3e"
            % (end[stood, 2].min(), end[stood, 2].max(), q0[2], np.abs(end[stood, 4]).max(), np.abs(end[stood, 3]).max(), np.abs(end[stood, 30:60]).max()))
    say("  latest fall: cell (row %d, column %d) at control tick %s" % (*divmod(best, G), "none" if first2[best] < 0 else str(first2[best])))
    return stood


first2, gap2, at2, flags2, st2 = run(grid, control)
stood1 = report("run 2", first2, gap2, flags2, st2)
if args.zoh:
    f10, g10, _, fl10, st10 = run_zoh(grid, control, n_substeps=10)
    report("run 3, n_substeps = 10 (control period 10 ms; first falls in control ticks of 10 ms)", f10, g10, fl10, st10)
    walk = BatchedController(B, cfg)
    walk.set_xscale(np.full(B, 0.03))
    walk.gen_walk(args.ticks * DT + 1.0)
    walk.set_params(**fields)
    fw, gw, _, flw, stw = run_zoh(walk, control, mode="plan")
    report("run 4, mode=\"plan\" on gen_walk's default plan (step length 0.03 m), n_substeps = 1", fw, gw, flw, stw)
    if args.impact:
        phase = walk.get_refs()["phase"]
        prev = torch.full((B,), int(phase[0]) & 3, dtype=torch.int32, device=walk.device)       # no impact on the first tick
        fi, gi, _, fli, sti = run_zoh(walk, control, mode="plan", impact=prev)
        report("run 5, run 4 with the plastic impact at every touchdown of the plan (rollout_zoh_rigid_impact)", fi, gi, fli, sti)
        falls = lambda f: "%d .. %d" % (f[f >= 0].min(), f[f >= 0].max()) if (f >= 0).any() else "none"
        say("  first-fall ticks of the cells that fall: %s with the impact, %s without (round 36: 649 .. 1024); cells that raise LMH_FLAG_IMPULSE_PULL: %d of %d, "
            "LMH_FLAG_IMPULSE_SLIP: %d; later than without: %d cells, earlier: %d, the same tick: %d"
            % (falls(fi), falls(fw), int(((fli & capi.FLAG_IMPULSE_PULL) != 0).sum()), B, int(((fli & capi.FLAG_IMPULSE_SLIP) != 0).sum()),
               int((np.where(fi < 0, args.ticks, fi) > np.where(fw < 0, args.ticks, fw)).sum()), int((np.where(fi < 0, args.ticks, fi) < np.where(fw < 0, args.ticks, fw)).sum()),
               int((fi == fw).sum())))
write_lines(args.out, lines)
