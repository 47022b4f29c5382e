"""What the timing scripts of this directory share (a private module, not a tool): the import path, bench.py's config-3 walkers, the
HIP-event timer with its median / min / max, say and the --out writer, and the parent-compare harness of the zoh_*_rate.py scripts (the
last section).  Importing it puts the repository root and tests/ on sys.path."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

DT, MPC_DT, N_PREVIEW = 1e-3, 1e-2, 32                              # config 3: dt = 1 ms, N = 32 x mpc_dt = 10 ms


def config3_gait(n_ticks):
    """-> (simulation time, gen_walk keywords) of bench.py's config-3 gait for launches of n_ticks."""
    sim = n_ticks * DT + 1.0
    return sim, dict(num_steps=max(2, int((sim - 0.3) / 0.5)), time_per_step=0.5, ds_time=0.2, step_height=0.02, settle_time=0.3)


def config3_walkers(B, n_ticks):
    """bench.py's config-3 workload on one handle: B warm-started walkers from the IK start posture on the config-3 gait.
    -> (ctl, q0, out, status, log [n_ticks,B,36])."""
    from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture
    q0, zcom = ik_start_posture(0)
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT, warm_start=1))
    ctl.set_xscale(np.array([np.random.default_rng(20260003 + i).uniform(0.02, 0.05) for i in range(B)]))     # bench.py's step lengths
    sim, gait = config3_gait(n_ticks)
    ctl.gen_walk(sim, **gait)
    log = torch.zeros((n_ticks, B, 36), dtype=torch.float64, device=ctl.device)
    return ctl, q0, ctl.new_out(), ctl.new_status(), log


def time_launches(launch, steps, warmup=1, reps=1, before=None):
    """Milliseconds per launch of `steps` timed groups after `warmup` untimed ones, from a HIP-event pair around `reps` launches back to
    back.  before() runs outside the pair, and what it returns (a fresh state) is handed to every launch of the group."""
    times = []
    for it in range(warmup + steps):
        fresh = (before(),) if before else ()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch(*fresh)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1) / reps)
    return times


def summary(times):
    """-> (median, min, max)"""
    return float(np.median(times)), min(times), max(times)


lines = []                                                          # what say() printed: the --out file


def say(s):
    print(s, flush=True)
    lines.append(s)


def write_lines(path, lines):
    """The --out file; no path, no file."""
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------- the zoh_*_rate.py scripts: this build against the parent
# Each script times rows of launches of this build, interleaved, and -- with --parent-variant NAME and linearmpchumanoid_amd/
# liblmh_hip_var_NAME.so in place (build.py) -- one launch on the parent's library in two child processes of itself, one before and one after
# its own rows: the parent's pass-to-pass spread in this session, which the judged rows are held to.
def zoh_rate_args(child_times, new_prototypes, calls=None):
    """The scripts' arguments.  In a child (--child: time `child_times` on the library LMH_VARIANT selects) the prototypes of the entry
    points the parent's library has not got are dropped; so call this before anything loads the library.  calls: the names a script that
    holds more than one call to the parent lets its child choose from (--call; parent_pass hands args.call on)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--substeps", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-variant", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) time %s on the library LMH_VARIANT selects and print one JSON line" % child_times)
    ap.add_argument("--out", default=None)
    if calls:
        ap.add_argument("--call", choices=calls, default=calls[0], help="(internal) the call a child times")
    args = ap.parse_args()
    if args.child:
        from linearmpchumanoid_amd import capi
        for name in new_prototypes:
            capi.PROTOTYPES.pop(name, None)
    assert torch.cuda.is_available(), "%s measures on the GPU only" % os.path.basename(sys.argv[0])
    return args


def standing(B, q0, seed=20261104):
    """zoh_rate.py's start: every sole vertex half a millimetre into the default ground, small velocities -> (q, v)"""
    rng = np.random.default_rng(seed)
    q = np.tile(q0, (B, 1)); q[:, 2] -= 5.0e-4
    v = np.zeros((B, 30)); v[:, 0:2] = rng.uniform(-0.05, 0.05, (B, 2)); v[:, 6:] = rng.normal(0.0, 0.01, (B, 24))
    return q, v


def child_branch(args, launch_of, before):
    """In a child: time launch_of(n_substeps) for every n_substeps, print the one JSON line and leave."""
    if args.child:
        print(json.dumps({"times": {str(n): time_launches(launch_of(n), args.steps, args.warmup, before=before) for n in args.substeps}}))
        sys.exit(0)


def have_parent(args):
    return bool(args.parent_variant) and os.path.exists(os.path.join(ROOT, "linearmpchumanoid_amd", "liblmh_hip_var_%s.so" % args.parent_variant))


def parent_pass(args, variant=None):
    """One child of this script on the parent's library (variant "": on this build's, timed the way the parent is) -> {str(n_substeps): times}"""
    env = {k: val for k, val in os.environ.items() if k != "LMH_DIAG"}
    env["LMH_VARIANT"] = args.parent_variant if variant is None else variant
    r = subprocess.run([sys.executable, os.path.abspath(sys.argv[0]), "--child", "--instances", str(args.instances), "--ticks", str(args.ticks), "--steps", str(args.steps),
                        "--warmup", str(args.warmup), "--substeps", *map(str, args.substeps), *(["--call", args.call] if getattr(args, "call", None) else [])], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["times"]


def head(args, title):
    """The first line(s) of the output and the parent's first pass -> [times] or []"""
    say("%s, %d robots x %d control ticks, fp64 (%s); %d timed launches after %d warm-up"
        % (title, args.instances, args.ticks, torch.cuda.get_device_name(0), args.steps, args.warmup))
    if not have_parent(args):
        say("no parent library (--parent-variant): this build only, nothing is compared with the parent")
    return [parent_pass(args)] if have_parent(args) else []


def time_rows(args, rows, before):
    """rows [(name, launch)] interleaved, one timed launch each per round (the first round also warms up) -> {name: times}"""
    times = {name: [] for name, _ in rows}
    for it in range(args.steps):
        for name, fn in rows:
            times[name] += time_launches(fn, 1, args.warmup if it == 0 else 0, before=before)
    return times


def fmt(args, t):
    m, lo, hi = summary(t)
    return "%8.2f ms (%.2f .. %.2f, spread %.1f %%) = %.3f M ticks/s" % (m, lo, hi, 100.0 * (hi - lo) / m, args.instances * args.ticks / m / 1e3)


def parent_report(args, parent, n_sub, width, judged, one_line=False):
    """The parent's two passes in a name column of `width`, their pass-to-pass spread, and for every (label, median of this build) of
    judged whether it lies inside the range of all the parent's timings (or below it); one_line: spread and verdict on one line."""
    allp = []
    for i, p in enumerate(parent):
        say("  %-*s %s" % (width, "parent, pass %d" % (i + 1), fmt(args, p[str(n_sub)])))
        allp += p[str(n_sub)]
    meds = [summary(p[str(n_sub)])[0] for p in parent]
    spread = "  parent pass-to-pass: medians %.2f / %.2f ms (%.2f %%), range of all timings %.2f .. %.2f ms" % (
        meds[0], meds[1], 100.0 * abs(meds[0] - meds[1]) / min(meds), min(allp), max(allp))
    verdicts = ["%s / parent median %.4f | inside the parent's own spread (or faster): %s" % (label, m / float(np.median(allp)), "PASS" if m <= max(allp) else "FAIL")
                for label, m in judged]
    if one_line:
        say(" | ".join([spread] + verdicts))
    else:
        say(spread)
        for v in verdicts:
            say("  " + v)
