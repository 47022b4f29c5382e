"""The scenarios of the rollout-trace tests (tests/test_gpu_trace.py), importable by the test process and by the child process that runs
the NaN-filled-LDS checker build: the traced launch, and the reference that cuts the same run into plain lmh_rollout launches of
`every` ticks and copies the three records back after each.

A sample is [state(96) | out(80) | status(4, as doubles)]; "equal" means equal as bytes, all 180 doubles of every sample.
Shapes: 16 robots of the mixed per-robot walking plan (push_cases.walking_controller) over 520 ticks -- two full 250-tick chunks and a
tail -- and, with the plant, push_cases.scenario_controller's standing robots (the reason is given there).
"""
import numpy as np
import torch

from helpers import same_bits as same_bytes
from plan_draw import DT, MPC_DT, N_PREVIEW, SIM_TIME, draw_walk_specs
from push_cases import Run, host_split, ik_posture, scenario_controller, walking_controller

TRACE_B, TRACE_NT = 16, 520
# (precision, plant, every, n_ticks): fp64 runs every tick (over 260 ticks: the reference is one launch per sample), a period that does
# not divide the chunk, exactly a chunk and more than a chunk; mixed and fp32 the period that does not divide the chunk; each with and
# without the plant
SPLIT_CASES = [(0, pl, ev, 260 if ev == 1 else TRACE_NT) for pl in (0, 1) for ev in (1, 7, 250, 260)] + \
              [(pr, pl, 7, TRACE_NT) for pr in (1, 2) for pl in (0, 1)]
# pushes of the push-rule test: around the first sample of every = 7 (end of tick 6), around the first hand-over between chunks (which
# is also the first sample of every = 250), and tick 0 (the chunk load of the launch)
PUSH_TICKS = {0: (0, 6, 7, 8, 249, 250, 251), 1: (6, 7, 8), 2: (249, 250, 251), 3: (7,), 4: (6,), 5: (8,), 6: (249,), 7: (250,), 8: (251,),
              9: (0,), 10: (0, 7, 250), 11: (6, 251), 12: (8, 249), 13: (7, 8), 14: (250, 251)}
ONLY_TICK_7, UNPUSHED = 3, 15
PUSH_SEED, PUSH_AMP = 20261019, 0.05


def case_controller(precision, plant, B=TRACE_B):
    if plant:
        return scenario_controller(1, precision=precision)          # its own 64 standing robots
    return walking_controller(B=B, precision=precision)


def cold_walking_controller(B=TRACE_B):
    """walking_controller with warm_start = 0: every evaluation starts its active set from scratch, so the state record alone restarts a run"""
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    q0, zcom = ik_posture()
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT, warm_start=0))
    sp, xs = draw_walk_specs(B)
    ctl.gen_walk_batch(SIM_TIME, sp)
    ctl.set_xscale(xs)
    return ctl, q0


def push_schedule(B=TRACE_B):
    """-> (ticks [B,7] int64 with -1 = unused, dv [B,7,30]): PUSH_TICKS with drawn planar base kicks of at most PUSH_AMP m/s per axis"""
    from linearmpchumanoid_amd import trajectories
    _, dv = trajectories.draw_pushes(B, 7, (1, 999), PUSH_AMP, PUSH_SEED)
    ticks = np.full((B, 7), -1, dtype=np.int64)
    for i, tk in PUSH_TICKS.items():
        ticks[i, :len(tk)] = tk
    return ticks, dv


def sample_of(res):
    """the three records of a result (push_cases.Run.result) as trace samples [B,180]"""
    return np.concatenate([res["state"], res["out"], res["status"].astype(np.float64)], axis=1)


def traced(ctl, q0, nt, every, state=None, log=True):
    """One traced launch from the start posture (or from `state`, a host array [B,96]).  -> dict(state, out, status, log, trace)"""
    st = ctl.new_state(q0, np.zeros(30), t=0.0) if state is None else torch.as_tensor(np.ascontiguousarray(state)).to(ctl.device)
    out, status, lg, tr = ctl.rollout_trace(st, nt, every, log=log)
    torch.cuda.synchronize()
    return dict(state=st.cpu().numpy(), out=out.cpu().numpy(), status=status.cpu().numpy(), log=None if lg is None else lg.cpu().numpy(),
                trace=tr.cpu().numpy())


def untraced(ctl, q0, nt):
    r = Run(ctl, q0)
    r.launch(nt)
    return r.result()


def split_trace(ctl, q0, nt, every, pushes=None):
    """The reference: plain lmh_rollout launches of `every` ticks on a handle of its own, the records copied back after each (status [1] /
    [2] merged as max / OR: push_cases.Run).  pushes = (ticks, dv): the handle has NO schedule and the host adds each dv itself
    (push_cases.host_split), stopping at the sample ticks as well.  -> (trace [nt // every, B, 180], launches)"""
    r = Run(ctl, q0)
    samples = []
    for j in range(nt // every):
        if pushes is None:
            r.launch(every)
        else:
            host_split(r, pushes[0], pushes[1], j * every, (j + 1) * every)
        samples.append(sample_of(r.result()))
    return np.stack(samples), len(r.logs)


def first_difference(a, b):
    """(sample, robot, double) of the first differing word of two traces, or None"""
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))
    return None if d.size == 0 else tuple(int(v) for v in d[0])


def trace_against_split(precision, plant, every, nt):
    """One case of SPLIT_CASES -> dict of the comparisons and of what makes them meaningful (JSON-serialisable)."""
    ctl, q0 = case_controller(precision, plant)
    got = traced(ctl, q0, nt, every)
    plain = untraced(ctl, q0, nt)
    ctl.close()
    ref_ctl, _ = case_controller(precision, plant)
    ref, launches = split_trace(ref_ctl, q0, nt, every)
    ref_ctl.close()
    final_diff = [k for k in ("state", "out", "status", "log") if not same_bytes(got[k], plain[k])]
    moving = float(np.abs(np.diff(got["trace"][:, :, :60], axis=0)).max()) if got["trace"].shape[0] > 1 else \
        float(np.abs(got["trace"][0, :, :30] - q0[None, :]).max())
    return dict(samples=int(got["trace"].shape[0]), launches=launches, first_diff=first_difference(got["trace"], ref), final_diff=final_diff,
                finite=bool(np.isfinite(got["trace"]).all() and np.isfinite(ref).all() and np.isfinite(got["log"]).all()),
                flags=int(np.bitwise_or.reduce(got["status"][:, 2])), trace_flags=int(np.bitwise_or.reduce(got["trace"][:, :, 178].astype(np.int64).ravel())),
                moving=moving)
