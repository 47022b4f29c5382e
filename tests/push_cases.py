"""The scenarios of the velocity-push tests (tests/test_gpu_pushes.py), importable by the test process and by the child process that runs
the NaN-filled-LDS checker build: the draw, the handles, the in-kernel run and the host that splits the launch at the push ticks.

Walking scenario: the mixed per-robot walking plan of tests/plan_draw.py (64 robots, dt = 1 ms, mpc_dt = 10 ms, N = 32, zero initial
velocity), three planar base kicks per robot from trajectories.draw_pushes -- U(-0.05, 0.05) m/s at distinct ticks of [1, 999), seed
PUSH_SEED -- and the first robots' ticks then overwritten with the corner cases (EDGE_TICKS): tick 0 (chunk load of the launch's first
chunk), 250 and 500 (hand-overs between 250-tick chunks), 249 / 250 / 251 (three ticks in a row across a hand-over), 999 (the last tick
of a 1000-tick launch), 1000 (not part of that launch: the record it writes must not hold it, a following launch applies it) and 5000
(never applied).
"""
import json
import os

import numpy as np
import torch

from helpers import bits_differ
from plan_draw import DT, MPC_DT, N_PREVIEW, SIM_TIME, draw_walk_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK_B, WALK_NT = 64, 1000
PUSH_SEED = 20261017
PUSH_AMP = 0.05
EDGE_TICKS = {0: (0, 300, 700), 1: (250, 10, 800), 2: (500, 20, 900), 3: (999, 30, 400), 4: (1000, 40, 600), 5: (5000, 50, 650),
              6: (0, 250, 500), 7: (999, 1000, 5000), 8: (249, 250, 251), 9: (0, 1, 2), 10: (750, 1000, 1001), 11: (1000, 5000, 6000)}
NEVER_IN_FIRST_LAUNCH = 11          # this robot's pushes all lie at or beyond tick 1000: inside the 1000-tick launch it is an unpushed robot


def ik_posture():
    ik = json.load(open(os.path.join(ROOT, "tests", "golden", "ik_posture.json")))
    return np.array(ik["q"]), float(ik["z_com"])


def walking_pushes(B=WALK_B):
    """-> (ticks [B,3] int64, dv [B,3,30]): the draw with the corner cases written over the first robots' ticks (their dv stay drawn)."""
    from linearmpchumanoid_amd import trajectories
    ticks, dv = trajectories.draw_pushes(B, 3, (1, 999), PUSH_AMP, PUSH_SEED)
    for i, tk in EDGE_TICKS.items():
        if i < B:
            ticks[i] = tk
    return ticks, dv


def walking_controller(B=WALK_B, **kw):
    """A handle on the mixed per-robot walking plan; kw: lmh_config overrides (precision, plant)."""
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    q0, zcom = ik_posture()
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT, warm_start=1, **kw))
    sp, xs = draw_walk_specs(B)
    ctl.gen_walk_batch(SIM_TIME, sp)
    ctl.set_xscale(xs)
    return ctl, q0


class Run:
    """State, out, status and the log of consecutive launches on one handle, merged as include/lmh.h says a split launch merges: state,
    out, status [0] and [3] of the last launch, [1] the maximum and [2] the OR over the launches, the log rows in order."""

    def __init__(self, ctl, q0, v0=None):
        self.ctl = ctl
        self.st = ctl.new_state(q0, np.zeros(30) if v0 is None else v0, t=0.0)
        self.out, self.status = ctl.new_out(), ctl.new_status()
        self.restart()

    def restart(self):
        """forget the launches so far (the records stay): what follows is compared on its own"""
        self.logs, self.itmax, self.flags = [], None, None

    def launch(self, nt):
        _, _, lg = self.ctl.rollout(self.st, nt, self.out, self.status, log=True)
        torch.cuda.synchronize()
        s = self.status.cpu().numpy()
        self.itmax = s[:, 1].copy() if self.itmax is None else np.maximum(self.itmax, s[:, 1])
        self.flags = s[:, 2].copy() if self.flags is None else (self.flags | s[:, 2])
        self.logs.append(lg.cpu().numpy())

    def add_dv(self, rows, dv):
        """what the host does between two launches: state[i, 30:60] += dv (one IEEE addition per component, on the device)"""
        self.st[torch.as_tensor(rows, device=self.st.device), 30:60] += torch.as_tensor(dv, device=self.st.device)

    def result(self):
        s = self.status.cpu().numpy().copy()
        s[:, 1], s[:, 2] = self.itmax, self.flags
        return dict(state=self.st.cpu().numpy().copy(), out=self.out.cpu().numpy().copy(), status=s, log=np.concatenate(self.logs, axis=0))


def host_split(run, ticks, dv, start, stop):
    """Ticks [start, stop) on a handle WITHOUT a schedule: launch by launch between the sorted distinct push ticks of that range, the
    host adding each dv to its robot's state[30:60] at those ticks."""
    cur = start
    for b in sorted({int(t) for t in np.asarray(ticks).ravel() if start <= t < stop}):
        if b > cur:
            run.launch(b - cur)
            cur = b
        rows, cols = np.nonzero(np.asarray(ticks) == b)
        run.add_dv(rows, dv[rows, cols])
    if stop > cur:
        run.launch(stop - cur)


def scenario_controller(plant, **kw):
    """plant = 0: the walking handle.  plant = 1: the same 64 robots, step lengths and control rates STANDING on the compliant contact
    (stance references): the compliant-contact plant does not carry the walking plan for 1000 ticks -- unpushed robots of the draw fall
    from tick ~640 on and end non-finite -- and a comparison of NaNs says nothing about a push."""
    if not plant:
        return walking_controller(**kw)
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    q0, zcom = ik_posture()
    ctl = BatchedController(WALK_B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT, warm_start=1, plant=1, **kw))
    ctl.set_refs_stance(SIM_TIME, 2)
    return ctl, q0


def in_kernel_against_split(precision=0, plant=0):
    """The walking scenario (plant = 1: the standing one, scenario_controller), one 1000-tick launch with the schedule set against host_split on a handle without one; then one more tick on
    both (the pushes at tick 1000).  -> dict of the comparisons (lists of differing fields) and of what makes them meaningful."""
    ticks, dv = walking_pushes()
    ctl, q0 = scenario_controller(plant, precision=precision)
    ctl.set_pushes(ticks, dv)
    k = Run(ctl, q0)
    k.launch(WALK_NT)
    first = k.result()
    k.restart()
    k.launch(1)                                                     # the following 1-tick launch: the pushes at tick 1000
    nxt = k.result()
    ctl.close()
    ref_ctl, _ = scenario_controller(plant, precision=precision)
    assert ref_ctl.get_pushes(0)["ticks"].size == 0
    r = Run(ref_ctl, q0)
    host_split(r, ticks, dv, 0, WALK_NT)
    ref, n_launches = r.result(), len(r.logs)
    r.restart()
    host_split(r, ticks, dv, WALK_NT, WALK_NT + 1)
    ref_nxt = r.result()
    plain = Run(ref_ctl, q0)                                        # the same robots never pushed: the pushes must matter
    plain.launch(WALK_NT)
    unpushed = plain.result()
    plain.restart()
    plain.launch(1)
    unpushed_nxt = plain.result()
    ref_ctl.close()
    moved = np.abs(first["state"][:, :60] - unpushed["state"][:, :60]).max(axis=1)
    n = NEVER_IN_FIRST_LAUNCH
    return dict(diff=bits_differ(first, ref), diff_next=bits_differ(nxt, ref_nxt), diff_never=bits_differ(first, unpushed, rows=slice(n, n + 1)),
                # the robot that was unpushed so far: after the launch that starts at tick 1000 it is a pushed robot
                next_applied=bool(np.abs(nxt["state"][n, :60] - unpushed_nxt["state"][n, :60]).max() > 0),
                nonfinite_robots=int((~(np.isfinite(first["state"][:, :60]).all(axis=1) & np.isfinite(first["log"]).all(axis=(0, 2)))).sum()),
                launches=n_launches, finite=bool(np.isfinite(first["log"]).all()), flags=int(np.bitwise_or.reduce(first["status"][:, 2])),
                robots_moved=int((moved > 0).sum()), robots_pushed=int((ticks < WALK_NT).any(axis=1).sum()))
