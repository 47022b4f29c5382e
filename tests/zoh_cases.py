"""Shared cases of the zero-order-hold loop tests (test_zoh.py on the CPU, test_gpu_zoh.py on the GPU).

lmh_rollout_zoh is DEFINED as n_ticks rounds of { lmh_eval ; lmh_plant_step([base_wrench | out.tau], n_substeps) }.  oracle_zoh states that
loop with the CPU oracle's parts alone: Oracle.eval for the evaluation, plant_step_cases.oracle_plant_steps for the hold, and between the
two the stale velocity exactly as lmh_eval documents it -- the evaluation stores Robot::v_ <- v, the hold leaves it alone (its helper moves
the oracle's Robot::v_, so the loop puts the evaluation's v back).  The inputs are plant_step_cases.contact_states() with v_prev = v, t = 0.
Results are cached per process and never written by a test."""
import numpy as np

import plant_step_cases as pc

DT, TH, B = pc.DT, pc.TH, pc.B
ORACLE_RUN = (3, 2)               # control ticks x substeps of the run the GPU test holds against the oracle


def oracle_zoh(o, x0, n_ticks, n_substeps, base_wrench=None, t0=0.0, v_prev=None):
    """The loop on one robot: x0 = q | v [60], v_prev = Robot::v_ before the first evaluation (None: v, as after new_state(.., v_prev=v)).
    -> dict(state [60], v_prev [30], t, tau [24], f [12], qpp [30] of the last evaluation, k [n_ticks], qp_status [n_ticks],
    taus [n_ticks,24]).  The clock takes n_substeps additions of DT per tick (Clock::step's order)."""
    x, t = np.asarray(x0, dtype=np.float64).copy(), float(t0)
    bw = np.zeros(6) if base_wrench is None else np.asarray(base_wrench, dtype=np.float64)
    held = x[30:].copy() if v_prev is None else np.asarray(v_prev, dtype=np.float64).copy()
    last, ks, status, taus = None, [], [], []
    for _ in range(n_ticks):
        o.set_prev_velocity(held)                                  # Robot::v_ as the controller's own previous call left it
        last = o.eval(x[:30], x[30:], t)
        held = x[30:].copy()                                       # v_prev <- v (controller.cpp:59)
        ks.append(last["k"]); status.append(last["qp_status"]); taus.append(last["tau"].copy())
        x = pc.oracle_plant_steps(o, x, np.concatenate([bw, last["tau"]]), n_substeps)
        for _ in range(n_substeps):
            t += DT
    return dict(state=x, v_prev=held, t=t, tau=last["tau"], f=last["f"], qpp=last["qpp"], k=np.array(ks), qp_status=np.array(status),
                taus=np.array(taus))


_cache = {}


def oracle_run():
    """The 16 contact states through ORACLE_RUN, one fresh oracle per robot: list of oracle_zoh results (computed once, shared)."""
    if "run" not in _cache:
        S = pc.contact_states()
        _cache["run"] = [oracle_zoh(pc.make_oracle(), np.concatenate([S["q"][i], S["v"][i]]), *ORACLE_RUN) for i in range(B)]
    return _cache["run"]
