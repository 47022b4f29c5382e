"""CPU side of the zero-order-hold loop (lmh_rollout_zoh): the oracle statement of the loop that the GPU parity test rests on is pinned
here, and the run the GPU test compares is shown to be a usable reference.  No GPU is used."""
import os
import re

import numpy as np

import plant_step_cases as pc
import zoh_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported(hip_lib):
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmh.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lmh_rollout_zoh\s*\(", src) and "lmh_rollout_zoh" in capi.EXPORTS and hasattr(hip_lib, "lmh_rollout_zoh")
    assert len(capi.PROTOTYPES["lmh_rollout_zoh"][1]) == 9 and callable(BatchedController.rollout_zoh)


def test_helper_is_the_written_out_loop():
    """oracle_zoh against the loop written out by hand on a second oracle, exactly: one tick without a hold is Oracle.eval; the second
    evaluation sees Robot::v_ = the v of the first one (not the velocity after the hold, which gives other torques); (a + b) ticks are (a)
    then (b) when the stale velocity and the clock are handed on; a base wrench enters rows 0..5 of the held tau30."""
    S = pc.contact_states()
    i = 3
    x0 = np.concatenate([S["q"][i], S["v"][i]])
    vp = np.random.default_rng(5).normal(0.0, 0.1, 30)
    o, o2 = pc.make_oracle(), pc.make_oracle()
    r = zc.oracle_zoh(o, x0, 1, 0, v_prev=vp)
    o2.set_prev_velocity(vp)
    e = o2.eval(x0[:30], x0[30:], 0.0)
    assert np.array_equal(r["tau"], e["tau"]) and np.array_equal(r["f"], e["f"]) and r["k"][0] == e["k"]
    assert np.array_equal(r["state"], x0) and np.array_equal(r["v_prev"], x0[30:]) and r["t"] == 0.0
    # two ticks of two substeps by hand
    bw = np.array([0.1, -0.2, 0.05, 1.0, -0.5, 2.0])
    r2 = zc.oracle_zoh(pc.make_oracle(), x0, 2, 2, base_wrench=bw)
    o2 = pc.make_oracle()
    o2.set_prev_velocity(x0[30:])
    e1 = o2.eval(x0[:30], x0[30:], 0.0)
    x1 = pc.oracle_plant_steps(o2, x0, np.concatenate([bw, e1["tau"]]), 2)
    t1 = (0.0 + pc.DT) + pc.DT
    o2.set_prev_velocity(x0[30:])                                  # the v of the first evaluation
    e2 = o2.eval(x1[:30], x1[30:], t1)
    x2 = pc.oracle_plant_steps(o2, x1, np.concatenate([bw, e2["tau"]]), 2)
    assert np.array_equal(r2["state"], x2) and np.array_equal(r2["tau"], e2["tau"]) and np.array_equal(r2["v_prev"], x1[30:])
    assert r2["t"] == (t1 + pc.DT) + pc.DT and list(r2["k"]) == [e1["k"], e2["k"]]
    o2.set_prev_velocity(x1[30:])                                  # the velocity after the hold instead: not the same torques
    assert not np.array_equal(o2.eval(x1[:30], x1[30:], t1)["tau"], e2["tau"])
    assert not np.array_equal(zc.oracle_zoh(pc.make_oracle(), x0, 2, 2)["state"], x2)      # the base wrench matters
    # splitting
    o3 = pc.make_oracle()
    a = zc.oracle_zoh(o3, x0, 1, 2, base_wrench=bw)
    b = zc.oracle_zoh(o3, a["state"], 1, 2, base_wrench=bw, t0=a["t"], v_prev=a["v_prev"])
    assert np.array_equal(b["state"], r2["state"]) and np.array_equal(b["tau"], r2["tau"]) and b["t"] == r2["t"]


def test_the_compared_run_is_a_usable_reference():
    """The 3 x 2 run of all 16 contact states: finite, the QP solved at every evaluation, and the preview index moves inside the run."""
    S = pc.contact_states()
    runs = zc.oracle_run()
    assert len(runs) == zc.B == 16 and zc.ORACLE_RUN == (3, 2)
    for i, r in enumerate(runs):
        assert np.isfinite(r["state"]).all() and np.isfinite(r["taus"]).all() and np.isfinite(r["f"]).all(), i
        assert not r["qp_status"].any(), (i, r["qp_status"])
        assert len(set(r["k"].tolist())) > 1 and list(r["k"]) == sorted(r["k"]), (i, r["k"])
        assert not np.array_equal(r["state"], np.concatenate([S["q"][i], S["v"][i]]))
