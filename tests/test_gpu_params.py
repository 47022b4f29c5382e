"""Per-robot gains, QP weights, friction and contact parameters (include/lmh.h, lmh_set_params) on the GPU.

The yardstick of the first five tests is bit equality with shared handles: robot i of a handle with per-robot parameters must equal, with
np.array_equal, robot i of a handle created with parameter set i as its config and given the same states -- same kernel, same arithmetic,
no tolerance.  The oracle comparisons use the rules of the existing gains and plant parity tests (tests/test_gpu_round2.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import TOL_REL, WEIGHT, cfg2, close, oracle_system, perturbed_velocities  # noqa: F401
from params_cases import PLANT_SETS, SIX_SETS, assert_robot_equal, columns, make_controller, run, states

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def six(cfg2):
    """six robots, six parameter sets on one handle: computed once, read by the shared-handle test and by the oracle test"""
    B = len(SIX_SETS)
    v, vprev = states(B, 321)
    ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    ctl.set_params(**columns(SIX_SETS, ctl.cfg))
    assert ctl.params_per_instance()
    res = run(ctl, cfg2["q0"], v, vprev)
    ctl.close()
    return dict(v=v, vprev=vprev, res=res)


# ------------------------------------------------------------------------------- 1. six robots, six sets, against shared handles
def test_six_sets_equal_shared_handles_bit_for_bit(cfg2, six):
    B = len(SIX_SETS)
    for part in six["res"].values():
        assert (part["status"][:, 2] == 0).all()
    for i, over in enumerate(SIX_SETS):
        ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1, **over)
        assert not ctl.params_per_instance()
        shared = run(ctl, cfg2["q0"], six["v"], six["vprev"])
        ctl.close()
        assert_robot_equal(six["res"], shared, i, over)
    # the sets do differ: a handle that ignored its records would have every robot on the defaults
    ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    dflt = run(ctl, cfg2["q0"], six["v"], six["vprev"], ticks=0)
    ctl.close()
    for i in range(1, B):
        assert not np.array_equal(six["res"]["eval0"]["out"][i], dflt["eval0"]["out"][i]), i
    # the plain (two-wave) and the debug (single-wave) schedule agree on every robot, as on a shared handle
    for ph in (0, 1):
        e = six["res"]["eval%d" % ph]
        assert np.array_equal(e["out"], e["out_dbg"])


# ------------------------------------------------------------------------------- 2. the same six robots against one oracle each
def test_six_sets_against_one_oracle_each(cfg2, six):
    res, v, vprev = six["res"], six["v"], six["vprev"]
    for i, over in enumerate(SIX_SETS):
        for ph in (0, 1):
            out = res["eval%d" % ph]["out"]
            o = oracle_system(cfg2["dt"], cfg2["th"])
            o.set_gains(**over)
            zx, zy = o.zmp()
            o.set_refs(zx, zy, np.full(len(zx), ph, dtype=np.uint8))
            o.set_prev_velocity(vprev[i])
            e = o.eval(cfg2["q0"], v[i], 0.0)
            assert close(out[i, :24], e["tau"]) and close(out[i, 24:36], e["f"], scale=WEIGHT) and close(out[i, 36:66], e["qpp"]), (ph, i)
            if "mu" in over:
                fx, fy, fz = out[i, 24 + 3:24 + 6]
                assert abs(fx) <= over["mu"] * fz + 1e-7 and abs(fy) <= over["mu"] * fz + 1e-7
        o = oracle_system(cfg2["dt"], cfg2["th"])
        o.set_gains(**over)
        r = o.rollout(np.concatenate([cfg2["q0"], v[i]]), 0.0, 30, log=True)
        log = res["rollout"]["log"]
        assert res["rollout"]["status"][i, 0] == r["k"][-1]
        for tk in range(0, 30, 4):
            assert close(log[tk, i, :24], r["log"][tk][:24], TOL_REL) and close(log[tk, i, 24:], r["log"][tk][24:], TOL_REL, scale=WEIGHT), (i, tk)


# ------------------------------------------------------------------------------- 3. the plant's ground, per robot
def test_plant_contact_constants_per_robot(cfg2):
    """plant = 1, four robots on four grounds, 40 ticks: bit-equal to shared handles, and against the oracle's plant at the tolerance of
    test_gpu_round2.test_plant_rollout_parity_and_physics."""
    from oracle.pyoracle import Oracle
    dt, th, nt = 1e-3, 0.032, 40
    B = len(PLANT_SETS)
    v = perturbed_velocities(B, seed=31337) * 0.2
    v[0] = 0.0

    def roll(ctl):
        ctl.set_refs_stance(2.0, 2)
        st = ctl.new_state(cfg2["q0"], v, t=0.0)
        out, status, log = ctl.rollout(st, nt, log=True)
        torch.cuda.synchronize()
        return dict(rollout=dict(out=out.cpu().numpy()[:, :78], state=st.cpu().numpy(), status=status.cpu().numpy(), log=log.cpu().numpy()))

    ctl = make_controller(B, dt, th, cfg2["zcom"], warm_start=1, plant=1)
    ctl.set_params(**columns(PLANT_SETS, ctl.cfg))
    res = roll(ctl)
    ctl.close()
    assert (res["rollout"]["status"][:, 2] == 0).all()
    for i, contact in enumerate(PLANT_SETS):
        ctl = make_controller(B, dt, th, cfg2["zcom"], warm_start=1, plant=1, **contact)
        shared = roll(ctl)
        ctl.close()
        assert_robot_equal(res, shared, i, contact)
        o = Oracle(sim_time=2.0, dt=dt, horizon_time=th, do_ik=True)
        o.set_zcom(cfg2["zcom"])
        o.set_plant(True, k=contact["contact_k"], d=contact["contact_d"], dt=contact["contact_dt"], mu=contact["contact_mu"])
        r = o.rollout(np.concatenate([cfg2["q0"], v[i]]), 0.0, nt, log=True)
        stn, log = res["rollout"]["state"], res["rollout"]["log"]
        assert res["rollout"]["status"][i, 0] == r["k"][-1]
        assert close(stn[i, :60], r["state"], 1e-6), (i, np.abs(stn[i, :60] - r["state"]).max())
        for tk in range(0, nt, 7):
            assert close(log[tk, i, :24], r["log"][tk][:24]) and close(log[tk, i, 24:], r["log"][tk][24:], scale=WEIGHT), (i, tk)
    assert not np.array_equal(res["rollout"]["state"][2, :60], shared["rollout"]["state"][2, :60])      # robots 2 and 3 stand on different grounds


# ------------------------------------------------------------------------------- 4. one workgroup, several robots
def test_workgroup_reuse_in_a_child_process():
    """300 robots alternating between two parameter sets, one workgroup per CU (LMH_ROLLOUT_GROUPS_PER_CU is read once per process, hence
    the child), 260 ticks so that units also change hands through the ring: every robot bit-equal to its counterpart in two shared handles
    run on all 300 states.  The smallest shape at which a cache or an LDS table left over from the previous robot on a workgroup shows."""
    env = dict(os.environ, LMH_ROLLOUT_GROUPS_PER_CU="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "params_reuse_child.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "reuse ok: 300 robots" in r.stdout, r.stdout[-2000:]


# ------------------------------------------------------------------------------- 5. the other precisions
@pytest.mark.parametrize("precision", [1, 2], ids=["mixed", "fp32"])
def test_other_precisions_equal_shared_handles(cfg2, precision):
    sets = SIX_SETS[:4]
    B = len(sets)
    v, vprev = states(B, 654)

    def go(ctl):
        return run(ctl, cfg2["q0"], v, vprev, phases=(0,), ticks=10)

    ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1, precision=precision)
    ctl.set_params(**columns(sets, ctl.cfg))
    res = go(ctl)
    ctl.close()
    for i, over in enumerate(sets):
        ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1, precision=precision, **over)
        shared = go(ctl)
        ctl.close()
        assert_robot_equal(res, shared, i, over)
    assert not np.array_equal(res["rollout"]["state"][0, 30:60], res["rollout"]["state"][1, 30:60])


# ------------------------------------------------------------------------------- 6. setter semantics
def test_setter_semantics(cfg2):
    import ctypes as C
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.capi import LmhError
    from linearmpchumanoid_amd.controller import nominal_links, param_records
    B = 12
    v, vprev = states(B, 987)
    q0 = cfg2["q0"]

    def go(ctl):
        return run(ctl, q0, v, vprev, phases=(1,), ticks=12)

    def same(a, b):
        for i in range(B):
            assert_robot_equal(a, b, i)

    fresh_ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    fresh = go(fresh_ctl)
    qd = torch.as_tensor(np.tile(q0, (B, 1))).to(fresh_ctl.device)
    vd = torch.as_tensor(v).to(fresh_ctl.device)
    terms0 = fresh_ctl.terms(qd, vd).cpu().numpy()

    ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    for i in (0, B - 1):                                            # without per-robot parameters: the config's values for every robot
        assert ctl.get_params(i) == {n: getattr(ctl.cfg, n) for n in capi.PARAM_FIELDS}
    fields = dict(kp_joints=np.linspace(250.0, 350.0, B), mu=np.linspace(0.4, 0.8, B), w_com_ang=np.where(np.arange(B) % 2, 30.0, 0.0), w_foot=8.0e4)
    ctl.set_params(**fields)
    assert ctl.params_per_instance()
    rec = param_records(ctl.cfg, B, **fields)
    for i in range(B):                                              # round trip
        assert ctl.get_params(i) == {n: rec[i, o] for n, o in capi.PARAM_FIELDS.items()}
    base = go(ctl)
    assert not np.array_equal(base["rollout"]["state"], fresh["rollout"]["state"])
    # terms() reads none of these fields
    assert np.array_equal(ctl.terms(qd, vd).cpu().numpy(), terms0)

    # refused calls: the previous set stays and results do not change
    ptr = rec.ctypes.data_as(C.c_void_p)
    assert capi.lib().lmh_set_params(ctl._h, ptr, B - 1) == -2       # n != B (LMH_ERR_BAD_ARG)
    with pytest.raises(LmhError, match="robot 7: .*weights") as ei:  # a non-positive weight at robot 7
        ctl.set_params(**dict(fields, w_joints=np.where(np.arange(B) == 7, 0.0, 1.0)))
    assert ei.value.code == -2
    with pytest.raises(ValueError):                                  # a NaN gain: refused in Python ...
        ctl.set_params(**dict(fields, kd_mom=np.where(np.arange(B) == 3, np.nan, 6.0)))
    bad = rec.copy()
    bad[3, capi.PARAM_FIELDS["kd_mom"]] = np.nan                    # ... and by the library itself
    assert capi.lib().lmh_set_params(ctl._h, bad.ctypes.data_as(C.c_void_p), B) == -2
    assert b"robot 3: " in capi.lib().lmh_last_error()
    assert ctl.params_per_instance()
    for i in range(B):
        assert ctl.get_params(i) == {n: rec[i, o] for n, o in capi.PARAM_FIELDS.items()}
    same(go(ctl), base)

    # set_params() with no arguments: a fresh handle
    ctl.set_params()
    assert not ctl.params_per_instance()
    assert ctl.get_params(5) == {n: getattr(ctl.cfg, n) for n in capi.PARAM_FIELDS}
    same(go(ctl), fresh)
    ctl.close()
    fresh_ctl.close()

    # the stale-pointer hazard: the other table setters after set_params give what they give before it
    raw = np.tile(nominal_links(), (B, 1, 1)) * (1.0 + 0.04 * np.linspace(-1.0, 1.0, B))[:, None, None]
    zc = cfg2["zcom"] * (1.0 + 0.02 * np.linspace(-1.0, 1.0, B))
    specs = dict(num_steps=2, time_per_step=np.linspace(0.3, 0.4, B), ds_time=0.01, settle_time=0.005)     # single support from tick 15 on
    ticks = np.full((B, 1), 4)
    dv = np.zeros((B, 1, 30)); dv[:, 0, 0] = np.linspace(-0.1, 0.1, B)

    def others(c):
        c.set_zcom(zc)
        c.set_model(raw)
        c.gen_walk_batch(1.0, specs)
        c.set_pushes(ticks, dv)

    def roll(c):
        st = c.new_state(q0, v * 0.3, t=0.0)
        out, status, log = c.rollout(st, 24, log=True)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (out[:, :78], st, status, log)]

    a = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    a.set_params(**fields)
    others(a)
    b = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    others(b)
    b.set_params(**fields)
    ra, rb = roll(a), roll(b)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    assert a.params_per_instance() and a.plans_per_instance and a.pushes_per_instance
    c = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)      # and the parameters are still in force behind them
    others(c)
    assert not np.array_equal(roll(c)[1], ra[1])
    for h in (a, b, c):
        h.close()


def test_one_robot_handle_reports_shared(cfg2):
    """On a handle of one robot a per-robot set is the shared set: the mode reports 0, the values are in force."""
    over = SIX_SETS[3]
    v, vprev = states(1, 321)
    ctl = make_controller(1, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    ctl.set_params(**over)
    assert not ctl.params_per_instance()
    assert {k: ctl.get_params(0)[k] for k in over} == over
    res = run(ctl, cfg2["q0"], v, vprev, phases=(0,), ticks=5)
    ctl.close()
    ctl = make_controller(1, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1, **over)
    shared = run(ctl, cfg2["q0"], v, vprev, phases=(0,), ticks=5)
    ctl.close()
    assert_robot_equal(res, shared, 0, over)
