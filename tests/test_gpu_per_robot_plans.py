"""Per-robot gait and jump schedules (lmh_gen_walk_batch / lmh_gen_jump_batch / lmh_set_plans): the batched generators against the host
statement, a per-robot handle with equal specs against the shared handle, robot i of a mixed batch against robot i alone, closed-loop /
plain / debug evaluation against the CPU oracle on each robot's own plan, the upload path, argument checks, the way back to one
shared plan and a refused lmh_set_segments, which releases nothing.  The draw (ranges, seed 20261016, order) is tests/plan_draw.py.  Rules as in the other GPU files: the HIP path through the
C ABI against the oracle, 1e-6 relative on tau / f (helpers.close), bit-exact k; "the same computation" means bit-identical."""
import os
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import pytest
import torch

import helpers
from helpers import TOL_REL, WEIGHT, bits_differ, close, horizon_controller, perturbed_velocities, run_probe, vec_err
from plan_draw import DT, MPC_DT, N_PREVIEW, SIM_TIME, draw_jump_specs, draw_walk_specs, spec_i

pytestmark = pytest.mark.gpu
KP_FEET = 500.0                                   # controller.hpp:108

# the four parameter sets of test_gpu_round2.test_walk_generator_kernel_matches_the_host_plan (without their simulation_time: the sample
# grid of a batch is shared)
ROUND2_GAITS = [
    dict(num_steps=4, time_per_step=0.5, ds_time=0.1, step_height=0.02, settle_time=0.3, first_support=1, foot_y=0.05),
    dict(num_steps=2, time_per_step=0.2, ds_time=0.05, step_height=0.02, settle_time=0.1, first_support=1, foot_y=0.05),
    dict(num_steps=7, time_per_step=0.17, ds_time=0.033, step_height=0.015, settle_time=0.0731, first_support=2, foot_y=0.045),
    dict(num_steps=5, time_per_step=0.2, ds_time=0.05, step_height=0.02, settle_time=0.1, first_support=1, foot_y=0.05),
]


make_controller = partial(horizon_controller, N=N_PREVIEW, zcom=0.26, mpc_dt=MPC_DT, dt=DT)
make_oracle = partial(helpers.make_oracle, mpc_dt=MPC_DT)


@pytest.fixture(scope="module")
def nao():
    o = make_oracle(N_PREVIEW, 1.0)
    K = o.gain_row()
    Px, _ = o.mpc_mats()
    return dict(zcom=o.zcom, q0=o.robot()["q"].copy(), kpx=K @ Px)


def stack_specs(*parts):
    return {k: np.concatenate([np.atleast_1d(p[k]) for p in parts]) for k in parts[0]}


def gaits_as_specs(gaits):
    return {k: np.array([g[k] for g in gaits]) for k in gaits[0]}


def run(ctl, st, nt, log=True):
    out, status, lg = ctl.rollout(st, nt, log=log)
    torch.cuda.synchronize()
    return dict(state=st.cpu().numpy().copy(), out=out.cpu().numpy().copy(), status=status.cpu().numpy().copy(),
                log=None if lg is None else lg.cpu().numpy().copy())


def same_bits(a, b, rows=None, rows_b=None):
    """state, out, status and log rows of two results bit for bit; rows / rows_b select the robots of a / b."""
    return not bits_differ(a, b, rows, rows_b)


def parallel(fn, items, workers=8):
    with ThreadPoolExecutor(max_workers=workers) as ex:               # the oracle's C calls release the interpreter lock
        return list(ex.map(fn, items))


def check_walk_plan(g, p, spec, time_step, used):
    """The criteria of test_walk_generator_kernel_matches_the_host_plan for one robot: g read back from the device (n_seg records, `used`
    of them the robot's own), p = trajectories.walk_plan."""
    assert np.array_equal(g["phase"], p["phase"]) and np.array_equal(g["seg_of_sample"], p["seg_of_sample"])
    assert np.array_equal(g["zmp_x"], p["zmp_x"]) and np.array_equal(g["zmp_y"], p["zmp_y"])
    assert p["segs"].shape[0] == used and g["segs"].shape[0] >= used
    assert not g["segs"][used:].any()                                 # padding records zero
    assert np.array_equal(g["segs"][:used, 0], p["segs"][:, 0])
    for sgd, sgh in zip(g["segs"][:used], p["segs"]):
        T = max(spec["time_per_step"] - spec["ds_time"], time_step)
        t = np.linspace(0.0, T, 41)
        for ft in range(2):
            for ax in range(3):
                cd, ch = sgd[1 + 24 * ft + 8 * ax: 9 + 24 * ft + 8 * ax], sgh[1 + 24 * ft + 8 * ax: 9 + 24 * ft + 8 * ax]
                if not np.abs(ch[1:]).max() > 1e-9:                # a standing foot: constants, exactly
                    assert cd[0] == ch[0] and np.abs(cd[1:]).max() == 0.0
                    continue
                for der in range(3):
                    pd = np.polynomial.polynomial.Polynomial(cd).deriv(der)(t) if der else np.polynomial.polynomial.polyval(t, cd)
                    phh = np.polynomial.polynomial.Polynomial(ch).deriv(der)(t) if der else np.polynomial.polynomial.polyval(t, ch)
                    assert close(pd, phh, 1e-12), (ft, ax, der)
                assert np.abs(cd - ch).max() < 1e-11 * np.abs(ch).max()


# ------------------------------------------------------------------------------- 3. batched generators against the host statement
@pytest.mark.parametrize("grid", ["draw", "cut"])
def test_batched_walk_generator_matches_the_host_plans(grid):
    """64 robots through get_plan(i) against trajectories.walk_plan, criteria of the single-plan test (samples, phase, seg_of_sample
    bit-exact, start times and standing feet exact, swing polynomials to 1e-12 in position / velocity / acceleration), padding zero.
    "draw": 60 robots of the draw plus the four parameter sets of the single-plan test on the draw's grid (2.6 s at 10 ms), where every
    gait ends inside the grid.  "cut": the single-plan test's own short grid (0.56 s at 1 ms, 1060 samples), where the five-step set's
    last swing is cut by the end of the grid; the grid is shared, and a gait whose swing would START beyond it has no host statement
    (walk_plan's polynomial fit is singular for a zero-length swing), so this batch holds the two sets that fit -- the five-step one
    (cut) and the two-step one -- each 32 times with settle_time moved earlier by 1 ms per robot; robots 0 and 1 are the sets themselves."""
    from linearmpchumanoid_amd import trajectories
    B = 64
    if grid == "draw":
        sim, mpc_dt = SIM_TIME, MPC_DT
        sp = stack_specs(draw_walk_specs(B - 4)[0], gaits_as_specs(ROUND2_GAITS))
    else:
        sim, mpc_dt = 0.56, 1e-3
        gaits = []
        for i in range(B):
            g = dict(ROUND2_GAITS[3 if i % 2 == 0 else 1])
            g["settle_time"] -= 0.001 * (i // 2)                       # earlier, so the cut swing only gets longer than the set's own
            gaits.append(g)
        sp = gaits_as_specs(gaits)
    ctl = make_controller(B, dt=1e-3, mpc_dt=mpc_dt)
    assert not ctl.plans_per_instance
    ctl.gen_walk_batch(sim, sp)
    assert ctl.plans_per_instance
    n_seg = 2 * int(sp["num_steps"].max()) + 2
    assert ctl.get_refs()["segs"].shape[0] == n_seg                 # lmh_num_segments: the common stride
    if grid == "cut":                                               # the property this grid is for
        p0 = trajectories.walk_plan(sim, mpc_dt, **spec_i(sp, 0))
        last_swing = int(p0["seg_of_sample"][-1])
        assert last_swing == 2 * 5 and p0["phase"][-1] != 0          # the grid ends inside the fifth swing
    for i in range(B):
        s = spec_i(sp, i)
        check_walk_plan(ctl.get_plan(i), trajectories.walk_plan(sim, mpc_dt, **s), s, mpc_dt, 2 * s["num_steps"] + 2)
    g0 = ctl.get_refs()                                             # lmh_get_refs on a per-robot handle: robot 0
    assert all(np.array_equal(g0[k], ctl.get_plan(0)[k]) for k in g0)
    ctl.close()


def test_batched_jump_generator_matches_the_host_plans():
    from linearmpchumanoid_amd import trajectories
    B = 64
    sp = draw_jump_specs(B)
    ctl = make_controller(B, N=48)
    ctl.gen_jump_batch(1.2, sp)
    assert ctl.plans_per_instance
    host = trajectories.jump_plans(1.2, MPC_DT, sp)
    for i in range(B):
        g = ctl.get_plan(i)
        assert len(g["segs"]) == 0
        for k in ("zmp_x", "zmp_y", "phase"):
            assert np.array_equal(g[k], host[k][i]), (i, k)
    ctl.close()


# ------------------------------------------------------------------------------- 4. B equal specs = the shared handle
def test_equal_specs_per_robot_is_the_shared_handle(nao):
    """gen_walk_batch with one spec repeated against gen_walk with that spec: 300 robots with distinct step lengths and small distinct
    initial velocities, 620 ticks (two chunk boundaries), log on: state, out, status and log bit-identical."""
    B, nt = 300, 620
    spec = dict(num_steps=3, time_per_step=0.45, ds_time=0.12, step_height=0.02, settle_time=0.1, first_support=2, foot_y=0.05)
    xs = np.linspace(0.02, 0.05, B)
    v = perturbed_velocities(B, seed=4100) * 0.1
    res = []
    for per_robot in (False, True):
        ctl = make_controller(B, zcom=nao["zcom"], warm_start=1)
        if per_robot:
            ctl.gen_walk_batch(SIM_TIME, spec)
        else:
            ctl.gen_walk(SIM_TIME, **spec)
        assert ctl.plans_per_instance == per_robot
        ctl.set_xscale(xs)
        res.append(run(ctl, ctl.new_state(nao["q0"], v, t=0.0), nt))
        ctl.close()
    assert np.isfinite(res[0]["log"]).all()
    assert same_bits(res[0], res[1])


# ------------------------------------------------------------------------------- 5. robot i of a mixed batch = robot i alone
MIXED_B = 256
MIXED_PICK = (0, 37, 74, 110, 147, 183, 220, 255)                   # first, last and six in between


def test_robot_of_a_mixed_batch_is_that_robot_alone(nao):
    """256 robots on the draw, 1000 ticks, log on.  For eight robots spread over the batch a B = 1 handle given that robot's plan through
    lmh_set_refs + lmh_set_segments (+ its step length) reproduces its state, out, status and log rows bit for bit: which workgroup runs
    a robot, and which robot that workgroup ran before, has no influence (a wrong stride or a stale reference cache would)."""
    B, nt = MIXED_B, 1000
    sp, xs = draw_walk_specs(B)
    ctl = make_controller(B, zcom=nao["zcom"], warm_start=1)
    ctl.gen_walk_batch(SIM_TIME, sp)
    ctl.set_xscale(xs)
    batch = run(ctl, ctl.new_state(nao["q0"], np.zeros(30), t=0.0), nt)
    assert np.isfinite(batch["log"]).all()
    for i in MIXED_PICK:
        plan = ctl.get_plan(i)
        one = make_controller(1, zcom=nao["zcom"], warm_start=1)
        one.set_refs(plan["zmp_x"], plan["zmp_y"], plan["phase"])
        one.set_segments(plan["segs"], plan["seg_of_sample"])
        one.set_xscale(xs[i:i + 1])
        assert not one.plans_per_instance
        alone = run(one, one.new_state(nao["q0"], np.zeros(30), t=0.0), nt)
        one.close()
        assert same_bits(batch, alone, rows=slice(i, i + 1), rows_b=slice(0, 1)), i
    ctl.close()


# ------------------------------------------------------------------------------- 6 / 7. oracle parity on each robot's own plan
ORC_B, ORC_NT, ORC_MID = 16, 1500, 700
_closed_loop = {}


def closed_loop(nao):
    """16 robots of the draw, 1500 ticks in launches of 700 + 800 (lmh_rollout(a + b) is lmh_rollout(a) then lmh_rollout(b)), the state
    at tick 700 kept for the single-evaluation test.  Cached per module."""
    if _closed_loop:
        return _closed_loop
    sp, xs = draw_walk_specs(ORC_B)
    ctl = make_controller(ORC_B, zcom=nao["zcom"], warm_start=1)
    ctl.gen_walk_batch(SIM_TIME, sp)
    ctl.set_xscale(xs)
    st = ctl.new_state(nao["q0"], np.zeros(30), t=0.0)
    a = run(ctl, st, ORC_MID)
    b = run(ctl, st, ORC_NT - ORC_MID)
    plans = [ctl.get_plan(i) for i in range(ORC_B)]
    _closed_loop.update(sp=sp, xs=xs, ctl=ctl, mid=a, end=b, log=np.concatenate([a["log"], b["log"]], axis=0), plans=plans,
                        flags=a["status"][:, 2] | b["status"][:, 2])
    return _closed_loop


def plan_oracle(plan, xscale, N=N_PREVIEW, sim=SIM_TIME):
    o = make_oracle(N, sim)
    o.set_refs(plan["zmp_x"], plan["zmp_y"], plan["phase"])
    if len(plan["segs"]):
        o.set_segments(plan["segs"], plan["seg_of_sample"], xscale=float(xscale))
    return o


def test_closed_loop_oracle_parity_on_per_robot_plans(nao):
    """Each robot against an oracle fed the plan read back with get_plan(i): k of the last tick exact, no status flag on any robot,
    tau and f / weight of every ninth tick within helpers.close's default (1e-6 relative).  The batch is really desynchronised: at tick
    700 the sixteen phase[k] values include double support and both single supports."""
    S = closed_loop(nao)
    assert (S["flags"] == 0).all(), S["flags"]
    q0 = np.concatenate([nao["q0"], np.zeros(30)])

    def one(i):
        return plan_oracle(S["plans"][i], S["xs"][i]).rollout(q0, 0.0, ORC_NT, dt=DT, log=True)

    refs = parallel(one, range(ORC_B))
    worst = 0.0
    for i, r in enumerate(refs):
        assert S["end"]["status"][i, 0] == r["k"][-1], i
        assert S["mid"]["status"][i, 0] == r["k"][ORC_MID - 1], i
        for tk in list(range(0, ORC_NT, 9)) + [ORC_NT - 1]:
            ref = r["log"][tk]
            worst = max(worst, vec_err(S["log"][tk, i, :24], ref[:24]))
            assert close(S["log"][tk, i, :24], ref[:24], TOL_REL), (i, tk, vec_err(S["log"][tk, i, :24], ref[:24]))
            assert close(S["log"][tk, i, 24:], ref[24:], TOL_REL, scale=WEIGHT), (i, tk, vec_err(S["log"][tk, i, 24:], ref[24:]))
    print("\nper-robot plans, closed loop: worst tau error %.2e" % worst)
    k700 = int(refs[0]["k"][ORC_MID])
    assert k700 == 70
    assert {int(S["plans"][i]["phase"][k700]) for i in range(ORC_B)} == {0, 1, 2}


def test_plain_and_debug_evaluation_on_per_robot_plans(nao):
    """The same sixteen robots, states of the rollout at tick 700: lmh_eval and lmh_eval_debug (one evaluation each, from identical
    copies of the state) against Oracle.eval with the robot's plan and v_prev: k exact, the debug record's footAccRef / u0 at the
    tolerances and scale rules of test_gpu_posture_sweep.py (1e-10 / 1e-11), tau / f / qdd at 1e-6."""
    from linearmpchumanoid_amd.controller import unpack_debug
    S = closed_loop(nao)
    ctl, state = S["ctl"], S["mid"]["state"]
    assert ctl.plans_per_instance
    s1, s2 = torch.as_tensor(state.copy()).to(ctl.device), torch.as_tensor(state.copy()).to(ctl.device)
    out, status = ctl.stand_step(s1)
    outd, statusd, dbg = ctl.stand_step(s2, debug=True)
    torch.cuda.synchronize()
    out, status, outd, statusd, dbg = (a.cpu().numpy() for a in (out, status, outd, statusd, dbg))
    phases = set()
    for i in range(ORC_B):
        o = plan_oracle(S["plans"][i], S["xs"][i])
        o.set_prev_velocity(state[i, 60:90])
        e = o.eval(state[i, 0:30], state[i, 30:60], float(state[i, 90]))
        qp, t, rb = o.qp(), o.terms(), o.robot()
        phases.add(e["phase"])
        for res, stt in ((out, status), (outd, statusd)):
            assert stt[i, 0] == e["k"] == 70 and stt[i, 2] == 0, (i, stt[i])
            assert close(res[i, :24], e["tau"]), (i, vec_err(res[i, :24], e["tau"]))
            assert close(res[i, 24:36], e["f"], scale=WEIGHT), (i, vec_err(res[i, 24:36], e["f"]))
            assert close(res[i, 36:66], e["qpp"]), (i, vec_err(res[i, 36:66], e["qpp"]))
        d = unpack_debug(dbg[i])
        psole = max(np.abs(t["T"][7][:3, 3]).max(), np.abs(t["T"][14][:3, 3]).max())
        fs = KP_FEET * (0.05 + psole) + np.abs(qp["footAccRef"]).max()
        assert np.abs(d["footAccRef"] - qp["footAccRef"]).max() / fs < 1e-10, i
        us = (9.81 / 0.26 * 0.05 + abs(nao["kpx"][0]) * np.abs(rb["CoM"][:2]).max() + abs(nao["kpx"][1]) * np.abs(rb["comVel"][:2]).max()
              + np.abs(qp["u0"]).max())
        assert np.abs(d["mpc"][:2] - qp["u0"]).max() / us < 1e-11, i
    assert phases == {0, 1, 2}


# ------------------------------------------------------------------------------- 8. jumping
def test_per_robot_jump_schedules_against_the_oracle(nao):
    """gen_jump_batch, 12 robots (stance_time U(0.3, 0.5), flight_time U(0.08, 0.16), seed 20261017), N = 48 x 10 ms, dt = 1e-3, 1000
    ticks: contact forces exactly zero on every tick whose phase[k] is flight FOR THAT ROBOT, tau / f against the oracle at 1e-6 on every
    ninth tick, no status flag."""
    B, N, nt, sim = 12, 48, 1000, 1.2
    sp = draw_jump_specs(B)
    ctl = make_controller(B, N=N, zcom=nao["zcom"], warm_start=1)
    ctl.gen_jump_batch(sim, sp)
    res = run(ctl, ctl.new_state(nao["q0"], np.zeros(30), t=0.0), nt)
    plans = [ctl.get_plan(i) for i in range(B)]
    ctl.close()
    q0 = np.concatenate([nao["q0"], np.zeros(30)])

    def one(i):
        o = plan_oracle(plans[i], 1.0, N=N, sim=sim)
        o.set_zcom(nao["zcom"])
        return o.rollout(q0, 0.0, nt, dt=DT, log=True)

    refs = parallel(one, range(B))
    takeoff = set()
    for i, r in enumerate(refs):
        ph = plans[i]["phase"][np.asarray(r["k"])]                    # phase of the k4-stage evaluation of every tick
        fl = ph == 3
        assert fl.any() and not fl.all()
        takeoff.add(int(np.argmax(fl)))
        assert not res["log"][fl, i, 24:].any(), i                  # exactly zero in this robot's flight
        assert np.abs(res["log"][~fl, i, 24:]).max(axis=1).min() > 0.0
        assert res["status"][i, 0] == r["k"][-1]
        for tk in list(range(0, nt, 9)) + [nt - 1]:
            ref = r["log"][tk]
            assert close(res["log"][tk, i, :24], ref[:24], TOL_REL), (i, tk, vec_err(res["log"][tk, i, :24], ref[:24]))
            assert close(res["log"][tk, i, 24:], ref[24:], TOL_REL, scale=WEIGHT), (i, tk, vec_err(res["log"][tk, i, 24:], ref[24:]))
    assert len(takeoff) >= 6                                        # the robots leave the ground in different ticks
    assert (res["status"][:, 2] == 0).all(), res["status"][:, 2]


# ------------------------------------------------------------------------------- 9. upload path and validation
def test_uploaded_plans_and_argument_checks(nao):
    """set_plans(walk_plans(...)) then get_plan(i) round-trips exactly.  A rollout on uploaded plans against one on generated plans: the
    generated plans read back and uploaded again are the same bits, so every robot is bit-identical; with the HOST plans uploaded, a robot
    whose host plan equals the generated one bit for bit is bit-identical and the others (swing coefficients from the host's linear solve
    instead of the device's closed form, equal to 1e-11) agree in tau / f to 1e-9 on every logged tick -- the count of each is printed.
    Bad arguments (n != B, a segment index beyond n_seg in robot 5 only, an invalid spec in robot 7 only) are LMH_ERR_BAD_ARG naming the
    robot, and the handle still runs its previous plans with unchanged results."""
    import ctypes as C
    from linearmpchumanoid_amd import capi, trajectories
    from linearmpchumanoid_amd.capi import LmhError
    B, nt = 48, 400
    sp, xs = draw_walk_specs(B)
    host = trajectories.walk_plans(SIM_TIME, MPC_DT, sp)
    gen = make_controller(B, zcom=nao["zcom"], warm_start=1)
    gen.gen_walk_batch(SIM_TIME, sp)
    gen.set_xscale(xs)
    ref = run(gen, gen.new_state(nao["q0"], np.zeros(30), t=0.0), nt)
    gplans = [gen.get_plan(i) for i in range(B)]

    up = make_controller(B, zcom=nao["zcom"], warm_start=1)
    up.set_xscale(xs)
    up.set_plans(**host)
    assert up.plans_per_instance
    for i in range(B):
        g = up.get_plan(i)
        assert all(np.array_equal(g[k], host[k][i]) for k in g), i
    on_host = run(up, up.new_state(nao["q0"], np.zeros(30), t=0.0), nt)
    exact = [i for i in range(B) if all(np.array_equal(gplans[i][k], host[k][i]) for k in host)]
    print("\nuploaded host plans: %d of %d robots have bit-identical plans" % (len(exact), B))
    for i in range(B):
        if i in exact:
            assert same_bits(ref, on_host, rows=slice(i, i + 1)), i
        else:
            for tk in range(nt):
                assert close(on_host["log"][tk, i, :24], ref["log"][tk, i, :24], 1e-9), (i, tk)
                assert close(on_host["log"][tk, i, 24:], ref["log"][tk, i, 24:], 1e-9, scale=WEIGHT), (i, tk)
    up.set_plans(**{k: np.stack([p[k] for p in gplans]) for k in host})
    assert same_bits(ref, run(up, up.new_state(nao["q0"], np.zeros(30), t=0.0), nt))
    up.close()

    # ---- bad arguments leave the handle on its previous plans
    def refused(fn, needle):
        with pytest.raises(LmhError) as ei:
            fn()
        assert ei.value.code == -2 and needle in str(ei.value), str(ei.value)
        assert gen.plans_per_instance
        assert all(np.array_equal(gen.get_plan(5)[k], gplans[5][k]) for k in gplans[5])

    refused(lambda: gen.set_plans(**{k: v[:B - 1] for k, v in host.items()}), "n_instances")
    arr = (capi.LmhWalkSpec * (B + 1))()
    assert capi.lib().lmh_gen_walk_batch(gen._h, SIM_TIME, arr, B + 1) == -2
    bad = {k: v.copy() for k, v in host.items()}
    bad["seg_of_sample"][5, 17] = host["segs"].shape[1]
    refused(lambda: gen.set_plans(**bad), "robot 5")
    bad_sp = {k: v.copy() for k, v in sp.items()}
    bad_sp["ds_time"][7] = bad_sp["time_per_step"][7]               # needs ds_time < time_per_step
    refused(lambda: gen.gen_walk_batch(SIM_TIME, bad_sp), "robot 7")
    jsp = dict(stance_time=np.full(B, 0.4), flight_time=np.full(B, 0.1))
    jsp["flight_time"][7] = -0.1
    refused(lambda: gen.gen_jump_batch(SIM_TIME, jsp), "robot 7")
    with pytest.raises(LmhError):
        gen.get_plan(B)
    assert same_bits(ref, run(gen, gen.new_state(nao["q0"], np.zeros(30), t=0.0), nt))
    gen.close()


# ------------------------------------------------------------------------------- 10. going back to one shared plan
def test_shared_plan_after_per_robot_plans_is_a_fresh_handle(nao):
    B, nt = 96, 300
    sp, xs = draw_walk_specs(B)
    spec = dict(num_steps=2, time_per_step=0.4, ds_time=0.1, step_height=0.02, settle_time=0.1)
    v = perturbed_velocities(B, seed=4200) * 0.1
    ctl = make_controller(B, zcom=nao["zcom"], warm_start=1)
    ctl.set_xscale(xs)
    ctl.gen_walk_batch(SIM_TIME, sp)
    run(ctl, ctl.new_state(nao["q0"], v, t=0.0), nt)
    ctl.gen_walk(2.0, **spec)                                       # fewer samples and segments than the per-robot set had
    assert not ctl.plans_per_instance
    back = run(ctl, ctl.new_state(nao["q0"], v, t=0.0), nt)
    shared = ctl.get_refs()
    assert all(np.array_equal(ctl.get_plan(B - 1)[k], shared[k]) for k in shared)     # get_plan on a shared handle: the shared plan
    # the other setters end per-robot plans as well
    ctl.gen_walk_batch(SIM_TIME, sp)
    ctl.set_refs_stance(1.0, 2)
    assert not ctl.plans_per_instance
    ctl.gen_jump_batch(1.0, dict(stance_time=np.linspace(0.3, 0.5, B), flight_time=0.1))
    assert ctl.plans_per_instance
    ctl.gen_jump(1.0, 0.4, 0.1)
    assert not ctl.plans_per_instance
    ctl.gen_walk_batch(SIM_TIME, sp)
    p0 = ctl.get_plan(0)
    ctl.set_segments(p0["segs"], p0["seg_of_sample"])               # robot 0's samples stay as the shared ones
    assert not ctl.plans_per_instance
    assert all(np.array_equal(ctl.get_plan(B - 1)[k], p0[k]) for k in p0)
    ctl.close()
    fresh = make_controller(B, zcom=nao["zcom"], warm_start=1)
    fresh.set_xscale(xs)
    fresh.gen_walk(2.0, **spec)
    assert same_bits(back, run(fresh, fresh.new_state(nao["q0"], v, t=0.0), nt))
    fresh.close()


# ------------------------------------------------------------------------------- 10b. a refused lmh_set_segments releases nothing
def test_refused_set_segments_leaves_the_handle_on_its_plan(nao):
    """set_segments with a seg_of_sample entry >= n_seg, and with a wrong n_samples, is LMH_ERR_BAD_ARG.  On a handle carrying a
    generated walking plan, after each refusal num_segments and get_refs() return exactly what they returned before, and a rollout into
    the first swing is bit-identical to the one of an untouched twin handle.  On a handle with per-robot plans the same refusals leave
    plans_per_instance true and every robot's get_plan unchanged."""
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.capi import LmhError
    B, nt = 8, 400
    spec = dict(num_steps=3, time_per_step=0.45, ds_time=0.12, step_height=0.02, settle_time=0.1, first_support=2, foot_y=0.05)
    xs = np.linspace(0.02, 0.05, B)

    def walker():
        c = make_controller(B, zcom=nao["zcom"], warm_start=1)
        c.gen_walk(SIM_TIME, **spec)
        c.set_xscale(xs)
        return c

    def refusals(plan):
        """The two refused calls on a handle whose (robot 0's) plan is `plan`."""
        beyond = plan["seg_of_sample"].copy()
        beyond[17] = len(plan["segs"])
        return (lambda c: c.set_segments(plan["segs"], beyond)), (lambda c: c.set_segments(plan["segs"], plan["seg_of_sample"][:-1]))

    def refused(fn, c):
        with pytest.raises(LmhError) as ei:
            fn(c)
        assert ei.value.code == -2, str(ei.value)

    ctl, twin = walker(), walker()
    before = ctl.get_refs()
    n_seg = capi.lib().lmh_num_segments(ctl._h)
    assert n_seg == 2 * spec["num_steps"] + 2 == len(before["segs"])
    assert before["phase"][int(nt * DT / MPC_DT) - 1] != 0             # the rollout reaches a swing: its foot references are the segments'
    want = run(twin, twin.new_state(nao["q0"], np.zeros(30), t=0.0), nt)
    twin.close()
    assert np.isfinite(want["log"]).all()
    for fn in refusals(before):
        refused(fn, ctl)
        assert capi.lib().lmh_num_segments(ctl._h) == n_seg
        after = ctl.get_refs()
        assert all(np.array_equal(after[k], before[k]) for k in before)
        assert same_bits(want, run(ctl, ctl.new_state(nao["q0"], np.zeros(30), t=0.0), nt))
    ctl.close()

    sp, _ = draw_walk_specs(B)
    per = make_controller(B, zcom=nao["zcom"], warm_start=1)
    per.gen_walk_batch(SIM_TIME, sp)
    plans = [per.get_plan(i) for i in range(B)]
    for fn in refusals(plans[0]):
        refused(fn, per)
        assert per.plans_per_instance
        for i in range(B):
            g = per.get_plan(i)
            assert all(np.array_equal(g[k], plans[i][k]) for k in g), i
    per.close()


# ------------------------------------------------------------------------------- 11. no result depends on LDS nobody wrote
_POISON_PROBE = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd.controller import BatchedController, default_config
from plan_draw import SIM_TIME, draw_walk_specs
ik = json.load(open("tests/golden/ik_posture.json"))
B = 256
sp, xs = draw_walk_specs(B)
ctl = BatchedController(B, default_config(dt=1e-3, time_horizon=0.32 + 1e-9, z_com=ik["z_com"], mpc_dt=1e-2, warm_start=1))
ctl.gen_walk_batch(SIM_TIME, sp)
ctl.set_xscale(xs)
st = ctl.new_state(np.array(ik["q"]), np.zeros(30), t=0.0)
out, status, log = ctl.rollout(st, 300, log=True)
o2, s2 = ctl.stand_step(st.clone())
torch.cuda.synchronize()
h = hashlib.sha256()
for a in (out, status, log, st, o2, s2):
    h.update(a.cpu().numpy().tobytes())
print(json.dumps({"sha": h.hexdigest(), "finite": bool(torch.isfinite(log).all().item()), "per_robot": ctl.plans_per_instance,
                  "build_flags": capi.lib().lmh_debug_build_flags()}))
"""


def test_per_robot_plans_do_not_depend_on_uninitialised_lds():
    """The mixed batch of 256 robots for 300 ticks (and one plain evaluation) on the checker build with NaN-filled LDS (-DLMH_POISON,
    lmh_debug_build_flags bit 0), each build in a fresh child process: bit-identical to the shipped build."""
    from linearmpchumanoid_amd import build as hipbuild
    so = hipbuild.build_variant("poison", ["-DLMH_POISON"])
    assert os.path.exists(so)
    res = {}
    for variant in ("", "poison"):
        res[variant] = run_probe(_POISON_PROBE, variant, timeout=600)
    assert res[""]["build_flags"] & 1 == 0 and res["poison"]["build_flags"] & 1 == 1, res
    assert res[""]["per_robot"] and res["poison"]["per_robot"] and res[""]["finite"] and res["poison"]["finite"], res
    assert res[""]["sha"] == res["poison"]["sha"], res
