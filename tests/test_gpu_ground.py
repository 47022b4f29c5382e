"""Per-robot ground planes (lmh_set_ground) on the GPU: the plant calls and the zero-order-hold family against a plane under each foot.

Inputs: ground_cases.tilted_states(), the 16 states of plant_step_cases.contact_states() with planes tilted 2 .. 6 degrees that put every
contact regime on both feet with margin (asserted on the CPU in test_ground.py).  References: the numpy statement
trajectories.ground_contact on the oracle's vertex kinematics for the forces, ground_cases.ground_plant_xdot (plant_step_cases' helper with
the statement's wrench) for the derivative and the step, the calls without a table for the flat record and the ledge, and
zoh_host_loop.host_loop -- made of stand_step and plant_step on a handle with the same table -- for the closed loop, bit for bit.
Tolerances are test_gpu_plant_step.py's: 1e-11 on the force scale of the ingredients, the forward-dynamics criterion at 1e-12, 1e-7 `close`
behind 20 substeps.  Every case runs at most 16 robots and 20 substeps."""
import ctypes as C

import numpy as np
import pytest
import torch

import ground_cases as gc
import plant_step_cases as pc
import zoh_ex_cases as zx
import zoh_io_cases as zi
from helpers import check_record_table, close, close_on, make_controller, rel_err, same_bits as _same, to_device
from zoh_host_loop import assert_same as _assert_same, fresh, host_loop

pytestmark = pytest.mark.gpu
DT, TH, B = pc.DT, pc.TH, pc.B
G = pc.GROUND


def _ctl(S, n=B, planes=None, **cfg):
    ctl = make_controller(n, DT, TH, S["zcom"], **cfg)
    if planes is not None:
        ctl.set_ground(planes)
    return ctl


def _scale(pos, vel):
    """test_gpu_plant_step._check_contact's force scale: k max|x_vertex| + (c + c_t) max|xdot_vertex|."""
    return G["k"] * np.abs(pos).max() + (G["d"] + G["dt"]) * np.abs(vel).max()


def _ninf(a):
    return float(np.abs(a).sum(axis=1).max()) if np.ndim(a) == 2 else float(np.abs(a).max())


def _split(c):
    from linearmpchumanoid_amd.controller import BatchedController
    return BatchedController.split_contact(c)


# ------------------------------------------------------------------------------- 1. contact against the statement
def test_contact_wrench_is_the_statement():
    S = gc.tilted_states()
    ctl = _ctl(S, planes=S["planes"])
    assert ctl.ground_per_instance and all(_same(ctl.get_ground(i), S["planes"][i]) for i in range(B))
    c = ctl.contact_wrench(to_device(ctl, S["q"]), to_device(ctl, S["v"])).cpu().numpy()
    worst = 0.0
    for i in range(B):
        s, scale = _split(c[i]), _scale(S["pos"][i], S["vel"][i])
        pen = gc.thresholds(S["pos"][i], S["vel"][i], S["planes"][i])[0]
        vf, w = S["force"][i], S["w"][i].reshape(2, 2, 3)
        print("robot %2d: vertex forces %.2e, wrench %.2e of the scale %.0f N" % (i, np.abs(s["vertex_force"] - vf).max() / scale, np.abs(s["w"] - S["w"][i]).max() / scale, scale))
        assert not s["vertex_force"][~(pen > 0.0)].any(), i                         # exactly 0 out of the ground
        assert np.array_equal(s["vertex_force"] == 0.0, vf == 0.0), i               # and the statement's clamps
        assert close_on(s["vertex_force"], vf, 1e-11, scale), (i, np.abs(s["vertex_force"] - vf).max() / scale)
        got = s["w"].reshape(2, 2, 3)
        assert close_on(got[:, 1], w[:, 1], 1e-11, 4 * scale) and close_on(got[:, 0], w[:, 0], 1e-11, 4 * scale * 0.11), i
        assert not s["pad"].any()
        worst = max(worst, float(np.abs(s["vertex_force"] - vf).max() / scale))
    print("contact against the statement: worst %.2e of the force scale" % worst)
    ctl.close()


# ------------------------------------------------------------------------------- 2. flat
def test_the_flat_record_is_the_model_without_a_table():
    """contact_wrench and plant_derivative with the flat record against the calls without a table: 1e-13 of the scale, the same zero
    pattern.  The contact forces on test_gpu_plant_step's force scale; qdot does not see the contact (the same bytes); the accelerations
    on the forward-dynamics scale cond(M) max|a| of that test, since a force that moves by ulps moves M^-1 J'w by cond(M) times as much
    at the most."""
    S = gc.tilted_states()
    flat, none = _ctl(S, planes=gc.FLAT), _ctl(S)
    assert not flat.ground_per_instance and _same(flat.get_ground(B - 1), gc.FLAT) and _same(none.get_ground(0), gc.FLAT)
    q, v, tau = (to_device(flat, S[k]) for k in ("q", "v", "tau"))
    ca, cb = flat.contact_wrench(q, v).cpu().numpy(), none.contact_wrench(q, v).cpu().numpy()
    xa, da, fa = flat.plant_derivative(q, v, tau)
    xb, db, fb = none.plant_derivative(q, v, tau)
    assert _same(da.cpu().numpy(), ca) and _same(db.cpu().numpy(), cb) and int(fa.abs().max()) == 0 and int(fb.abs().max()) == 0
    xa, xb = xa.cpu().numpy(), xb.cpu().numpy()
    o = pc.make_oracle()
    for i in range(B):
        scale = _scale(S["pos"][i], S["vel"][i])
        assert np.array_equal(ca[i] == 0.0, cb[i] == 0.0), i
        assert close_on(ca[i, 12:36], cb[i, 12:36], 1e-13, scale) and close_on(ca[i, 0:12], cb[i, 0:12], 1e-13, 4 * scale), (i, np.abs(ca[i] - cb[i]).max() / scale)
        assert _same(xa[i, :30], xb[i, :30]), i
        o.set_prev_velocity(S["v"][i]); o.eval(S["q"][i], S["v"][i], 0.0)
        cond = np.linalg.cond(o.terms()["M"])
        err = np.abs(xa[i, 30:] - xb[i, 30:]).max() / (cond * np.abs(xb[i, 30:]).max())
        print("robot %2d: contact %.2e of the force scale, acceleration %.2e of cond(M) max|a|" % (i, np.abs(ca[i] - cb[i]).max() / scale, err))
        assert err <= 1e-13, (i, err)
    flat.close(); none.close()


def _every_call(ctl, S, zoh):
    """The bytes of every plant and zero-order-hold call from the same inputs."""
    q, v, tau = (to_device(ctl, S[k]) for k in ("q", "v", "tau"))
    res = [("contact", ctl.contact_wrench(q, v))]
    xdot, c, f = ctl.plant_derivative(q, v, tau)
    res += [("xdot", xdot), ("xdot contact", c), ("xdot flags", f)]
    st, f = ctl.plant_step(fresh(ctl, S["q"], S["v"]), tau, 3)
    res += [("step", st), ("step flags", f)]
    st = fresh(ctl, S["q"], S["v"])
    out, status, log = ctl.rollout_zoh(st, 2, 2, base_wrench=zoh["bw"][0], log=True)
    res += [("zoh state", st), ("zoh out", out), ("zoh status", status), ("zoh log", log)]
    st = fresh(ctl, S["q"], S["v"])
    out, status = ctl.rollout_zoh(st, 2, 2, ref=zoh["refs"][:2].contiguous())
    res += [("ref state", st), ("ref out", out), ("ref status", status)]
    st, m = fresh(ctl, S["q"], S["v"]), ctl.new_metrics(0.3, 0.2)
    r = ctl.rollout_zoh_ex(st, 2, 2, base_wrench=zoh["bw"][:2].contiguous(), log=True, trace_every=1, metrics=m)
    res += [("ex state", st), ("ex metrics", m)] + [("ex " + k, r[k]) for k in ("out", "status", "log", "trace")]
    st = fresh(ctl, S["q"], S["v"])
    r = ctl.rollout_zoh_io(st, 2, 2, meas=zoh["meas"][:2].contiguous(), applied=True, log=True)
    res += [("io state", st)] + [("io " + k, r[k]) for k in ("out", "status", "log", "applied")]
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def zoh():
    """A wrench per tick, a CoM reference per tick and a measurement error per tick for 16 robots and 6 control ticks."""
    S = gc.tilted_states()
    ctl = _ctl(S, warm_start=1)
    ctl.set_refs_stance(2.0, 2)
    dev = ctl.device
    out0, _ = ctl.stand_step(fresh(ctl, S["q"], S["v"]))
    refs = torch.full((6, B, 16), -7.0e3, dtype=torch.float64, device=dev)
    d = np.random.default_rng(20261023).uniform(-1.0, 1.0, (6, B, 6)) * np.array([0.005, 0.02, 0.1, 0.005, 0.02, 0.1])
    refs[:, :, 0:6] = out0[:, 72:78] + torch.as_tensor(d).to(dev)
    res = dict(bw=torch.as_tensor(zx.wrench_sequence(20261024, 6)).to(dev), refs=refs, meas=torch.as_tensor(zi.measurement_noise(20261025, 6)).to(dev))
    torch.cuda.synchronize()
    ctl.close()
    return res


def test_a_cleared_table_is_a_handle_that_never_had_one(zoh):
    S = gc.tilted_states()
    a, b = _ctl(S, warm_start=1), _ctl(S, warm_start=1)
    for c in (a, b):
        c.set_refs_stance(2.0, 2)
    a.set_ground(S["planes"])
    with_table = _every_call(a, S, zoh)
    a.set_ground(None)
    assert not a.ground_per_instance and _same(a.get_ground(3), gc.FLAT)
    cleared, never = _every_call(a, S, zoh), _every_call(b, S, zoh)
    _assert_same("cleared", [(n, x, y) for (n, x), (_, y) in zip(cleared, never)])
    differ = {n for (n, x), (_, y) in zip(with_table, never) if not _same(x, y)}
    assert {"contact", "xdot", "step", "zoh state", "ref state", "ex state", "io state"} <= differ, differ       # the table mattered
    a.close(); b.close()


# ------------------------------------------------------------------------------- 3. ledge
def test_a_ledge_is_the_flat_ground_under_a_lowered_robot():
    """Horizontal planes h_R = +3 mm, h_L = -2 mm at states whose base does not turn (v[3:6] = 0: lowering the robot then moves no vertex
    velocity): the right foot's vertex forces are those of a call without a table with q[2] - h_R, the left foot's with q[2] - h_L."""
    from linearmpchumanoid_amd import trajectories
    S = gc.tilted_states()
    hr, hl = 3.0e-3, -2.0e-3
    v = S["v"].copy(); v[:, 3:6] = 0.0
    ledge, none = _ctl(S, planes=trajectories.ground_planes(0.0, 0.0, hr, hl)), _ctl(S)
    got = _split(ledge.contact_wrench(to_device(ledge, S["q"]), to_device(ledge, v)).cpu().numpy())["vertex_force"]
    worst, n_in = 0.0, [0, 0]
    for foot, h in ((0, hr), (1, hl)):
        q = S["q"].copy(); q[:, 2] -= h
        want = _split(none.contact_wrench(to_device(none, q), to_device(none, v)).cpu().numpy())["vertex_force"]
        for i in range(B):
            scale = _scale(S["pos"][i], S["vel"][i])
            a, b = got[i, 4 * foot:4 * foot + 4], want[i, 4 * foot:4 * foot + 4]
            assert np.array_equal(a == 0.0, b == 0.0) and close_on(a, b, 1e-11, scale), (foot, i, np.abs(a - b).max() / scale)
            worst, n_in[foot] = max(worst, float(np.abs(a - b).max() / scale)), n_in[foot] + int((b != 0.0).any())
    print("\nledge: worst %.2e of the force scale; states in contact right %d, left %d" % (worst, *n_in))
    assert n_in[0] > 0 and n_in[1] > 0
    ledge.close(); none.close()


# ------------------------------------------------------------------------------- 4. derivative
_ref = {}


def _derivative_reference():
    if not _ref:
        S, o = gc.tilted_states(), pc.make_oracle()
        _ref["r"] = [gc.ground_plant_xdot(o, S["q"][i], S["v"][i], S["tau"][i], S["planes"][i]) for i in range(B)]
    return _ref["r"]


def test_plant_derivative_against_the_helper():
    S, ref = gc.tilted_states(), _derivative_reference()
    ctl = _ctl(S, planes=S["planes"])
    q, v, tau = (to_device(ctl, S[k]) for k in ("q", "v", "tau"))
    xdot, c, flags = ctl.plant_derivative(q, v, tau)
    cw = ctl.contact_wrench(q, v)
    torch.cuda.synchronize()
    assert _same(c, cw) and int(flags.abs().max()) == 0           # the contact record is contact_wrench's, bitwise
    xdot = xdot.cpu().numpy()
    for i in range(B):
        want, r = ref[i]
        M, J, Cv = r["terms"]["M"], r["terms"]["J"], r["terms"]["C"]
        qdd = xdot[i, 30:]
        x = np.concatenate([r["terms"]["X"][0] @ np.concatenate([qdd[3:6], qdd[0:3]]), qdd[6:]])
        rhs = S["tau"][i] + J.T @ r["w"] - Cv
        e = rel_err(xdot[i, :30], want[:30])
        back = _ninf(M @ x - rhs) / (_ninf(M) * _ninf(x) + _ninf(rhs))
        fwd = _ninf(x - r["a"]) / (np.linalg.cond(M) * _ninf(r["a"]))
        print("robot %2d: qdot %.2e, backward %.2e, forward/cond %.2e" % (i, e, back, fwd))
        assert np.isfinite(xdot[i]).all() and e <= 1e-13 and back <= 1e-12 and fwd <= 1e-12, (i, e, back, fwd)
    ctl.close()


# ------------------------------------------------------------------------------- 5. step
def test_plant_step_composition_and_parity():
    S = gc.tilted_states()
    ctl = _ctl(S, planes=S["planes"])
    tau_np = np.random.default_rng(20261020).normal(0.0, 0.05, (B, 30))
    tau = to_device(ctl, tau_np)
    mk = lambda: fresh(ctl, S["q"], S["v"], 0.25)
    s20, f20 = ctl.plant_step(mk(), tau, 20)
    s7, _ = ctl.plant_step(mk(), tau, 7)
    s713, _ = ctl.plant_step(s7.clone(), tau, 13)
    torch.cuda.synchronize()
    assert torch.equal(s713, s20) and int(f20.abs().max()) == 0    # step(7) then step(13) is step(20), bit for bit
    o, a, worst = pc.make_oracle(), s20.cpu().numpy(), 0.0
    for i in range(B):
        ref = gc.ground_plant_steps(o, np.concatenate([S["q"][i], S["v"][i]]), tau_np[i], S["planes"][i], 20, DT)
        worst = max(worst, rel_err(a[i, :60], ref))
        assert close(a[i, :60], ref, 1e-7), (i, rel_err(a[i, :60], ref))
    print("\nplant step on the tilted planes vs the helper's RK4, 20 substeps: %.2e" % worst)
    ctl.close()


# ------------------------------------------------------------------------------- 6. per robot
def test_robot_i_is_a_one_robot_handle_with_record_i():
    """ONE state under 16 grounds: slopes of 0.5 .. 8 degrees in 16 directions, each foot's plane 2 mm above that foot's lowest vertex."""
    from linearmpchumanoid_amd import trajectories
    S = gc.tilted_states()
    k = 2                                                          # a sticking state
    planes = trajectories.ground_planes(np.deg2rad(0.5 * (1 + np.arange(B))), 0.4 * np.arange(B))
    for i in range(B):
        for f in range(2):
            n = planes[i, 4 * f:4 * f + 3]
            planes[i, 4 * f + 3] = (S["pos"][k, 4 * f:4 * f + 4] @ n).min() + 2.0e-3
    q, v, tau = (np.tile(S[name][k], (B, 1)) for name in ("q", "v", "tau"))

    def run(ctl, n):
        ctl.set_refs_stance(2.0, 2)
        dq, dv, dtau = (to_device(ctl, x[:n]) for x in (q, v, tau))
        xdot, _, _ = ctl.plant_derivative(dq, dv, dtau)
        step, _ = ctl.plant_step(fresh(ctl, q[:n], v[:n]), dtau, 3)
        st = fresh(ctl, q[:n], v[:n])
        out, status, log = ctl.rollout_zoh(st, 3, 2, log=True)
        res = dict(contact=ctl.contact_wrench(dq, dv), xdot=xdot, step=step, zoh_state=st, zoh_out=out, zoh_status=status, zoh_log=log[:, :n])
        torch.cuda.synchronize()
        return {name: t.cpu() for name, t in res.items()}

    whole = _ctl(S, planes=planes, warm_start=1)
    batch = run(whole, B)
    whole.close()
    for i in range(B):
        one = _ctl(S, n=1, planes=planes[i], warm_start=1)
        single = run(one, 1)
        one.close()
        for name, t in single.items():
            mine = batch[name][:, i:i + 1] if name == "zoh_log" else batch[name][i:i + 1]
            assert _same(mine.contiguous(), t.contiguous()), (i, name)
    for name in ("contact", "xdot", "step", "zoh_state"):
        rows = {batch[name][i].numpy().tobytes() for i in range(B)}
        assert len(rows) == B, (name, len(rows))


# ------------------------------------------------------------------------------- 7. closed loop
NB, NT, NS = 8, 6, 3
PUSH_TICKS = [[4, -1], [7, -1], [0, -1], [6, -1], [4, 5], [10, 11], [17, -1], [2, 9]]      # inside holds, on tick boundaries, at the start


@pytest.fixture(scope="module")
def loop(zoh):
    S = gc.tilted_states()
    S8 = dict(q=S["q"][:NB], v=S["v"][:NB], zcom=S["zcom"])
    mk = lambda: _ctl(S, n=NB, planes=S["planes"][:NB], warm_start=1)
    ctl, plain = mk(), mk()                                        # pushes and actuator records | neither: the host loop's handle, on the same ground
    for c in (ctl, plain):
        c.set_refs_stance(2.0, 2)
    ticks, dv = np.array(PUSH_TICKS, dtype=np.int64), np.stack([zx.push_dv(20261030 + i, 2) for i in range(NB)])
    ctl.set_pushes(ticks, dv)
    tau_max = 0.05 + 0.1 * ((np.arange(NB)[:, None] + np.arange(24)[None, :]) % 5)
    tau_max[0::4] = np.inf
    rec = zi.robot_records(np.tile(tau_max, (2, 1)))[:NB]
    rec[:, 48] = np.arange(NB) % 4                                 # delays 0 .. 3
    ctl.set_actuators(tau_max=rec[:, 0:24], alpha=rec[:, 24:48], delay=rec[:, 48])
    cut = lambda t: t[:, :NB].contiguous()
    out0, _ = plain.stand_step(fresh(plain, S8["q"], S8["v"]))
    yield dict(S=S8, ctl=ctl, plain=plain, ticks=ticks, dv=dv, bw=cut(zoh["bw"]), refs=cut(zoh["refs"]), meas=cut(zoh["meas"]),
               rec=torch.as_tensor(rec).to(ctl.device), tau0=out0[:, 0:24].contiguous() * 0.5)
    ctl.close(); plain.close()


def _st(ctl, lp):
    return fresh(ctl, lp["S"]["q"], lp["S"]["v"])


def test_rollout_zoh_is_the_host_loop_bit_for_bit(loop):
    ctl, plain = loop["ctl"], loop["plain"]
    sa, sb = _st(ctl, loop), _st(plain, loop)
    out, status, log = ctl.rollout_zoh(sa, NT, NS, base_wrench=loop["bw"][0], log=True)
    rb = host_loop(plain, sb, plain.new_status(), NT, NS, bw=loop["bw"][0])
    torch.cuda.synchronize()
    _assert_same("rollout_zoh", (("state", sa, sb), ("out", out, rb["out"]), ("status", status, rb["status"]), ("log", log, rb["log"])))
    sa, sb = _st(ctl, loop), _st(plain, loop)
    out, status, log = ctl.rollout_zoh(sa, NT, NS, ref=loop["refs"], log=True)
    rb = host_loop(plain, sb, plain.new_status(), NT, NS, refs=loop["refs"])
    torch.cuda.synchronize()
    _assert_same("rollout_zoh(ref=)", (("state", sa, sb), ("out", out, rb["out"]), ("status", status, rb["status"]), ("log", log, rb["log"])))
    # the ground is in the loop: the same launch on a handle without a table ends elsewhere on every robot
    none = _ctl(dict(zcom=loop["S"]["zcom"]), n=NB, warm_start=1)
    none.set_refs_stance(2.0, 2)
    sc = _st(none, loop)
    none.rollout_zoh(sc, NT, NS, ref=loop["refs"])
    torch.cuda.synchronize()
    assert all(not _same(sa[i], sc[i]) for i in range(NB))
    none.close()


def _ex(ctl, lp, n_ticks, st=None, status=None, first=0, every=1, metrics=None):
    st = _st(ctl, lp) if st is None else st
    cut = slice(first, first + n_ticks)
    r = ctl.rollout_zoh_ex(st, n_ticks, NS, base_wrench=lp["bw"][cut].contiguous(), pushes=True, log=True, trace_every=every, metrics=metrics, status=status)
    return dict(r, state=st)


def test_rollout_zoh_ex_is_the_host_loop_bit_for_bit(loop):
    """A push inside a hold (substep 4 of 3-substep holds) and on tick boundaries, a wrench per tick, an every-tick trace, the metrics;
    (2 + 4) ticks are (2) then (4)."""
    from linearmpchumanoid_amd import metrics as hm
    ctl, plain = loop["ctl"], loop["plain"]
    m6, m24 = ctl.new_metrics(0.3, 0.2), ctl.new_metrics(0.3, 0.2)
    ra = _ex(ctl, loop, NT, metrics=m6)
    sb = _st(plain, loop)
    rb = host_loop(plain, sb, plain.new_status(), NT, NS, bw=loop["bw"], sched=(loop["ticks"], loop["dv"]))
    torch.cuda.synchronize()
    _assert_same("rollout_zoh_ex", (("state", ra["state"], sb), ("out", ra["out"], rb["out"]), ("status", ra["status"], rb["status"]), ("log", ra["log"], rb["log"]),
                                    ("trace", ra["trace"], rb["trace"])))
    assert _same(m6.cpu().numpy(), hm.fold_trace(hm.identity(NB, 0.3, 0.2), rb["trace"].cpu().numpy()))
    r2 = _ex(ctl, loop, 2, metrics=m24)
    status2 = r2["status"].clone()
    r4 = _ex(ctl, loop, 4, st=r2["state"], status=r2["status"].clone(), first=2, metrics=m24)
    torch.cuda.synchronize()
    _assert_same("split", (("state", ra["state"], r4["state"]), ("out", ra["out"], r4["out"]), ("log", ra["log"], torch.cat([r2["log"], r4["log"]])), ("metrics", m6, m24)))
    s6, s4 = ra["status"], r4["status"]
    assert torch.equal(s6[:, 0], s4[:, 0]) and torch.equal(s6[:, 3], s4[:, 3])
    assert torch.equal(s6[:, 1], torch.maximum(status2[:, 1], s4[:, 1])) and torch.equal(s6[:, 2], status2[:, 2] | s4[:, 2])


def test_rollout_zoh_io_is_the_host_loop_bit_for_bit(loop):
    """A measurement error and actuators with delays 0 .. 3, limits and lags, on top of the pushes and the wrench per tick."""
    ctl, plain = loop["ctl"], loop["plain"]
    sa, sb = _st(ctl, loop), _st(plain, loop)
    mem_a, mem_b = ctl.new_act_mem(loop["tau0"]), plain.new_act_mem(loop["tau0"])
    ra = ctl.rollout_zoh_io(sa, NT, NS, meas=loop["meas"], actuators=True, act_mem=mem_a, applied=True, base_wrench=loop["bw"], ref=loop["refs"], pushes=True,
                            log=True, trace_every=1)
    rb = host_loop(plain, sb, plain.new_status(), NT, NS, bw=loop["bw"], sched=(loop["ticks"], loop["dv"]), refs=loop["refs"], meas=loop["meas"],
                   act=(loop["rec"], mem_b))
    torch.cuda.synchronize()
    _assert_same("rollout_zoh_io", (("state", sa, sb), ("out", ra["out"], rb["out"]), ("status", ra["status"], rb["status"]), ("log", ra["log"], rb["log"]),
                                    ("trace", ra["trace"], rb["trace"]), ("applied", ra["applied"], rb["applied"]), ("act_mem", mem_a, mem_b)))
    assert not _same(ra["applied"], ra["log"][:, :, 0:24].contiguous())                # the actuator changed what the plant received


def test_captured_on_a_fresh_handle_replays_to_the_eager_bytes(loop):
    from linearmpchumanoid_amd import capi, metrics as hm
    S = gc.tilted_states()
    p = lambda t: C.c_void_p(t.data_ptr())
    ctl = _ctl(S, n=NB, planes=S["planes"][:NB], warm_start=1)    # fresh: set_ground, then no launch before the capture
    ctl.set_refs_stance(2.0, 2)
    ctl.set_pushes(loop["ticks"], loop["dv"])
    dev = ctl.device
    ident = torch.as_tensor(hm.identity(NB, 0.3, 0.2)).to(dev)
    st0 = _st(ctl, loop)
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    st, out, status, log, trace, m = st0.clone(), sent(NB, 80), ctl.new_status(), sent(NT, NB, 36), sent(NT, NB, 180), ident.clone()
    bw = loop["bw"]
    opts = capi.LmhZohOpts(d_base_wrench=p(bw), d_ref=None, d_log=p(log), d_trace=p(trace), d_metrics=p(m), trace_every=1, wrench_per_tick=1, pushes=1, reserved=0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = capi.lib().lmh_rollout_zoh_ex(ctl._h, p(st), p(out), p(status), C.byref(opts), NT, NS, ctl._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _same(st, st0) and bool((out == -7).all()) and _same(m, ident)          # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (st, out, status, log, trace, m)]
    del g
    e_st, e_m = st0.clone(), ident.clone()                         # (the same sentinels: the launch does not write the out record's pads)
    e = ctl.rollout_zoh_ex(e_st, NT, NS, base_wrench=bw, pushes=True, log=sent(NT, NB, 36), trace_every=1, trace=sent(NT, NB, 180), metrics=e_m, out=sent(NB, 80))
    torch.cuda.synchronize()
    for name, a, b in zip(("state", "out", "status", "log", "trace", "metrics"), got, (e_st, e["out"], e["status"], e["log"], e["trace"], e_m)):
        assert _same(a, b), name
    assert float(got[5][0, 0]) == NT
    ctl.close()


# ------------------------------------------------------------------------------- 8. refusals and the setter rule
def test_the_table_reads_back_empty_shared_per_robot_and_after_a_refused_set():
    S = gc.tilted_states()
    ctl = _ctl(S, n=2)
    planes = np.ascontiguousarray(S["planes"][:2])
    bad = planes.copy(); bad[1, 0:3] *= 2.0
    check_record_table(ctl, "ground", gc.FLAT, planes, bad, "a ground normal must have unit length (| |n|^2 - 1 | <= 1e-12; nothing is normalised here)")
    ctl.close()


def test_refusals_leave_the_table_in_place():
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.capi import LmhError
    S = gc.tilted_states()
    ctl = _ctl(S, planes=S["planes"], warm_start=1)
    ctl.set_refs_stance(2.0, 2)
    kept = lambda: all(_same(ctl.get_ground(i), S["planes"][i]) for i in range(B)) and ctl.ground_per_instance
    bad = S["planes"].copy(); bad[7, 0:3] *= 1.0 + 1e-9
    with pytest.raises(LmhError, match=r"robot 7: a ground normal must have unit length") as e:
        ctl.set_ground(bad)
    assert e.value.code == -2 and kept()
    bad = S["planes"].copy(); bad[5, 4:7] = [0.0, 1.0, 0.0]
    with pytest.raises(LmhError, match=r"robot 5: a ground normal must point up \(n_z > 0\)"):
        ctl.set_ground(bad)
    assert kept()
    bad = S["planes"].copy(); bad[9, 6] = -bad[9, 6]
    with pytest.raises(LmhError, match=r"robot 9: a ground normal must point up"):
        ctl.set_ground(bad)
    assert kept()
    bad = S["planes"].copy(); bad[11, 3] = np.nan; bad[12, 0:3] *= 2.0
    with pytest.raises(LmhError, match=r"robot 11: every word of a ground record must be finite"):
        ctl.set_ground(bad)
    assert kept()
    with pytest.raises(LmhError, match=r"lmh_set_ground: n_sets must be 1 or n_instances"):
        ctl.set_ground(S["planes"][:3])
    assert kept()
    with pytest.raises(ValueError):
        ctl.set_ground(np.zeros((B, 7)))
    assert kept()
    one = _ctl(S, plant=1)
    with pytest.raises(LmhError, match=r"lmh_set_ground: not offered on a plant = 1 handle"):
        one.set_ground(gc.FLAT)
    assert _same(one.get_ground(0), gc.FLAT) and not one.ground_per_instance
    one.close()
    # rollout_zoh_box on a handle with a table: refused before anything is enqueued
    L, p = capi.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    ns = L.lmh_num_ref_samples(ctl._h)
    box = torch.tensor([-1.0, 1.0, -1.0, 1.0], dtype=torch.float64, device=ctl.device)[:, None].repeat(1, ns).contiguous()
    st0 = fresh(ctl, S["q"], S["v"])
    st, out, status = st0.clone(), torch.full((B, 80), -7.0, dtype=torch.float64, device=ctl.device), ctl.new_status()
    status0 = status.clone()
    rc = L.lmh_rollout_zoh_box(ctl._h, p(st), p(out), p(status), None, p(box), ns, 1, None, 3, 2, ctl._stream())
    torch.cuda.synchronize()
    assert rc == -2 and "lmh_rollout_zoh_box: not offered on a handle with a ground table" in L.lmh_last_error().decode()
    assert _same(st, st0) and bool((out == -7).all()) and _same(status, status0) and kept()
    ctl.set_ground(None)                                           # and accepted again without one
    assert L.lmh_rollout_zoh_box(ctl._h, p(st), p(out), p(status), None, p(box), ns, 1, None, 1, 1, ctl._stream()) == 0
    torch.cuda.synchronize()
    ctl.close()


# ------------------------------------------------------------------------------- 9. the handle is untouched
def test_every_other_call_reads_nothing_of_the_table():
    S = gc.tilted_states()
    a, b = _ctl(S, planes=S["planes"]), _ctl(S)
    res = []
    for ctl in (a, b):
        ctl.set_refs_stance(2.0, 2)
        st = fresh(ctl, S["q"], S["v"])
        out, status = ctl.stand_step(st)
        st10 = fresh(ctl, S["q"], S["v"])
        out10, status10, log10 = ctl.rollout(st10, 10, log=True)
        terms = ctl.terms(to_device(ctl, S["q"]), to_device(ctl, S["v"]))
        mpc = ctl.mpc_step(ctl.new_lip((0.01, -0.01), (0.05, 0.02), t=0.1))
        torch.cuda.synchronize()
        res.append((("eval state", st), ("eval out", out), ("eval status", status), ("rollout state", st10), ("rollout out", out10), ("rollout status", status10),
                    ("rollout log", log10), ("terms", terms), ("mpc", mpc)))
    _assert_same("with and without a table", [(n, x, y) for (n, x), (_, y) in zip(*res)])
    a.close(); b.close()
