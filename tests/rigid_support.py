"""GPU-side helpers of the rigid-plant tests (randomised_links also of test_gpu_plant_step.py): mode words, states, the device's own terms,
and the one walk over the batch by which the derivative and the impact are held to their numpy statements.  Not a test file."""
import numpy as np
import torch

import plant_step_cases as pc
import rigid_cases as rc
from helpers import make_controller, same_bits, to_device

DT, TH, B = pc.DT, pc.TH, pc.B


def imode(ctl, m):
    return torch.as_tensor(np.ascontiguousarray(m, dtype=np.int32)).to(ctl.device)


def fresh(ctl, S, t0=0.0, v_prev=None):
    st = ctl.new_state(S["q"], S["v"], t=t0, v_prev=S["v"] if v_prev is None else v_prev)
    st[:, 91:96] = torch.arange(1.0, 6.0, dtype=torch.float64, device=ctl.device)          # the pads: left alone
    return st


def randomised_links(n):
    from linearmpchumanoid_amd.controller import nominal_links
    raw = np.tile(nominal_links(), (n, 1, 1))
    rng = np.random.default_rng(20260004)
    raw[:, :, 0] *= rng.uniform(0.9, 1.1, (n, 28))
    raw[:, :, 1:4] += rng.uniform(-5e-3, 5e-3, (n, 28, 3)) * (raw[:, :, 0:1] > 0)
    return raw


def device_terms(ctl, S, q=None, v=None):
    """The GPU's own terms(q, v) record (M, C, J, Jpqp); vhat and the base's X_0, pure functions of the base pose, stay the oracle's."""
    t = ctl.split_terms(ctl.terms(to_device(ctl, S["q"] if q is None else q), to_device(ctl, S["v"] if v is None else v)).cpu().numpy())
    return [dict(M=t["M"][i], C=t["C"][i], J=t["J"][i], Jpqp=t["Jpqp"][i], vhat=S["terms"][i]["vhat"], X=S["terms"][i]["X"]) for i in range(B)]


def check_figures(b, out, lam, rows, worst, where):
    """One robot's answer: finite, exact zeros on the rows that are not held, the three figures of b <= 1e-12 (worst keeps the largest)."""
    for k in worst:
        worst[k] = max(worst[k], b[k])
    assert np.isfinite(out).all() and not lam[[r for r in range(12) if r not in rows]].any(), where
    assert b["backward"] <= 1e-12 and b["constraint"] <= 1e-12 and b["forward"] <= 1e-12, (where, b)


def against_the_statement(ctl, what, tag, kvs, call, robot):
    """The walk of the derivative and of the impact against their statements: modes mixed over the batch (mode[i] = (i + s) % 3,
    s = 0, 1, 2), every kv of kvs, one launch each by call(mode tensor, kv) -> (out, lam, flags), device tensors [B, .].
    robot(i, mode_i, kv, out_i, lam_i, flags_i, where) runs the numpy statement on the caller's terms of robot i, makes the caller's flag
    assertion and -> (bounds of the device's answer, rows held, the statement's flags, flag decisions it did not compare).  Per robot
    check_figures, and neither FLAG_NOT_SPD nor FLAG_NONFINITE.  -> (worst figures, flag decisions not compared)."""
    from linearmpchumanoid_amd import capi
    worst, undecided = dict(backward=0.0, constraint=0.0, forward=0.0), 0
    for s in range(3):
        mode = [(i + s) % 3 for i in range(B)]
        for kv in kvs:
            out, lam, flags = call(imode(ctl, mode), kv)
            torch.cuda.synchronize()
            out, lam, flags = out.cpu().numpy(), lam.cpu().numpy(), flags.cpu().numpy()
            for i in range(B):
                b, rows, flags_s, skipped = robot(i, mode[i], kv, out[i], lam[i], flags[i], (tag, s, kv, i))
                print("\n%s vs the statement on %s, shift %d, kv %s, robot %d: backward %.2e constraint %.2e forward/cond %.2e flags %d (statement %d)"
                      % (what, tag, s, kv, i, b["backward"], b["constraint"], b["forward"], flags[i], flags_s), end="")
                check_figures(b, out[i], lam[i], rows, worst, (tag, s, kv, i))
                assert not flags[i] & (capi.FLAG_NOT_SPD | capi.FLAG_NONFINITE), (tag, s, kv, i, flags[i])
                undecided += skipped
    print("\n%s vs the statement on %s: backward %.2e, constraint %.2e, forward/cond %.2e (flags not compared: %d)"
          % (what, tag, worst["backward"], worst["constraint"], worst["forward"], undecided))
    return worst, undecided


def flight_against_the_plain_derivative(ctl, q, v, tau, tag):
    """States out of the ground, LMH_PHASE_FLIGHT, kv 0 and 50: xdot is lmh_plant_derivative's bit for bit, lambda and the flags exactly 0
    -> (that xdot, xdot with both soles held at kv = 0) for the caller's last assertion: a constraint knows no plane."""
    xd, c, f = ctl.plant_derivative(q, v, tau)
    for kv in rc.KVS:
        xr, lam, fr = ctl.plant_derivative_rigid(q, v, tau, imode(ctl, np.full(B, 3)), kv)
        torch.cuda.synchronize()
        assert float(c.abs().max()) == 0.0 and int(f.abs().max()) == 0 and bool(torch.isfinite(xd).all())
        worst = float(((xr - xd).abs() / xd.abs().clamp_min(1e-300)).max())
        print("\nflight vs plant_derivative, %skv = %g: largest relative difference %.2e" % (tag, kv, worst))
        assert same_bits(xr, xd) and float(lam.abs().max()) == 0.0 and int(fr.abs().max()) == 0
    held, _, _ = ctl.plant_derivative_rigid(q, v, tau, None, 0.0)
    torch.cuda.synchronize()
    return xd, held


def flag_margins(lam, rows, mu=rc.MU):
    """Which of the two informational flags the statement decides by more than 1e-9 N on this case -> (pull decided, slip decided)."""
    held = [ft for ft in range(2) if 6 * ft in rows]
    pull = all(abs(lam[6 * ft + 5]) > 1e-9 for ft in held)
    slip = all(abs(np.hypot(lam[6 * ft + 3], lam[6 * ft + 4]) - mu * lam[6 * ft + 5]) > 1e-9 for ft in held)
    return pull, slip


def derivative_against(terms_of, tag, S=None, decided=None):
    """Modes mixed over the batch, kv 0 and 50, against the statement on terms_of(i).  S: the states (q, v, tau, zcom and the oracle's
    terms for X_0; rigid_cases.rigid_cases() by default); decided(lam, rows, bounds) -> (pull, slip): which flags the statement's
    multiplier decides (by 1e-9 N by default).  test_gpu_fall_rigid.py runs the same checks on the states of a fall.
    -> (worst figures, flag decisions not compared)."""
    from linearmpchumanoid_amd import capi
    S = rc.rigid_cases() if S is None else S
    decided = (lambda lam, rows, b: flag_margins(lam, rows)) if decided is None else decided
    ctl = make_controller(B, DT, TH, S["zcom"])
    q, v, tau = (to_device(ctl, S[k]) for k in ("q", "v", "tau"))
    xd_plain, _, _ = ctl.plant_derivative(q, v, tau)

    def call(mode, kv):
        xdot, lam, flags = ctl.plant_derivative_rigid(q, v, tau, mode, kv)
        torch.cuda.synchronize()
        assert same_bits(xdot[:, :30], xd_plain[:, :30])           # qdot: lmh_plant_derivative's, bit for bit
        return xdot, lam, flags

    def robot(i, mode, kv, xdot, lam, flags, where):
        tm, info = terms_of(i), {}
        _, lam_s, flags_s = rc.rigid_contact_acceleration(tm["M"], tm["C"], tm["J"], tm["Jpqp"], tm["vhat"], S["tau"][i], mode, kv, contact_mu=rc.MU, info=info)
        b = rc.bounds(tm, S["tau"][i], mode, kv, rc.a_from_xdot(xdot, S["terms"][i]["X"][0]), lam)
        pull, slip = decided(lam_s, info["rows"], b)
        if pull:
            assert (flags & capi.FLAG_CONTACT_PULL) == (flags_s & capi.FLAG_CONTACT_PULL), where
        if slip:
            assert (flags & capi.FLAG_CONTACT_SLIP) == (flags_s & capi.FLAG_CONTACT_SLIP), where
        return b, info["rows"], flags_s, (not pull) + (not slip)

    worst, undecided = against_the_statement(ctl, "rigid derivative", tag, rc.KVS, call, robot)
    assert undecided <= 8                                          # the margins leave the comparison its cases
    return worst, undecided
