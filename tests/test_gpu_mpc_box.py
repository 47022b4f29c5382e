"""GPU tests of the box-constrained MPC calls (include/lmh.h: lmh_mpc_box_preview, lmh_mpc_box_step, lmh_mpc_box_rollout).

  statement   at every horizon and mpc_dt of mpc_box_cases.CASES, with per-robot and with shared bounds: the working set, its sides, k, flags
              and active counts of the numpy statement; multipliers exactly zero off the set, Z exactly the bound on it and inside the box
              everywhere; U, lambda, Z and the CoM arrays within the derived bounds (mpc_box_cases.py).  The round count is not judged.
  identities  (I1) the step is formed from the preview record, (I2) the rollout is the host loop of steps, splits and runs without a
              trajectory, (I3) bounds that never bind leave lmh_mpc_preview's bytes.
  faults      an empty and a NaN box sample are flagged and stay with their robots.
  the handle is untouched, refusals enqueue nothing, one captured graph of the three calls replays to the same bytes."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import mpc_box_cases as bc
import mpc_cases as mc
import preview_cases as pc
import helpers
from helpers import horizon_controller, same_bits

pytestmark = pytest.mark.gpu
B = bc.B


@pytest.fixture(scope="module")
def nao():
    o = pc.make_oracle(16, "coupled")
    return dict(zcom=o.zcom, q0=o.robot()["q"].copy())


def to_device(ctl, a):
    return helpers.to_device(ctl, np.array(a))                      # (the drawn cases are read-only: upload a copy)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def box_controller(N, mpc_dt, zcom):
    """B robots on the host plans, step lengths and LIPM heights of mpc_box_cases.draw(N, mpc_dt)."""
    d = bc.draw(N, mpc_dt)
    ctl = horizon_controller(B, N, zcom, mpc_dt, mc.DT)
    assert ctl.N == N
    p = d["plans"]
    ctl.set_plans(p["zmp_x"], p["zmp_y"], p["phase"], p["segs"], p["seg_of_sample"])
    ctl.set_xscale(d["xs"])
    ctl.set_zcom(d["zcoms"])
    return ctl, d


def fma(a, b, c):
    """The correctly rounded a * b + c of finite doubles."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ------------------------------------------------------------------------------- 1. against the numpy statement
@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("N,mpc_dt", bc.CASES)
def test_preview_against_the_statement(nao, N, mpc_dt, shared):
    from linearmpchumanoid_amd import capi
    ctl, d = box_controller(N, mpc_dt, nao["zcom"])
    rec = ctl.mpc_box_preview(to_device(ctl, d["lip"]), d["shared"] if shared else d["box"])
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    ctl.close()
    f = ctl.split_box_preview(rec, N)
    want = bc.statement(N, mpc_dt, shared)
    worst = dict(a=0.0, b=0.0, c=0.0, d=0.0)
    rounds = []
    for i, pv in enumerate(want):
        assert (f["k"][i], f["flags"][i], f["N"][i]) == (pv["k"], pv["flags"], N) and rec[i, 7] == 0
        for name, (off, extra) in capi.MPC_BOX_ARRAYS.items():
            assert (rec[i, off + N + extra:off + capi.MPC_PREVIEW_ARRAY] == 0).all(), name
            assert np.isfinite(rec[i, off:off + N + extra]).all(), name
        for ax, nm in enumerate("xy"):
            U, Z, lam = f["U_" + nm][i], f["Z_" + nm][i], f["lam_" + nm][i]
            side, lo, hi = pv["side"][ax], pv["lo"][ax], pv["hi"][ax]
            assert (np.sign(lam).astype(np.int64) == side).all(), (i, nm, np.sign(lam), side)       # the same working set and sides
            assert f["active_" + nm][i] == pv["active"][ax] == (lam != 0).sum()
            assert (Z[side > 0] == hi[side > 0]).all() and (Z[side < 0] == lo[side < 0]).all()      # Z is the bound itself
            assert (Z >= lo).all() and (Z <= hi).all()
            assert f["rounds_" + nm][i] <= capi.MPC_BOX_MAX_ROUNDS
            rounds.append(int(f["rounds_" + nm][i]))
            r = bc.check_against_statement(N, mpc_dt, i, ax, pv, U, lam, Z, f["C_" + nm][i], f["Cv_" + nm][i], shared)
            assert same_bits(np.ascontiguousarray(rec[i, [272 + 132 * ax, 338 + 132 * ax]]), np.ascontiguousarray(d["lip"][i, 2 * ax:2 * ax + 2]))
            worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"\nbox preview N = {N}, mpc_dt = {mpc_dt}, shared = {shared}: " + ", ".join(f"({k}) {v:.3g}" for k, v in worst.items()) +
          f" of the bounds; rounds mean {np.mean(rounds):.2f}, max {max(rounds)}")
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------- 2. the identities
@pytest.fixture(scope="module")
def roll(nao):
    """N = 16 at 10 ms; the host loop of 12 constrained steps is computed once and shared."""
    N, mpc_dt = 16, 1e-2
    ctl, d = box_controller(N, mpc_dt, nao["zcom"])
    lipn = d["lip"].copy()
    lipn[:, 5:8] = 7.0                                              # the pads of the state are the caller's
    lip0, box = to_device(ctl, lipn), to_device(ctl, d["box"])
    lip, tr = lip0.clone(), []
    for _ in range(12):
        rec = ctl.mpc_box_step(lip, box)
        tr.append(rec)
        lip[:, 0], lip[:, 1], lip[:, 2], lip[:, 3] = rec[:, 0], rec[:, 1], rec[:, 3], rec[:, 4]
        lip[:, 4] = lip[:, 4] + ctl.cfg.mpc_dt
    torch.cuda.synchronize()
    yield dict(ctl=ctl, d=d, lip0=lip0, box=box, end=lip, tr=torch.stack(tr), N=N, mpc_dt=mpc_dt)
    ctl.close()


@pytest.mark.parametrize("N,mpc_dt", ((2, 1e-2), (64, 1e-2), (16, 1e-3)))
def test_i1_the_step_is_formed_from_the_preview_record(nao, N, mpc_dt):
    ctl, d = box_controller(N, mpc_dt, nao["zcom"])
    lip = to_device(ctl, d["lip"])
    pv, st = ctl.mpc_box_preview(lip, d["box"]), ctl.mpc_box_step(lip, d["box"])
    torch.cuda.synchronize()
    pv, st = pv.cpu().numpy(), st.cpu().numpy()
    ctl.close()
    f = ctl.split_box_preview(pv, N)
    dt = np.float64(mpc_dt)
    want = np.zeros((B, 8))
    for i in range(B):
        for ax, nm in enumerate("xy"):
            x, xd, u = d["lip"][i, 2 * ax], d["lip"][i, 2 * ax + 1], f["U_" + nm][i][0]
            want[i, 3 * ax:3 * ax + 3] = fma((dt * dt) / 2, u, fma(1.0, x, dt * xd)), fma(dt, u, fma(0.0, x, 1.0 * xd)), u
            want[i, 6 + ax] = f["Z_" + nm][i][0]
    assert same_bits(np.ascontiguousarray(st[:, 0:8]), want)
    assert same_bits(np.ascontiguousarray(st[:, 8:13]), np.ascontiguousarray(d["lip"][:, 0:5]))
    assert list(st[:, 13]) == list(pv[:, 0]) and list(st[:, 14]) == list(pv[:, 1]) and list(st[:, 15]) == list(pv[:, 5] + pv[:, 6])
    assert (st[:, 15] > 0).any()


def test_i2_the_rollout_is_the_host_loop_of_steps(roll):
    ctl, box = roll["ctl"], roll["box"]
    lip = roll["lip0"].clone()
    tr = torch.full((12, B, 16), -7.0, dtype=torch.float64, device=ctl.device)
    assert ctl.mpc_box_rollout(lip, box, 12, traj=tr) is tr
    assert same_bits(lip, roll["end"]) and same_bits(tr, roll["tr"])
    assert bool((lip[:, 5:8] == 7.0).all()) and bool((tr[:, :, 15] > 0).any()) and bool((tr[:, 2:, 14] == 0).all())
    a = roll["lip0"].clone()
    ta, tb = ctl.mpc_box_rollout(a, box, 5), ctl.mpc_box_rollout(a, box, 7)
    assert same_bits(a, roll["end"]) and same_bits(torch.cat([ta, tb]), roll["tr"])
    quiet = roll["lip0"].clone()
    assert ctl.mpc_box_rollout(quiet, box, 12, traj=False) is None
    assert same_bits(quiet, roll["end"])
    first = ctl.split_mpc(roll["tr"][0].cpu().numpy())
    want = bc.statement(roll["N"], roll["mpc_dt"])
    assert list(first["k"]) == [pv["k"] for pv in want] and list(roll["tr"][0, :, 15].cpu().numpy()) == [float(pv["active"].sum()) for pv in want]


@pytest.mark.parametrize("N,mpc_dt", ((1, 1e-2), (16, 1e-2), (64, 1e-2)))
def test_i3_bounds_that_never_bind_leave_the_previews_bytes(nao, N, mpc_dt):
    from linearmpchumanoid_amd import capi
    ctl, d = box_controller(N, mpc_dt, nao["zcom"])
    lip = to_device(ctl, d["lip"])
    plain = ctl.mpc_preview(lip)
    inf = np.tile(np.array([-np.inf, np.inf, -np.inf, np.inf])[:, None], (1, d["n"]))
    wide = np.tile(np.array([-10.0, 10.0, -10.0, 10.0])[None, :, None], (B, 1, d["n"]))
    for box in (inf, wide):
        rec = ctl.mpc_box_preview(lip, box)
        torch.cuda.synchronize()
        assert same_bits(rec[:, :capi.MPC_PREVIEW_STRIDE].contiguous(), plain)
        assert bool((rec[:, 3:8] == 0).all()) and bool((rec[:, capi.MPC_PREVIEW_STRIDE:] == 0).all())
        step, free = ctl.mpc_box_step(lip, box).cpu().numpy(), ctl.mpc_step(lip).cpu().numpy()
        assert same_bits(np.ascontiguousarray(step[:, 8:16]), np.ascontiguousarray(free[:, 8:16]))
        assert same_bits(np.ascontiguousarray(step[:, 2]), plain[:, 8].cpu().numpy()) and same_bits(np.ascontiguousarray(step[:, 5]), plain[:, 74].cpu().numpy())
    ctl.close()


# ------------------------------------------------------------------------------- 3. faults stay with their robot
def test_an_empty_and_a_nan_box_sample_stay_with_their_robots(roll):
    from linearmpchumanoid_amd import capi
    ctl, d, N = roll["ctl"], roll["d"], roll["N"]
    lip = roll["lip0"]
    good_pv, good_st = ctl.mpc_box_preview(lip, roll["box"]), ctl.mpc_box_step(lip, roll["box"])
    box = d["box"].copy()
    k5, k6 = mc.k_of(d["lip"][5, 4], roll["mpc_dt"]), mc.k_of(d["lip"][6, 4], roll["mpc_dt"])
    box[5, 0, k5 + 3] = box[5, 1, k5 + 3] + 1e-3                    # lo_x > hi_x inside robot 5's window
    box[6, 3, k6 + N] = np.nan                                      # a NaN bound at the last sample of robot 6's
    pv, st = ctl.mpc_box_preview(lip, box), ctl.mpc_box_step(lip, box)
    end = lip.clone()
    tr = ctl.mpc_box_rollout(end, box, 3)
    torch.cuda.synchronize()
    others = [0, 1, 2, 3, 4, 7]
    assert same_bits(pv[others], good_pv[others]) and same_bits(st[others], good_st[others]) and same_bits(tr[:, others], roll["tr"][:3, others])
    pvn, stn, trn = pv.cpu().numpy(), st.cpu().numpy(), tr.cpu().numpy()
    for i in (5, 6):
        assert int(pvn[i, 1]) == capi.FLAG_BOX_EMPTY | capi.FLAG_NONFINITE and (pvn[i, 3:8] == 0).all()
        for name, (off, extra) in capi.MPC_BOX_ARRAYS.items():
            assert np.isnan(pvn[i, off:off + N + extra]).all() and (pvn[i, off + N + extra:off + 66] == 0).all(), name
        assert int(stn[i, 14]) == capi.FLAG_BOX_EMPTY | capi.FLAG_NONFINITE and np.isnan(stn[i, 0:8]).all() and stn[i, 15] == 0
        assert (trn[:, i, 14].astype(np.int64) & capi.FLAG_NONFINITE).all() and int(trn[0, i, 14]) & capi.FLAG_BOX_EMPTY
        assert np.isnan(end[i, 0:4].cpu().numpy()).all()


# ------------------------------------------------------------------------------- 4. the handle, refusals, capture
def test_the_handle_is_untouched(nao):
    ctl, d = box_controller(16, 1e-2, nao["zcom"])

    def whole_body():
        st = ctl.new_state(nao["q0"], pc.velocities(B), t=0.013)
        out, status = ctl.stand_step(st)
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (st, out, status)]

    before = whole_body()
    lip = to_device(ctl, d["lip"])
    ctl.mpc_box_step(lip, d["box"]); ctl.mpc_box_rollout(lip, d["shared"], 5); ctl.mpc_box_preview(lip, d["box"])
    after = whole_body()
    ctl.close()
    for a, b in zip(before, after):
        assert same_bits(a, b)


def test_refusals_enqueue_nothing(roll):
    from linearmpchumanoid_amd import capi
    ctl, L, d = roll["ctl"], capi.lib(), roll["d"]
    s, ns = ctl._stream(), roll["d"]["n"]
    lip, box = roll["lip0"].clone(), roll["box"]
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=ctl.device)
    rec, tr, pv = sent(B, 16), sent(3, B, 16), sent(B, capi.MPC_BOX_STRIDE)
    BAD = -2

    def refused(rc, text):
        return rc == BAD and L.lmh_last_error() == text.encode()

    for name, out in (("lmh_mpc_box_preview", pv), ("lmh_mpc_box_step", rec)):
        call = getattr(L, name)
        null = name + ": null device pointer"
        assert refused(call(ctl._h, None, _p(box), ns, B, _p(out), s), null) and refused(call(ctl._h, _p(lip), None, ns, B, _p(out), s), null)
        assert refused(call(ctl._h, _p(lip), _p(box), ns, B, None, s), null)
        assert refused(call(ctl._h, _p(lip), _p(box), ns - 1, B, _p(out), s), name + ": n_samples must be lmh_num_ref_samples")
        assert refused(call(ctl._h, _p(lip), _p(box), -1, B, _p(out), s), name + ": n_samples must be lmh_num_ref_samples")
        for sets in (0, 2, B + 1, -1):
            assert refused(call(ctl._h, _p(lip), _p(box), ns, sets, _p(out), s), name + ": n_sets must be 1 or n_instances")
        assert refused(call(None, _p(lip), _p(box), ns, B, _p(out), s), "null handle")
    call, name = L.lmh_mpc_box_rollout, "lmh_mpc_box_rollout"
    assert refused(call(ctl._h, None, _p(box), ns, B, 3, _p(tr), s), name + ": null device pointer")
    assert refused(call(ctl._h, _p(lip), None, ns, B, 3, _p(tr), s), name + ": null device pointer")
    assert refused(call(ctl._h, _p(lip), _p(box), ns + 1, B, 3, _p(tr), s), name + ": n_samples must be lmh_num_ref_samples")
    assert refused(call(ctl._h, _p(lip), _p(box), ns, 3, 3, _p(tr), s), name + ": n_sets must be 1 or n_instances")
    assert refused(call(ctl._h, _p(lip), _p(box), ns, B, -1, _p(tr), s), name + ": n_ticks must be >= 0")
    assert refused(call(None, _p(lip), _p(box), ns, B, 3, _p(tr), s), "null handle")
    assert call(ctl._h, _p(lip), _p(box), ns, B, 0, _p(tr), s) == 0  # the empty call
    assert ctl.mpc_box_rollout(lip, box, 0).shape == (0, B, 16)
    with pytest.raises(ValueError):
        ctl.mpc_box_step(lip, d["box"][:3])
    torch.cuda.synchronize()
    assert same_bits(lip, roll["lip0"]) and all(bool((b == -7).all()) for b in (rec, tr, pv))


def test_capture_of_the_three_calls_on_a_fresh_handle(nao):
    from linearmpchumanoid_amd import capi
    ctl, d = box_controller(16, 1e-2, nao["zcom"])
    L = capi.lib()
    lip0, box, shared = to_device(ctl, d["lip"]), to_device(ctl, d["box"]), to_device(ctl, d["shared"])
    lip = lip0.clone()
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=ctl.device)
    rec, tr, pv = sent(B, 16), sent(6, B, 16), sent(B, capi.MPC_BOX_STRIDE)
    ns = d["n"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcs = (L.lmh_mpc_box_step(ctl._h, _p(lip), _p(box), ns, B, _p(rec), ctl._stream()),
               L.lmh_mpc_box_rollout(ctl._h, _p(lip), _p(shared), ns, 1, 6, _p(tr), ctl._stream()),
               L.lmh_mpc_box_preview(ctl._h, _p(lip), _p(box), ns, B, _p(pv), ctl._stream()))
    assert rcs == (0, 0, 0)
    torch.cuda.synchronize()
    assert same_bits(lip, lip0) and all(bool((b == -7).all()) for b in (rec, tr, pv))      # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (rec, tr, pv, lip)]
    del g
    e_lip = lip0.clone()
    e_rec, e_tr = ctl.mpc_box_step(e_lip, box), ctl.mpc_box_rollout(e_lip, shared, 6)
    e_pv = ctl.mpc_box_preview(e_lip, box)
    torch.cuda.synchronize()
    ctl.close()
    for a, b in zip(got, (e_rec, e_tr, e_pv, e_lip)):
        assert same_bits(a, b)
