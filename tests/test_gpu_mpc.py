"""GPU tests of the public MPC calls (include/lmh.h: lmh_mpc_step, lmh_mpc_rollout, lmh_mpc_preview) and of Mpc3dLip::compute of the shim.

  step      bit for bit what lmh_eval leaves in out[72:78] / status at the same CoM state and clock, at the horizons where the window's
            code changes path, with per-robot walking plans, step lengths, LIPM heights and clocks, both clamps included; and against a
            longdouble statement within the derived step bound (mpc_cases.py), the zmp words bit for bit against numpy's x + D * u.
  rollout   bit for bit the host loop of steps it is defined as; splits; runs without a trajectory; flags a window that leaves the plan
            from that tick on; agrees with trajectories.lip_rollout within the accumulated bound.
  preview   residual, solution, predicted ZMP / CoM and header against longdouble references formed from the oracle's Px, Pu.
  the handle is untouched, refusals enqueue nothing, one captured graph of the three calls replays to the same bytes.
mpc_cases.py holds the cases and derives every bound; test_mpc.py has checked them on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mpc_cases as mc
import plan_draw
import preview_cases as pc
from oracle.pyoracle import Oracle
from helpers import ROOT, horizon_controller, horizon_time, same_bits, to_device

pytestmark = pytest.mark.gpu
B = mc.B_STEP
SIM_TIME = plan_draw.SIM_TIME
ZCOMS8 = np.array([0.24, 0.25, 0.255, 0.26, 0.262, 0.268, 0.272, 0.275])


@pytest.fixture(scope="module")
def nao():
    o = pc.make_oracle(16, "coupled")
    return dict(zcom=o.zcom, q0=o.robot()["q"].copy())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def walking_controller(N, mpc_dt, zcom, per_robot_zcom=True, **cfg):
    """B robots on walking plans of their own (lmh_gen_walk_batch), with their own step lengths and -- per_robot_zcom -- LIPM heights."""
    sp, xs = plan_draw.draw_walk_specs(B)
    ctl = horizon_controller(B, N, zcom, mpc_dt, mc.DT, **cfg)
    assert ctl.N == N
    ctl.gen_walk_batch(SIM_TIME, sp)
    ctl.set_xscale(xs)
    if per_robot_zcom:
        ctl.set_zcom(ZCOMS8)
    plans = [ctl.get_plan(i) for i in range(B)]
    return ctl, plans, xs


def host_loop(ctl, lip, n_ticks):
    """The definition of lmh_mpc_rollout: n_ticks launches of the step, the state moved on between them.  -> (lip, samples)."""
    lip = lip.clone()
    tr = []
    for _ in range(n_ticks):
        rec = ctl.mpc_step(lip)
        tr.append(rec)
        lip[:, 0], lip[:, 1], lip[:, 2], lip[:, 3] = rec[:, 0], rec[:, 1], rec[:, 3], rec[:, 4]
        lip[:, 4] = lip[:, 4] + ctl.cfg.mpc_dt
    return lip, torch.stack(tr)


# ------------------------------------------------------------------------------- 1. the step
@pytest.mark.parametrize("mpc_dt", mc.MPC_DTS)
@pytest.mark.parametrize("N", mc.H_STEP)
def test_step_is_the_evaluations_mpc_bit_for_bit(nao, N, mpc_dt):
    ctl, plans, _ = walking_controller(N, mpc_dt, nao["zcom"], warm_start=0)
    n = len(plans[0]["zmp_x"])
    t = mc.step_clocks(B, n, N, mpc_dt)
    st = ctl.new_state(nao["q0"], pc.velocities(B), t=t)
    out, status = ctl.stand_step(st)
    lip = ctl.new_lip(out[:, [66, 67]].cpu().numpy(), out[:, [69, 70]].cpu().numpy(), t)
    rec = ctl.mpc_step(lip)
    torch.cuda.synchronize()
    out, status, rec = out.cpu().numpy(), status.cpu().numpy(), rec.cpu().numpy()
    ctl.close()
    ks = [mc.k_of(ti, mpc_dt) for ti in t]
    assert ks[0] == -3 and ks[1] + N == n - 1 + mc.PAST_END
    f = ctl.split_mpc(rec)
    assert same_bits(np.ascontiguousarray(rec[:, 0:6]), np.ascontiguousarray(out[:, 72:78]))
    assert list(f["k"]) == list(status[:, 0]) == ks
    assert list(f["flags"] & 4) == list(status[:, 2] & 4) and list(f["flags"][:2] & 4) == [4, 4] and not (f["flags"][2:] & 4).any()
    assert same_bits(np.ascontiguousarray(rec[:, 8:13]), lip.cpu().numpy()[:, 0:5]) and (rec[:, 15] == 0).all()
    assert len({tuple(p["zmp_x"]) for p in plans}) == B             # every robot read a plan of its own


@pytest.mark.parametrize("mpc_dt", mc.MPC_DTS)
@pytest.mark.parametrize("N", mc.H_STEP)
def test_step_against_numpy(nao, N, mpc_dt):
    ctl, plans, xs = walking_controller(N, mpc_dt, nao["zcom"], per_robot_zcom=False)
    K = ctl.mpc_gain()
    Px0, Px1 = mc.px_closed(N, mpc_dt)
    n = len(plans[0]["zmp_x"])
    rng = np.random.default_rng(20261020 + N)
    lipn = np.zeros((B, 8))
    lipn[:, 0:4] = rng.uniform(-1, 1, (B, 4)) * np.array([0.03, 0.2, 0.03, 0.2])
    lipn[:, 4] = mc.step_clocks(B, n, N, mpc_dt)
    rec = ctl.mpc_step(to_device(ctl, lipn))
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    ctl.close()
    D = -np.float64(nao["zcom"]) / np.float64(mc.GRAVITY)
    worst = 0.0
    for i in range(B):
        zx, zy = plans[i]["zmp_x"], plans[i]["zmp_y"]
        k, _, tol = mc.step_terms(K, Px0, Px1, zx, zy, lipn[i], mpc_dt, xs[i])
        ref = mc.step_reference(K, Px0, Px1, zx, zy, lipn[i], mpc_dt, xs[i])
        worst = max(worst, float((np.abs(rec[i, 0:6] - ref).reshape(2, 3) / tol).max()))
        assert rec[i, 13] == k and rec[i, 14] == (4 if (k < 0 or k + N >= n) else 0)
        zmp = np.array([lipn[i, 0] + D * rec[i, 2], lipn[i, 2] + D * rec[i, 5]])
        assert same_bits(np.ascontiguousarray(rec[i, 6:8]), zmp), (rec[i, 6:8], zmp)
    print(f"\nstep N = {N}, mpc_dt = {mpc_dt}: worst error {worst:.3f} step bounds")
    assert worst <= 1.0


# ------------------------------------------------------------------------------- 2. the rollout
@pytest.fixture(scope="module")
def roll(nao):
    """N = 32 at 10 ms on per-robot walking plans; robot 0 starts where its window leaves the plan after 20 ticks.  The host loop of 40
    steps is computed once and shared."""
    N, mpc_dt = 32, 1e-2
    ctl, plans, xs = walking_controller(N, mpc_dt, nao["zcom"])
    n = len(plans[0]["zmp_x"])
    rng = np.random.default_rng(20261021)
    lipn = np.zeros((B, 8))
    lipn[:, 0:4] = rng.uniform(-1, 1, (B, 4)) * np.array([0.02, 0.1, 0.02, 0.1])
    lipn[:, 4] = rng.integers(0, 30, B) * mpc_dt + 0.004
    lipn[0, 4] = (n - N - 20) * mpc_dt + 0.004
    lipn[:, 5:8] = 7.0                                              # the pads of the state are the caller's
    lip0 = to_device(ctl, lipn)
    end, tr = host_loop(ctl, lip0, 40)
    torch.cuda.synchronize()
    yield dict(ctl=ctl, plans=plans, xs=xs, lip0=lip0, lipn=lipn, end=end, tr=tr, N=N, mpc_dt=mpc_dt, n=n)
    ctl.close()


def test_rollout_is_the_host_loop_of_steps(roll):
    ctl = roll["ctl"]
    lip = roll["lip0"].clone()
    tr = torch.full((40, B, 16), -7.0, dtype=torch.float64, device=ctl.device)
    assert ctl.mpc_rollout(lip, 40, traj=tr) is tr
    assert same_bits(lip, roll["end"]) and same_bits(tr, roll["tr"])
    assert bool((tr[:, :, 15] == 0).all()) and bool((lip[:, 5:8] == 7.0).all())
    a = roll["lip0"].clone()
    ta, tb = ctl.mpc_rollout(a, 17), ctl.mpc_rollout(a, 23)
    assert same_bits(a, roll["end"]) and same_bits(torch.cat([ta, tb]), roll["tr"])
    quiet = roll["lip0"].clone()
    assert ctl.mpc_rollout(quiet, 40, traj=False) is None
    assert same_bits(quiet, roll["end"])


def test_rollout_plans_step_at_different_ticks_and_the_flag_starts_on_time(roll):
    tr, N, n, mpc_dt = roll["tr"].cpu().numpy(), roll["N"], roll["n"], roll["mpc_dt"]
    first_step = [int(np.flatnonzero(np.abs(p["zmp_y"]) > 0)[0]) for p in roll["plans"]]
    assert len(set(first_step)) >= B // 2, first_step               # the robots' ZMP references step at different samples
    t = roll["lipn"][:, 4].copy()
    for j in range(40):                                            # k on the accumulated clock, flag from the tick the window leaves
        ks = np.array([mc.k_of(ti, mpc_dt) for ti in t])
        assert list(tr[j, :, 13]) == list(ks.astype(np.float64)) and same_bits(np.ascontiguousarray(tr[j, :, 12]), t)
        assert list(tr[j, :, 14]) == [4.0 if (k < 0 or k + N >= n) else 0.0 for k in ks]
        t = t + mpc_dt
    flagged = tr[:, 0, 14] == 4
    assert not flagged[:20].any() and flagged[20:].all() and not (tr[:, 1:, 14] != 0).any()


def test_rollout_against_lip_rollout(roll):
    from linearmpchumanoid_amd.trajectories import lip_rollout
    N, mpc_dt = roll["N"], roll["mpc_dt"]
    Px0, Px1 = mc.px_closed(N, mpc_dt)
    worst = 0.0
    # a handle whose gain row can be read back (lmh_get_mpc_gain reports robot 0's): one LIPM height for all, plans and step lengths per robot
    ctl2, plans, xs = walking_controller(N, mpc_dt, float(ZCOMS8[3]), per_robot_zcom=False)
    K = ctl2.mpc_gain()
    lip = to_device(ctl2, roll["lipn"])
    got = ctl2.mpc_rollout(lip, 40)
    torch.cuda.synchronize()
    got, lip = got.cpu().numpy(), lip.cpu().numpy()
    ctl2.close()
    for i in range(B):
        zx, zy = plans[i]["zmp_x"], plans[i]["zmp_y"]
        end, ref = lip_rollout(K, Px0, Px1, zx, zy, roll["lipn"][i], 40, mpc_dt, ZCOMS8[3], xscale=xs[i])
        tol = mc.accumulated_bounds(K, Px0, Px1, zx, zy, ref, mpc_dt, xs[i])
        worst = max(worst, float((np.abs(got[:, i, 0:6] - ref[:, 0:6]).reshape(40, 2, 3) / tol).max()))
        assert same_bits(np.ascontiguousarray(got[:, i, 12:15]), np.ascontiguousarray(ref[:, 12:15]))
        assert np.abs(lip[i, 0:4] - end[0:4]).max() <= tol[-1, :, :2].max() and lip[i, 4] == end[4]
    print(f"\nrollout against lip_rollout, 40 ticks: worst error {worst:.3f} accumulated bounds")
    assert worst <= 1.0


# ------------------------------------------------------------------------------- 3. the preview
@pytest.mark.parametrize("N", mc.H_PREVIEW)
def test_preview_against_longdouble(nao, N):
    from linearmpchumanoid_amd import capi
    mpc_dt, n = 1e-2, 150
    zcoms = np.repeat(np.array(pc.ZCOMS), 2)                       # robots 2 i, 2 i + 1: z_com i with an inside and a clamped window
    Bp = len(zcoms)
    xs = np.linspace(0.6, 1.4, Bp)
    ctl = horizon_controller(Bp, N, nao["zcom"], mpc_dt, mc.DT)
    zx, zy, ph = pc.zmp_arrays(n)
    ctl.set_refs(zx, zy, ph)
    ctl.set_zcom(zcoms)
    ctl.set_xscale(xs)
    lipn = mc.preview_lips(mpc_dt, n, N, pc.ZCOMS)
    lip = to_device(ctl, lipn)
    pv, step = ctl.mpc_preview(lip), ctl.mpc_step(lip)
    torch.cuda.synchronize()
    pv, step = pv.cpu().numpy(), step.cpu().numpy()
    ctl.close()
    f = ctl.split_preview(pv, N)
    worst = dict(a=0.0, b=0.0, c=0.0, d=0.0)
    mats = {}
    for z in pc.ZCOMS:                                             # Px, Pu of the reference's own set-up at this height (Oracle(dt = mpc_dt), set_zcom)
        o = Oracle(sim_time=1.0, dt=mpc_dt, horizon_time=horizon_time(N, mpc_dt), do_ik=False)
        o.set_zcom(z)
        assert o.horizon == N
        mats[z] = o.mpc_mats()
    cond_max = 0.0
    for i in range(Bp):
        Px, Pu = mats[zcoms[i]]
        k = mc.k_of(lipn[i, 4], mpc_dt)
        clamped = k + N >= n
        assert clamped == bool(i % 2)
        assert (f["k"][i], f["flags"][i], f["N"][i]) == (k, capi.FLAG_ZMP_RANGE if clamped else 0, N) and (pv[i, 3:8] == 0).all()
        assert not f["flags"][i] & capi.FLAG_NOT_SPD
        for name, (off, extra) in capi.MPC_PREVIEW_ARRAYS.items():
            assert (pv[i, off + N + extra:off + capi.MPC_PREVIEW_ARRAY] == 0).all(), name
            assert np.isfinite(pv[i, off:off + N + extra]).all(), name
        for ax, (z, s, nm) in enumerate(((zx, xs[i], "x"), (zy, 1.0, "y"))):
            x2 = lipn[i, 2 * ax:2 * ax + 2]
            U, Z, Cc, Cv = f["U_" + nm][i], f["Z_" + nm][i], f["C_" + nm][i], f["Cv_" + nm][i]
            H, g = mc.preview_system(Px, Pu, x2, s * pc.window(z, k, N))
            bound_a = mc.residual_bound(H, U, g)
            worst["a"] = max(worst["a"], mc.residual(H, U, g) / bound_a)
            cond = mc.cond_inf(H)
            cond_max = max(cond_max, cond)
            bound_b = cond * bound_a / mc.inf_norm(H)
            U_ref = mc.chol_solve_ld(H, -g)
            worst["b"] = max(worst["b"], float(np.abs(U - U_ref).max()) / bound_b)
            Zr, Za, cr, ca = mc.predicted(Px, Pu, x2, U, mpc_dt)
            worst["c"] = max(worst["c"], float((np.abs(Z - Zr) / mc.sum_bound(N + 1, Za)).max()))
            got = np.stack([Cc, Cv], axis=1).astype(mc.LD)
            assert same_bits(np.ascontiguousarray(got[0].astype(np.float64)), np.ascontiguousarray(x2))       # c_0 = x_k
            worst["c"] = max(worst["c"], float((np.abs(got[1:] - cr[1:]) / mc.sum_bound(N + 1, ca[1:])).max()))
            sw = step[i, 3 * ax:3 * ax + 3]                         # (d): the step is the preview's first move
            worst["d"] = max(worst["d"], abs(U[0] - sw[2]) / bound_b, abs(Cc[1] - sw[0]) / bound_b, abs(Cv[1] - sw[1]) / bound_b)
    print(f"\npreview N = {N}: residual {worst['a']:.3f} of (a), |U - U_ref| {worst['b']:.3g} of (b), Z / CoM {worst['c']:.3f} of (c), "
          f"against the step {worst['d']:.3g} of (b); cond_inf(H) up to {cond_max:.1f}")
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------- 4. the handle, refusals, capture
def test_the_handle_is_untouched(nao):
    def whole_body(ctl):
        st = ctl.new_state(nao["q0"], pc.velocities(B), t=0.013)
        out, status = ctl.stand_step(st)
        out2, status2, log = ctl.rollout(st, 20, log=True)
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (st, out, status, out2, status2, log)]

    ctl, _, _ = walking_controller(32, 1e-2, nao["zcom"])
    before = whole_body(ctl)
    lip = ctl.new_lip((0.01, -0.01), (0.05, 0.02), t=0.3)
    ctl.mpc_step(lip); ctl.mpc_rollout(lip, 25); ctl.mpc_preview(lip)
    after = whole_body(ctl)
    ctl.close()
    for a, b in zip(before, after):
        assert same_bits(a, b)


def test_refusals_and_the_empty_call(roll):
    from linearmpchumanoid_amd import capi
    ctl, L = roll["ctl"], capi.lib()
    s = ctl._stream()
    lip = roll["lip0"].clone()
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=ctl.device)
    rec, tr, pv = sent(B, 16), sent(3, B, 16), sent(B, capi.MPC_PREVIEW_STRIDE)
    BAD = -2
    assert L.lmh_mpc_step(ctl._h, None, _p(rec), s) == BAD and L.lmh_mpc_step(ctl._h, _p(lip), None, s) == BAD
    assert b"lmh_mpc_step" in L.lmh_last_error()
    assert L.lmh_mpc_rollout(ctl._h, None, 3, _p(tr), s) == BAD and L.lmh_mpc_rollout(ctl._h, _p(lip), -1, _p(tr), s) == BAD
    assert b"lmh_mpc_rollout" in L.lmh_last_error()
    assert L.lmh_mpc_preview(ctl._h, None, _p(pv), s) == BAD and L.lmh_mpc_preview(ctl._h, _p(lip), None, s) == BAD
    assert L.lmh_mpc_step(None, _p(lip), _p(rec), s) == BAD
    assert L.lmh_mpc_rollout(ctl._h, _p(lip), 0, _p(tr), s) == 0    # the empty call
    assert ctl.mpc_rollout(lip, 0).shape == (0, B, 16)
    torch.cuda.synchronize()
    assert same_bits(lip, roll["lip0"]) and all(bool((b == -7).all()) for b in (rec, tr, pv))


def test_capture_of_the_three_calls_on_a_fresh_handle(nao):
    from linearmpchumanoid_amd import capi
    ctl, _, _ = walking_controller(32, 1e-2, nao["zcom"])
    L = capi.lib()
    lip0 = ctl.new_lip((0.01, -0.01), (0.05, 0.02), t=np.linspace(0.0, 0.5, B))
    lip = lip0.clone()
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=ctl.device)
    rec, tr, pv = sent(B, 16), sent(12, B, 16), sent(B, capi.MPC_PREVIEW_STRIDE)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcs = (L.lmh_mpc_step(ctl._h, _p(lip), _p(rec), ctl._stream()), L.lmh_mpc_rollout(ctl._h, _p(lip), 12, _p(tr), ctl._stream()),
               L.lmh_mpc_preview(ctl._h, _p(lip), _p(pv), ctl._stream()))
    assert rcs == (0, 0, 0)
    torch.cuda.synchronize()
    assert same_bits(lip, lip0) and all(bool((b == -7).all()) for b in (rec, tr, pv))      # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (rec, tr, pv, lip)]
    del g
    e_lip = lip0.clone()
    e_rec, e_tr = ctl.mpc_step(e_lip), ctl.mpc_rollout(e_lip, 12)
    e_pv = ctl.mpc_preview(e_lip)
    torch.cuda.synchronize()
    ctl.close()
    for a, b in zip(got, (e_rec, e_tr, e_pv, e_lip)):
        assert same_bits(a, b)


# ------------------------------------------------------------------------------- 5. the shim
DRIVER = r"""
#include <cstdio>
#include "linearMpcHumanoid/controller/mpcLinearPendulum.hpp"
int main()
{
    const int n = %(n)d;
    Eigen::VectorXd zx(n), zy(n);
    for (int j = 0; j < n; j++) { zx(j) = 0.02 * j - 0.001 * j * j; zy(j) = 0.05 - 0.003 * j; }
    Mpc3dLip mpc(%(dt)r, %(th)r, %(zcom)r, %(alpha)r, %(beta)r);
    Mpc3dLip held = mpc;                                           // a copy made before the first compute stays a plain parameter set
    Eigen::Vector2d pos, vel;
    pos << 0.0125, -0.0075;
    vel << 0.04, -0.03;
    const double ts[3] = {%(t0)r, %(t1)r, %(t0)r};
    for (int c = 0; c < 3; c++) {
        if (c == 2) for (int j = 0; j < n; j++) zy(j) = -zy(j);    // the arrays moved: the third call uploads them again
        mpc.compute(pos, vel, zx, zy, ts[c]);
        const Eigen::Vector3d x = mpc.getXRef(), y = mpc.getYRef();
        std::printf("REF %%a %%a %%a %%a %%a %%a\n", x(0), x(1), x(2), y(0), y(1), y(2));
    }
    return held.getXRef()(0) == 0.0 ? 0 : 1;
}
"""


def test_shim_compute_is_the_step(tmp_path):
    from linearmpchumanoid_amd import build as b
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    shim_so, _ = b.build_shim()
    case = dict(n=90, dt=0.01, th=0.3, zcom=0.255, alpha=2e-3, beta=0.9, t0=0.123, t1=0.687)
    src = tmp_path / "mpc_driver.cpp"
    src.write_text(DRIVER % case)
    exe = tmp_path / "mpc_driver"
    libdir = os.path.dirname(shim_so)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + b.SHIM_DIR, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-llmh_shim", "-llmh_hip", "-Wl,-rpath," + libdir])
    lines = [ln.split()[1:] for ln in subprocess.check_output([str(exe)], timeout=120).decode().splitlines() if ln.startswith("REF")]
    got = np.array([[float.fromhex(w) for w in ln] for ln in lines])
    assert got.shape == (3, 6)
    j = np.arange(case["n"], dtype=np.float64)
    zx, zy = 0.02 * j - 0.001 * j * j, 0.05 - 0.003 * j
    ctl = BatchedController(1, default_config(dt=case["dt"], mpc_dt=case["dt"], time_horizon=case["th"], z_com=case["zcom"],
                                              alpha=case["alpha"], beta=case["beta"]))
    assert ctl.N == 30
    want = []
    for c, t in enumerate((case["t0"], case["t1"], case["t0"])):
        ctl.set_refs(zx, -zy if c == 2 else zy)
        want.append(ctl.mpc_step(ctl.new_lip((0.0125, -0.0075), (0.04, -0.03), t)).cpu().numpy()[0, 0:6])
    ctl.close()
    assert same_bits(got, np.array(want))
    assert mc.k_of(case["t1"], case["dt"]) + 30 >= case["n"] and not same_bits(got[0], got[2])    # a clamped window and a new plan were among them
