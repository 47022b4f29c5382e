"""Cases, references and derived bounds of the box-constrained MPC calls (lmh_mpc_box_preview / _step / _rollout): test_mpc_box.py checks them
on the CPU against the numpy statement (trajectories.lip_box_preview), test_gpu_mpc_box.py holds the kernels to them.  Nothing here imports the
HIP library.

Cases: B = 8 robots at every (N, mpc_dt) of CASES on walking plans, step lengths and LIPM heights of their own (plan_draw's draw).  The robots
have roles, so that every horizon holds what the kernel can get wrong:
    0  front clamp (k = -3), a millimetre off its reference, the whole sole: no active bound
    1  window PAST_END samples past the plan's end (the back clamp), a few millimetres off
    2  3 cm and 0.2 m/s off sideways in a +-2 mm box (N <= 16: wholly in single support): every sample of the y axis active
    3  between its feet where it changes them without a double support (ds_time = 0): an upper, then a lower bound active in one window
    4  a stretch of +-inf rows (a flight phase) inside its window
    5-7  drawn: up to 3 cm and 0.2 m/s off, margins between the whole sole and +-2 mm
`shared` solves the same robots against ONE set of bounds (n_sets = 1), robot 5's at a small margin.

Bounds (EPS = 2^-52, n = N + 1, inf-norms; every one derived from the arithmetic, none from what the kernels return).  W is the working set
of the solution, S = Pu_W H^-1 Pu_W' its system, b_W its bounds:
  (a) stationarity   ||H U + g + Pu' lam||inf <= 8 n EPS (||H|| ||U|| + ||g|| + ||Pu'|| ||lam||): mpc_cases.residual_bound with the multiplier
                     term added -- the backward error of the Cholesky solve of H U = -(g + Pu' lam) and of forming its right-hand side.
  (b) multipliers    lam_W solves S lam = Z0_W - b_W.  The computed S carries the error of H^-1 applied through the factor, eS = cond(H) 8 n EPS
                     ||Pu_W|| ||H^-1|| ||Pu_W'||; the right-hand side carries that of U0 (mpc_cases (b)) through Pu and of the n-term sums of
                     Z0 (mpc_cases (c)), eR; the solve itself 8 n EPS (||S|| ||lam|| + ||rhs||).  Hence
                         ||dlam|| <= ||S^-1|| (eS ||lam|| + eR + 8 n EPS (||S|| ||lam|| + ||rhs||)).
                     The conditioning of S is in it through ||S^-1||: a plain term bound on the active rows is exceeded by numpy's own solve.
  (c) solution       ||dU|| <= cond(H) (a) / ||H|| + ||H^-1|| ||Pu'|| ||dlam||: mpc_cases (b) for the solve, plus what dlam moves.
  (d) predictions    Z at inactive samples and the CoM arrays, from the U returned: mpc_cases.sum_bound on their n-term sums.
The reference of (b) and (c) is the longdouble solution on the SAME working set (mpc_cases.chol_solve_ld).
"""
import functools

import numpy as np

import mpc_cases as mc
import plan_draw
from linearmpchumanoid_amd import trajectories as tj
from linearmpchumanoid_amd.capi import PHASE_FLIGHT

EPS, LD = mc.EPS, mc.LD
B = 8
CASES = ((1, 1e-2), (2, 1e-2), (16, 1e-2), (63, 1e-2), (64, 1e-2), (16, 1e-3))
ZCOMS8 = np.array([0.24, 0.25, 0.255, 0.26, 0.262, 0.268, 0.272, 0.275])
SIM_TIME = plan_draw.SIM_TIME
SEED = 20261101
STRICT = 1e-6
FLIGHT = (3, 9)                                                    # robot 4's +-inf rows: samples k + 3 .. k + 8 of its window (cut to it)
MARGINS = np.array([0.0, 0.015, 0.023, 0.02, 0.01, 0.0, 0.0, 0.0])  # robots 5-7: drawn
SHARED_MARGIN = 0.005


@functools.lru_cache(maxsize=None)
def draw(N, mpc_dt):
    """-> dict(plans (walk_plans), xs [B], zcoms [B], lip [B,8], box [B,4,n], shared [4,n], n)."""
    sp, xs = plan_draw.draw_walk_specs(B)
    sp["ds_time"][3] = 0.0                                         # robot 3 changes feet without a double support: its box jumps across the CoM
    plans = tj.walk_plans(SIM_TIME, mpc_dt, sp)
    n = plans["zmp_x"].shape[1]
    rng = np.random.default_rng(SEED + 97 * N + int(round(1e5 * mpc_dt)))
    margins = MARGINS.copy()
    margins[5:] = rng.choice([0.0, 0.01, 0.02, 0.023], 3)
    k = rng.integers(20, n - N - 30, B)
    t = (k + rng.uniform(0.1, 0.9, B)) * mpc_dt
    t[0] = -3.5 * mpc_dt
    t[1] = (n - 1 - N + mc.PAST_END + 0.5) * mpc_dt
    ph3 = plans["phase"][3].astype(np.int64)
    switch = int(np.flatnonzero((ph3[1:] != ph3[:-1]) & (ph3[1:] != 0) & (ph3[:-1] != 0))[0]) + 1    # robot 3's first change of feet
    t[3] = (switch - 1 + 0.5) * mpc_dt                              # ... is the second sample of its window
    if N <= 16:                                                    # robot 2's whole window inside its first single support
        t[2] = (int(np.flatnonzero(plans["phase"][2] != 0)[0]) + 1 + 0.5) * mpc_dt
    off = rng.uniform(-1, 1, (B, 4)) * np.array([0.03, 0.2, 0.03, 0.2])
    off[0] = [0.001, 0.005, -0.001, 0.004]
    off[1] = [0.004, 0.02, -0.003, 0.01]
    off[2] = [0.005, 0.0, 0.03, 0.2]
    off[3] = [-0.02, 0.15, 0.012, -0.18]
    off[4] = [0.01, -0.05, -0.01, 0.05]
    lip = np.zeros((B, 8))
    for i in range(B):
        k0 = int(np.clip(mc.k_of(t[i], mpc_dt), 0, n - 1))
        lip[i, 0:4] = off[i] + np.array([xs[i] * plans["zmp_x"][i, k0], 0.0, plans["zmp_y"][i, k0], 0.0])
        lip[i, 4] = t[i]
    lip[3, 2:4] = [0.004, -0.05]                                   # between its feet
    box_plans = {key: v.copy() for key, v in plans.items()}
    k4 = mc.k_of(t[4], mpc_dt)
    box_plans["phase"][4, k4 + min(FLIGHT[0], N):k4 + min(FLIGHT[1], N + 1)] = PHASE_FLIGHT
    box = tj.zmp_boxes(box_plans, xs, margin=margins)
    shared = tj.zmp_box({key: v[5] for key, v in plans.items()}, xs[5], margin=SHARED_MARGIN)
    for a in (lip, box, shared):
        a.setflags(write=False)
    return dict(plans=plans, xs=xs, zcoms=ZCOMS8, lip=lip, box=box, shared=shared, n=n, margins=margins)


@functools.lru_cache(maxsize=None)
def statement(N, mpc_dt, shared=False):
    """The numpy statement's solutions of draw(N, mpc_dt): a list of B lip_box_preview dicts (computed once, shared by the tests)."""
    d = draw(N, mpc_dt)
    return [tj.lip_box_preview(d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i], d["shared"] if shared else d["box"][i], d["lip"][i], N, mpc_dt,
                               d["zcoms"][i], mc.ALPHA, mc.BETA, mc.GRAVITY, d["xs"][i]) for i in range(B)]


def system(N, mpc_dt, i, ax, shared=False, box_shift=0):
    """Robot i, axis ax of draw(N, mpc_dt) in np.longdouble: dict(Px, Pu, H, g, p, lo, hi, x2, k).  box_shift: the window of the BOUNDS
    read that many samples late (the mistake the sensitivity test plants)."""
    d = draw(N, mpc_dt)
    Px, Pu = tj.lip_matrices(N, mpc_dt, d["zcoms"][i], mc.GRAVITY)
    z = (d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i])[ax]
    s = (d["xs"][i], 1.0)[ax]
    x2 = d["lip"][i, 2 * ax:2 * ax + 2]
    k = mc.k_of(d["lip"][i, 4], mpc_dt)
    idx = np.clip(k + np.arange(N + 1), 0, d["n"] - 1)
    H, g = mc.preview_system(Px, Pu, x2, s * z[idx])
    bx = d["shared"] if shared else d["box"][i]
    bidx = np.clip(k + box_shift + np.arange(N + 1), 0, d["n"] - 1)
    return dict(Px=Px, Pu=Pu, H=H, g=g, p=Px.astype(LD) @ x2.astype(LD), lo=bx[2 * ax, bidx], hi=bx[2 * ax + 1, bidx], x2=x2, k=k)


def solve_on_set_ld(sy, side):
    """The solution on a given working set (side [n]: -1 lower, +1 upper, 0 inactive) in np.longdouble -> (U, lam, Z)."""
    H, g, Pu = sy["H"], sy["g"], sy["Pu"].astype(LD)
    n = len(g)
    W = np.flatnonzero(side)
    lam = np.zeros(n, dtype=LD)
    U0 = mc.chol_solve_ld(H, -g)
    if len(W):
        b = np.where(side > 0, sy["hi"], sy["lo"]).astype(LD)
        Y = np.stack([mc.chol_solve_ld(H, Pu[w]) for w in W], axis=1)          # H^-1 Pu_W'
        S = Pu[W] @ Y
        lam[W] = mc.chol_solve_ld(S, (sy["p"] + Pu @ U0)[W] - b[W])
    U = mc.chol_solve_ld(H, -(g + Pu.T @ lam))
    return U, lam, sy["p"] + Pu @ U


def stationarity(sy, U, lam):
    """-> (||H U + g + Pu' lam||inf in longdouble, its bound (a))."""
    Ul, ll, Put = np.asarray(U, dtype=LD), np.asarray(lam, dtype=LD), sy["Pu"].T.astype(LD)
    res = float(np.abs(sy["H"] @ Ul + sy["g"] + Put @ ll).max())
    n = len(Ul)
    bound = 8.0 * n * EPS * (mc.inf_norm(sy["H"]) * mc.inf_norm(U) + mc.inf_norm(sy["g"]) + mc.inf_norm(sy["Pu"].T) * mc.inf_norm(lam))
    return res, bound


def solution_bounds(sy, side, U, lam):
    """-> (bound (b) on ||lam - lam_ld||inf, bound (c) on ||U - U_ld||inf) for a solution on the working set `side`."""
    H64, Pu = np.asarray(sy["H"], dtype=np.float64), sy["Pu"]
    n = H64.shape[0]
    Hinv = np.linalg.inv(H64)
    condH, nH, nHinv = mc.cond_inf(H64), mc.inf_norm(H64), mc.inf_norm(Hinv)
    _, bound_a = stationarity(sy, U, lam)
    W = np.flatnonzero(side)
    dlam = 0.0
    if len(W):
        S = Pu[W] @ Hinv @ Pu[W].T
        Sinv = mc.inf_norm(np.linalg.inv(S))
        U0 = -(Hinv @ np.asarray(sy["g"], dtype=np.float64))
        Z0a = np.abs(sy["Px"]) @ np.abs(sy["x2"]) + np.abs(Pu) @ np.abs(U0)
        b = np.where(side > 0, sy["hi"], sy["lo"])
        rhs = (np.asarray(sy["p"], dtype=np.float64) + Pu @ U0)[W] - b[W]
        eS = condH * 8.0 * n * EPS * mc.inf_norm(Pu[W]) * nHinv * mc.inf_norm(Pu[W].T)
        eU0 = condH * mc.residual_bound(H64, U0, np.asarray(sy["g"], dtype=np.float64)) / nH
        eR = mc.inf_norm(Pu[W]) * eU0 + float(mc.sum_bound(n, Z0a)[W].max())
        dlam = Sinv * (eS * mc.inf_norm(lam) + eR + 8.0 * n * EPS * (mc.inf_norm(S) * mc.inf_norm(lam) + mc.inf_norm(rhs)))
    dU = condH * bound_a / nH + nHinv * mc.inf_norm(Pu.T) * dlam
    return dlam, dU


def strictness(pv, ax):
    """The smallest of: an active multiplier over the largest one, an inactive slack over the box's width (inf where there is none)."""
    side, lam, Z, lo, hi = pv["side"][ax], pv["lam"][ax], pv["Z"][ax], pv["lo"][ax], pv["hi"][ax]
    m = np.inf
    if (side != 0).any():
        m = min(m, float(np.abs(lam[side != 0]).min() / np.abs(lam).max()))
    free = (side == 0) & np.isfinite(hi - lo)
    if free.any():
        m = min(m, float((np.minimum(Z - lo, hi - Z)[free] / (hi - lo)[free]).min()))
    return m


def check_against_statement(N, mpc_dt, i, ax, pv, U, lam, Z, C, Cv, shared=False):
    """One robot and axis of a computed solution against the bounds, on the working set `pv` (the numpy statement's) has.
    -> dict of ratios error / bound for a, b, c, d."""
    sy = system(N, mpc_dt, i, ax, shared)
    side = pv["side"][ax]
    res, bound_a = stationarity(sy, U, lam)
    bl, bu = solution_bounds(sy, side, U, lam)
    U_ld, lam_ld, _ = solve_on_set_ld(sy, side)
    r = dict(a=res / bound_a, c=float(np.abs(U - U_ld).max()) / bu)
    r["b"] = float(np.abs(lam - lam_ld).max()) / bl if (side != 0).any() else 0.0
    Zr, Za, cr, ca = mc.predicted(sy["Px"], sy["Pu"], sy["x2"], U, mpc_dt)
    free = side == 0
    d = 0.0
    if free.any():
        d = float((np.abs(Z - Zr) / mc.sum_bound(N + 1, Za))[free].max())
    got = np.stack([C, Cv], axis=1).astype(LD)
    d = max(d, float((np.abs(got[1:] - cr[1:]) / mc.sum_bound(N + 1, ca[1:])).max()))
    r["d"] = d
    return r
