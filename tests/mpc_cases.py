"""Cases, references and derived bounds of the public MPC calls (lmh_mpc_step / lmh_mpc_rollout / lmh_mpc_preview): test_mpc.py checks them on
the CPU, test_gpu_mpc.py holds the kernels to them.  Nothing here imports the HIP library.

Bounds (EPS = 2^-52; every one is derived from the arithmetic, none from what the kernels return):

  step      u = -((kp0 x + kp1 xdot) - xscale sum_j K_j z_j) is a sum of N + 1 products plus two products and two sums: with the sums K.Px0,
            K.Px1 of N + 1 terms themselves, every term carries at most N + 4 roundings of relative size EPS / 2, so
                |du| <= 4 (N + 4) EPS S,   S = |kp0 x| + |kp1 xdot| + xscale sum_j |K_j z_j|
            with a factor 8 to spare for the order of the sums.  The other words carry it through A = [1 dt; 0 1], B = [dt^2 / 2, dt]:
                |dx_next| <= 4 (N + 4) EPS (|x| + dt |xdot| + dt^2 / 2 S),   |dxdot_next| <= 4 (N + 4) EPS (|xdot| + dt S).
  rollout   the error e = (dx, dxdot) of a tick enters the next through x_next = A x + B u(x): componentwise
                e' <= G e + b,   G = |A| + |B| (|kp0| |kp1|),   b = the step bounds of that tick;
            accumulated_bounds() runs that recursion beside the numpy trajectory.
  preview   (a) ||H U + g||inf <= 8 n EPS (||H||inf ||U||inf + ||g||inf), n = N + 1: the backward error of a Cholesky solve (Higham, Accuracy
            and Stability, thm 10.4: (n + 1) u per triangular factor) plus the error of forming H and g from Pu in fp64 (n-term sums);
            (b) ||U - U_ref||inf <= cond_inf(H) * (a) / ||H||inf;
            (c) an n-term fp64 sum against its exact value: 4 n EPS times the sum of the absolute values of its terms.
"""
import numpy as np

import preview_cases as pc

EPS = float(np.finfo(np.float64).eps)
GRAVITY = 9.81
ALPHA, BETA = 1e-3, 1.0                     # lmh_config_default (mpcLinearPendulum.hpp:46-48)
H_STEP = (1, 2, 45, 46, 63, 64)             # 45 | 46: gain record on chip | in memory for lmh_eval; 64: the second trip of the window loop
H_PREVIEW = (1, 16, 45, 64)
H_CHOLESKY = (1, 16, 50, 64)
SENSITIVITY = 1e3
DT = 1e-3                                   # control step of the handles (only lmh_eval's rollouts use it)
MPC_DTS = (1e-3, 1e-2)                      # mpc_dt = dt and mpc_dt = 10 dt
B_STEP = 8
PAST_END = 5
LD = np.longdouble


def px_closed(N, mpc_dt):
    """The two columns of Px = [C A^j] in closed form: 1 and j mpc_dt."""
    j = np.arange(N + 1, dtype=np.float64)
    return np.ones(N + 1), j * np.float64(mpc_dt)


def k_of(t, mpc_dt):
    from linearmpchumanoid_amd.trajectories import preview_index
    return preview_index(t, mpc_dt)


def window(z, k, N):
    return pc.window(z, k, N)


def step_terms(K, Px0, Px1, zx, zy, lip, mpc_dt, xscale=1.0):
    """-> k, S [2] (the size of the terms of u per axis), tol [2,3] (the step bounds of x_next, xdot_next, u per axis)."""
    N = len(K) - 1
    dt = float(mpc_dt)
    k = k_of(lip[4], mpc_dt)
    kp0, kp1 = abs(K @ Px0), abs(K @ Px1)
    S, tol = np.zeros(2), np.zeros((2, 3))
    c = 4.0 * (N + 4) * EPS
    for ax, (z, s) in enumerate(((zx, float(xscale)), (zy, 1.0))):
        x, xd = abs(lip[2 * ax]), abs(lip[2 * ax + 1])
        S[ax] = kp0 * x + kp1 * xd + abs(s) * (np.abs(K) @ np.abs(window(z, k, N)))
        tol[ax] = c * np.array([x + dt * xd + 0.5 * dt * dt * S[ax], xd + dt * S[ax], S[ax]])
    return k, S, tol


def step_reference(K, Px0, Px1, zx, zy, lip, mpc_dt, xscale=1.0, shift=0, drop_last=False):
    """(x_ref | y_ref) [6] of one step in np.longdouble (rounded to fp64 at the end).  shift / drop_last state the two mistakes the
    sensitivity test plants: the window one sample late, the window without its last term."""
    N = len(K) - 1
    k = k_of(lip[4], mpc_dt)
    Kl, dt = K.astype(LD), LD(mpc_dt)
    out = np.zeros(6, dtype=LD)
    for ax, (z, s) in enumerate(((zx, xscale), (zy, 1.0))):
        x, xd = LD(lip[2 * ax]), LD(lip[2 * ax + 1])
        w = window(z, k + shift, N).astype(LD)
        if drop_last:
            w[N] = 0
        u = -((Kl @ Px0.astype(LD)) * x + (Kl @ Px1.astype(LD)) * xd - LD(s) * (Kl @ w))
        out[3 * ax:3 * ax + 3] = [x + dt * xd + dt * dt / 2 * u, xd + dt * u, u]
    return out.astype(np.float64)


def hand_rollout(K, Px0, Px1, zx, zy, lip, n_ticks, mpc_dt, z_com, xscale=1.0):
    """The rollout's definition written out term by term in plain Python floats, for trajectories.lip_rollout to be held against: the
    gain sums and the window sum through numpy's dot (the one operation whose order numpy owns), everything else one operation at a time."""
    N, n = len(K) - 1, len(zx)
    dt = float(mpc_dt)
    D = -float(z_com) / GRAVITY
    kp0, kp1 = float(K @ Px0), float(K @ Px1)
    x, xd, y, yd, t = (float(v) for v in lip[:5])
    rows = []
    for _ in range(n_ticks):
        k = int(t / dt)
        idx = [min(max(k + j, 0), n - 1) for j in range(N + 1)]
        wx, wy = float(K @ zx[idx]), float(K @ zy[idx])
        ux = -((kp0 * x + kp1 * xd) - float(xscale) * wx)
        uy = -((kp0 * y + kp1 * yd) - wy)
        xn, xdn = x + dt * xd + (dt * dt) / 2 * ux, xd + dt * ux
        yn, ydn = y + dt * yd + (dt * dt) / 2 * uy, yd + dt * uy
        flags = 4 if (k < 0 or k + N >= n) else 0
        rows.append([xn, xdn, ux, yn, ydn, uy, x + D * ux, y + D * uy, x, xd, y, yd, t, float(k), float(flags), 0.0])
        x, xd, y, yd, t = xn, xdn, yn, ydn, t + dt
    return np.array([x, xd, y, yd, t, 0.0, 0.0, 0.0]), np.array(rows).reshape(n_ticks, 16)


def accumulated_bounds(K, Px0, Px1, zx, zy, traj, mpc_dt, xscale=1.0):
    """Per tick the bounds [n_ticks,2,3] on (x_next, xdot_next, u) of a rollout against the exact trajectory from the same start: the step
    bounds of every tick fed through e' <= G e + b (module docstring), along the samples `traj` [n_ticks,16]."""
    dt = float(mpc_dt)
    kp = np.array([abs(K @ Px0), abs(K @ Px1)])
    G = np.array([[1.0, dt], [0.0, 1.0]]) + np.outer([0.5 * dt * dt, dt], kp)
    e = np.zeros((2, 2))
    out = np.zeros((len(traj), 2, 3))
    for i, rec in enumerate(traj):
        _, _, tol = step_terms(K, Px0, Px1, zx, zy, rec[8:13], mpc_dt, xscale)
        for ax in range(2):
            out[i, ax, 2] = kp @ e[ax] + tol[ax, 2]
            e[ax] = G @ e[ax] + tol[ax, :2]
            out[i, ax, :2] = e[ax]
    return out


# ------------------------------------------------------------------------------- the preview's linear system
def preview_system(Px, Pu, x2, zwin, alpha=ALPHA, beta=BETA):
    """H = alpha I + beta Pu'Pu and g = beta Pu'(Px x - z) in np.longdouble from fp64 Px [n,2], Pu [n,n] (Oracle.mpc_mats)."""
    Pul, Pxl = Pu.astype(LD), Px.astype(LD)
    n = Pu.shape[0]
    H = LD(alpha) * np.eye(n, dtype=LD) + LD(beta) * (Pul.T @ Pul)
    g = LD(beta) * (Pul.T @ (Pxl @ np.asarray(x2, dtype=LD) - np.asarray(zwin, dtype=LD)))
    return H, g


def chol_solve_ld(H, b):
    """H^-1 b by a Cholesky factorisation written out in np.longdouble (numpy's LAPACK routines stop at fp64)."""
    n = H.shape[0]
    L = np.zeros_like(H)
    for j in range(n):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def inf_norm(M):
    M = np.asarray(M)
    return float(np.abs(M).sum(axis=1).max()) if M.ndim == 2 else float(np.abs(M).max())


def residual_bound(H, U, g):
    """(a): 8 n EPS (||H||inf ||U||inf + ||g||inf)."""
    return 8.0 * H.shape[0] * EPS * (inf_norm(H) * inf_norm(U) + inf_norm(g))


def residual(H, U, g):
    return float(np.abs(H @ np.asarray(U, dtype=LD) + g).max())


def cond_inf(H):
    H64 = np.asarray(H, dtype=np.float64)
    return inf_norm(H64) * inf_norm(np.linalg.inv(H64))


def predicted(Px, Pu, x2, U, mpc_dt):
    """From a given U in np.longdouble: Z = Px x + Pu U [n], the CoM states c [n+1,2] with c_0 = x, c_{j+1} = A c_j + B u_j, and for
    each the same expression evaluated with absolute values (the size of its terms)."""
    Ul, x = np.asarray(U, dtype=LD), np.asarray(x2, dtype=LD)
    Z = Px.astype(LD) @ x + Pu.astype(LD) @ Ul
    Za = np.abs(Px).astype(LD) @ np.abs(x) + np.abs(Pu).astype(LD) @ np.abs(Ul)
    dt = LD(mpc_dt)
    A, Bv = np.array([[1, dt], [0, 1]], dtype=LD), np.array([dt * dt / 2, dt], dtype=LD)
    n = len(Ul)
    c, ca = np.zeros((n + 1, 2), dtype=LD), np.zeros((n + 1, 2), dtype=LD)
    c[0], ca[0] = x, np.abs(x)
    for j in range(n):
        c[j + 1] = A @ c[j] + Bv * Ul[j]
        ca[j + 1] = A @ ca[j] + Bv * abs(Ul[j])
    return Z, Za, c, ca


def sum_bound(n, absolute):
    """(c): 4 n EPS times the terms' absolute sum."""
    return 4.0 * n * EPS * np.asarray(absolute, dtype=np.float64)


def preview_lips(mpc_dt, n_samples, N, zcoms):
    """LIP states [2 len(zcoms), 8] for the preview tests: per z_com one state whose window lies inside the arrays and one whose window
    runs PAST_END samples past their end; CoM and velocity differ per robot."""
    rows = []
    for i, _ in enumerate(zcoms):
        for clamped in (False, True):
            k = (n_samples - 1 - N + PAST_END) if clamped else 7 + 3 * i
            rows.append([0.01 + 0.003 * i, 0.05 - 0.02 * i, -0.008 + 0.004 * i, 0.03 * (i - 1), (k + 0.5) * mpc_dt, 0, 0, 0])
    return np.array(rows, dtype=np.float64)


def step_clocks(B, n_samples, N, mpc_dt, seed=20261019):
    """Per-robot clocks for the step tests: robot 0 before the arrays (k = -3: the front clamp), robot 1 with its window PAST_END samples
    past the end, the others drawn inside."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, n_samples - N - 1, B).astype(np.float64)
    t = (k + rng.uniform(0.1, 0.9, B)) * mpc_dt
    t[0] = -3.5 * mpc_dt
    t[1] = (n_samples - 1 - N + PAST_END + 0.5) * mpc_dt
    return t
