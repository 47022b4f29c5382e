"""Cases of the preview-window tests (test_preview_cases.py on the CPU, test_gpu_preview_window.py on the GPU).

The MPC step is u = -K (Px x - z[k .. k + N]) per axis: a gain row of N + 1 entries against a window of the ZMP reference.  With a
constant reference the window sum is z * sum(K), and a window that is shifted by a sample or that drops its last term returns the same
number; the arrays here differ at every sample, and sensitivity() measures, from the oracle's gain row and the arrays alone, by how
much those two mistakes would move u -- the CPU test asserts that it is at least 1e3 times the tolerance the GPU test compares with.

Horizons: 45 is the last N whose gain record is kept on chip (it then ends where the next LDS block starts), 46 and 47 the first two read
from memory, 64 the only one whose window sum takes a second trip of the 64-lane loop; 1 and 2 the shortest, 15 / 17 and 63 either side
of the sizes the rest of the suite runs (16, 64)."""
import numpy as np

from helpers import horizon_time, perturbed_velocities

H = (1, 2, 15, 17, 44, 45, 46, 47, 63, 64)
H_ROLLOUT = (1, 45, 46, 63, 64)
H_ZCOM = (45, 46, 64)
H_CLAMP = (17, 46, 64)
ZCOMS = (0.24, 0.26, 0.275)
DT = 1e-3
# name -> MPC sample time, number of reference samples, clock of the single evaluation
MODES = {"coupled": dict(mpc_dt=1e-3, n=700, t=0.0123), "decoupled": dict(mpc_dt=1e-2, n=150, t=0.457)}
ROLLOUT_TICKS = 25
ZCOM_TICKS = 12
TOL_WINDOW = 1e-11               # the suite's stage-parity tolerance for fp64 sums of this length (test_stage_parity_single_evaluation)
SENSITIVITY = 1e3                # a dropped term or a shifted window must move u by this many tolerances
B_EVAL = 3
SEED = 20261018
T_FRONT = -0.0035                # the front clamp: k = int(t / mpc_dt) = -3 coupled, 0 decoupled (the cast truncates towards zero)
PAST_END = 5                     # the end clamp: k + N runs this many samples past the last one


def zmp_arrays(n):
    """ZMP references that differ at every sample, phase all double support."""
    j = np.arange(n, dtype=np.float64)
    zx = 0.02 * np.sin(0.37 * j) + 0.005 * np.cos(1.13 * j + 0.3)
    zy = 0.015 * np.sin(0.53 * j + 1.0) + 0.004 * np.cos(0.91 * j)
    return zx, zy, np.zeros(n, dtype=np.uint8)


def velocities(B, seed=SEED, base=0.05):
    """perturbed_velocities with the base's horizontal velocity scaled to +-base m/s (joints N(0, 0.05^2) rad/s)."""
    v = perturbed_velocities(B, seed=seed)
    v[:, 0:2] *= base / 0.3
    return v


def pushed_velocities(B, seed=SEED + 500):
    """The same with the base moving at the 0.15 m/s of test_gpu_cone_routes's pushes, in a drawn direction: bounds of the contact QP
    become active, so a warm-started rollout keeps a K_f^-1 block (the LDS block that starts where the N = 45 gain record ends)."""
    v = velocities(B, seed=seed)
    for i in range(B):
        a = np.random.default_rng(seed + 77 + i).uniform(0.0, 2.0 * np.pi)
        v[i, 0:2] = 0.15 * np.array([np.cos(a), np.sin(a)])
    return v


def make_oracle(N, mode, zcom=None, pad_front=0, pad_back=0, n=None):
    """Oracle at horizon N on the arrays of zmp_arrays(n), optionally padded by repeating the first / last sample (what the kernel's
    clamped window reads); zcom re-initialises the LIPM height."""
    from oracle.pyoracle import Oracle
    m = MODES[mode]
    o = Oracle(sim_time=1.0, dt=m["mpc_dt"], horizon_time=horizon_time(N, m["mpc_dt"]), do_ik=True)
    assert o.horizon == N
    if zcom is not None:
        o.set_zcom(zcom)
    zx, zy, ph = zmp_arrays(m["n"] if n is None else n)
    zx = np.concatenate([np.full(pad_front, zx[0]), zx, np.full(pad_back, zx[-1])])
    zy = np.concatenate([np.full(pad_front, zy[0]), zy, np.full(pad_back, zy[-1])])
    o.set_refs(zx, zy, np.zeros(len(zx), dtype=np.uint8))
    return o


def window(z, k, N):
    """z[k .. k + N] with every index pinned to the array (the kernel's clamp)."""
    return np.asarray(z)[np.clip(k + np.arange(N + 1), 0, len(z) - 1)]


def scales(K, Px, zx, zy, k, com, com_vel, mpc_dt):
    """Per axis the size S of the terms of u = -K (Px x - z) and the tolerances of (x_ref, y_ref) = (A x + B u, u) that follow from it:
    S = sum|K_i||z_{k+i}| + |sum K Px0||c| + |sum K Px1||cdot|; position and velocity carry it through A = [1 dt; 0 1], B = [dt^2/2, dt].
    -> S [2], tol [2,3] (TOL_WINDOW times the sizes)."""
    N = len(K) - 1
    S, tol = np.zeros(2), np.zeros((2, 3))
    for ax, z in enumerate((zx, zy)):
        c, cd = abs(com[ax]), abs(com_vel[ax])
        S[ax] = np.abs(K) @ np.abs(window(z, k, N)) + abs(K @ Px[:, 0]) * c + abs(K @ Px[:, 1]) * cd
        tol[ax] = TOL_WINDOW * np.array([c + mpc_dt * cd + 0.5 * mpc_dt ** 2 * S[ax], cd + mpc_dt * S[ax], S[ax]])
    return S, tol


def sensitivity(K, zx, zy, k, S):
    """In units of the tolerance TOL_WINDOW * S, the larger over the two axes of what u moves by when (drop) the term i = N is left
    out, (shift) the window starts one sample late, (last) term N is read from sample k + N - 1."""
    N = len(K) - 1
    out = dict(drop=0.0, shift=0.0, last=0.0)
    for ax, z in enumerate((zx, zy)):
        w0, w1 = window(z, k, N), window(z, k + 1, N)
        unit = TOL_WINDOW * S[ax]
        out["drop"] = max(out["drop"], abs(K[N] * w0[N]) / unit)
        out["shift"] = max(out["shift"], abs(K @ (w1 - w0)) / unit)
        out["last"] = max(out["last"], abs(K[N] * (w0[N] - w0[N - 1])) / unit)
    return out


def mpc_reference_longdouble(K, Px, zx, zy, k, com, com_vel, mpc_dt):
    """(x_ref | y_ref) [6] of the clamped window stated in numpy, in np.longdouble: u = -K (Px x - z_clamped), then A x + B u."""
    ld = np.longdouble
    N = len(K) - 1
    out = np.zeros(6, dtype=ld)
    for ax, z in enumerate((zx, zy)):
        x = np.array([com[ax], com_vel[ax]], dtype=ld)
        u = -(K.astype(ld) @ (Px.astype(ld) @ x - window(z, k, N).astype(ld)))
        dt = ld(mpc_dt)
        out[3 * ax:3 * ax + 3] = [x[0] + dt * x[1] + dt * dt / 2 * u, x[1] + dt * u, u]
    return out.astype(np.float64)


def k_of(t, mpc_dt):
    """(int)(t / mpc_dt) of mpcLinearPendulum.cpp:92: an fp64 quotient truncated towards zero (Python's int() does the same)."""
    return int(np.float64(t) / np.float64(mpc_dt))


def k4_sequence(nt, mpc_dt, t0=0.0):
    """k of the fourth-stage evaluation of every tick: int((t + dt) / mpc_dt) on the float-accumulated clock."""
    t, ks = t0, []
    for _ in range(nt):
        ks.append(k_of(t + DT, mpc_dt))
        t += DT
    return ks


def clamp_cases():
    """(N, mode, where, t): the window leaves the arrays at the end by PAST_END samples (either mode), or at the front (t = T_FRONT on
    the 1 ms grid; on the 10 ms grid that clock is still sample 0 and nothing is clamped)."""
    out = []
    for N in H_CLAMP:
        for mode, m in MODES.items():
            k_end = m["n"] - 1 - N + PAST_END                      # k + N = n - 1 + PAST_END
            out.append((N, mode, "end", (k_end + 0.5) * m["mpc_dt"]))
        out.append((N, "coupled", "front", T_FRONT))
    return out


def clamp_oracle(N, mode, where, t):
    """The oracle of a clamped evaluation: the same arrays padded by repeating the last (or first) sample, and the clock of an
    in-range sample that reads the window the kernel's clamp reads.  Standing foot references are constants, so the clock enters the
    evaluation through k alone (test_preview_cases.py checks that).  -> (oracle, t_oracle, k of the kernel)."""
    m = MODES[mode]
    k = k_of(t, m["mpc_dt"])
    pad_front = max(0, -k)
    pad_back = max(0, k + N - (m["n"] - 1))
    o = make_oracle(N, mode, pad_front=pad_front, pad_back=pad_back)
    return o, (k + pad_front + 0.5) * m["mpc_dt"], k
