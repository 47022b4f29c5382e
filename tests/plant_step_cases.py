"""Shared cases of the torque-driven plant tests (test_plant_step.py on the CPU, test_gpu_plant_step.py on the GPU).

Everything here is computed with the CPU oracle alone: the helper oracle_plant_xdot restates lmh_plant_derivative from Oracle.eval / terms /
contact, and contact_states draws the 16 input states around touch-down.  Results are cached per process and never written by a test.
fall_cases.py draws the rest of the range: the postures, tilts and velocities of a fall."""
import numpy as np

from helpers import oracle_system, posture_sweep

DT, TH = 1e-3, 0.016
B = 16
# lmh_config's default ground (lmh_config_default): what a handle created without overrides uses, plant = 0 or 1
GROUND = dict(k=2.0e4, d=3.0, dt=3.0, mu=0.7)
VERTICES = np.array([[0.1, 0.025, 0.0], [0.1, -0.025, 0.0], [-0.05, 0.025, 0.0], [-0.05, -0.025, 0.0]])      # Robot.cpp:38-42
RF_Q0 = np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]])                                                        # Robot.cpp:28-31
REGIMES = ("out", "stick", "slide", "lifted")


def make_oracle(raw_links=None, ground=GROUND):
    o = oracle_system(DT, TH, raw_links=raw_links)
    o.set_plant(True, **ground)
    return o


def euler_rate_matrix(rpy):
    """matrixAngularVelToEulerDot (generalizedFunctions.cpp:43-50)."""
    cp, sy, cy, tp = np.cos(rpy[1]), np.sin(rpy[2]), np.cos(rpy[2]), np.tan(rpy[1])
    return np.array([[cy / cp, sy / cp, 0.0], [-sy, cy, 0.0], [cy * tp, sy * tp, 1.0]])


def oracle_plant_xdot(o, q, v, tau30, t=0.0):
    """lmh_plant_derivative from the oracle's parts: the terms at the one velocity v (Robot::v_ set to v before the evaluation), the
    contact wrench of that state, a = solve(M, tau30 + J'w - C), the base rows back through X[0] (plant_acceleration,
    orc_controller.c:346-351) and qdot as orc_plant_derivative maps it (:362-370).  Leaves the oracle's Robot::v_ at v.
    Returns (xdot [60], dict(w, vf, terms, a))."""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    o.set_prev_velocity(v)
    o.eval(q, v, t)
    tm = o.terms()
    w, vf = o.contact()
    a = np.linalg.solve(tm["M"], np.asarray(tau30, dtype=np.float64) + tm["J"].T @ w - tm["C"])
    sol = np.linalg.solve(tm["X"][0], a[:6])
    qdot = v.copy()
    qdot[0:3] += np.cross(v[3:6], q[0:3])
    qdot[3:6] = euler_rate_matrix(q[3:6]) @ v[3:6]
    return np.concatenate([qdot, sol[3:6], sol[0:3], a[6:]]), dict(w=w, vf=vf, terms=tm, a=a)


def rk4_tick(x, dt, xdot_of):
    """rk4.hpp:5-18; xdot_of(stage, state) -> xdot [60]."""
    k1 = xdot_of(0, x)
    k2 = xdot_of(1, x + 0.5 * dt * k1)
    k3 = xdot_of(2, x + 0.5 * dt * k2)
    k4 = xdot_of(3, x + dt * k3)
    return x + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def oracle_plant_steps(o, x, tau30, n, dt=DT):
    """n RK4 substeps of the helper with the torques held."""
    x = np.asarray(x, dtype=np.float64).copy()
    for _ in range(n):
        x = rk4_tick(x, dt, lambda stage, s: oracle_plant_xdot(o, s[:30], s[30:], tau30)[0])
    return x


def vertex_kinematics_of(tm, v):
    """vertex_kinematics from the terms `tm` of an evaluation at (q, v) that has already run."""
    vhat = np.asarray(v, dtype=np.float64).copy()
    X0 = tm["X"][0]
    vhat[:6] = X0 @ np.concatenate([v[3:6], v[0:3]])                # swapBaseVelocityAndRefToWorldFrame
    twist = tm["J"] @ vhat
    pos, vel = np.zeros((8, 3)), np.zeros((8, 3))
    for f, frame in enumerate((7, 14)):
        T = tm["T"][frame]
        for vi in range(4):
            rp = T[:3, :3] @ (RF_Q0.T @ VERTICES[vi])
            pos[4 * f + vi] = rp + T[:3, 3]
            vel[4 * f + vi] = twist[6 * f + 3:6 * f + 6] + np.cross(twist[6 * f:6 * f + 3], rp)
    return pos, vel


def vertex_kinematics(o, q, v):
    """World position [8,3] and velocity [8,3] of the sole vertices (foot-major) from the oracle's transforms and Jacobian."""
    o.set_prev_velocity(v)
    o.eval(q, v, 0.0)
    return vertex_kinematics_of(o.terms(), v)


def classify(pos, vel, vf, g=GROUND):
    """Regime of every vertex from the oracle's own forces: out of the ground | stick (tangential force unclamped and non-zero) | slide
    (clamped onto mu f_n > 0) | lifted (penetrating, normal force clamped to 0)."""
    out = []
    for i in range(8):
        pen = -pos[i, 2]
        if not pen > 0.0:
            out.append("out"); continue
        if vf[i, 2] == 0.0:
            out.append("lifted" if g["k"] * pen - g["d"] * vel[i, 2] < 0.0 else "?"); continue
        raw = g["dt"] * np.hypot(vel[i, 0], vel[i, 1])
        ft = np.hypot(vf[i, 0], vf[i, 1])
        out.append("slide" if raw > g["mu"] * vf[i, 2] else ("stick" if ft > 0.0 else "?"))
    return out


_cache = {}


def contact_states():
    """The 16 GPU inputs: posture_sweep postures (band 0.3) with tilts of a few degrees, lowered so that a chosen vertex of a chosen foot
    sits at a chosen depth, velocities of a few dm/s.  State i aims at foot i % 2 and regime REGIMES[(i // 2) % 4] in the MIDDLE of that
    regime's band (a factor two from its thresholds: round-off cannot move a vertex across one), which at the default ground means
    depths between 10 um and 2 mm.  Returns dict(q0, zcom, q [16,30], v [16,30], regimes [16][8], tau [16,30])."""
    if _cache:
        return _cache
    o = make_oracle()
    q0, zcom = o.robot()["q"].copy(), o.zcom
    q, v, _ = posture_sweep(q0, B, band=0.3)
    g = GROUND
    regimes = []
    for i in range(B):
        rng = np.random.default_rng(20261018 + i)
        q[i, 3:5] *= 0.3                                           # tilts up to 5 degrees: the vertices of one sole spread over a centimetre
        v[i, 0:3] = rng.uniform(-0.3, 0.3, 3)                      # a few dm/s
        foot, want = i % 2, REGIMES[(i // 2) % 4]
        if want in ("slide", "lifted"):
            v[i, 2] = abs(v[i, 2]) + (0.2 if want == "lifted" else 0.0)        # going up
        pos, vel = vertex_kinematics(o, q[i], v[i])
        mine = range(4 * foot, 4 * foot + 4)
        if want == "out":
            j = min(mine, key=lambda n: pos[n, 2]); depth = -1.0e-3            # the whole foot a millimetre up
        elif want == "stick":
            j = min(mine, key=lambda n: pos[n, 2]); depth = 2.0e-3             # f_n ~ 40 N against a tangential 3 N s/m x 0.3 m/s
        elif want == "slide":                                      # mu f_n = half the unclamped tangential force
            ok = [n for n in mine if 0.5 * g["dt"] * np.hypot(vel[n, 0], vel[n, 1]) / g["mu"] + g["d"] * vel[n, 2] > 0.0]
            j = ok[0]; depth = (0.5 * g["dt"] * np.hypot(vel[j, 0], vel[j, 1]) / g["mu"] + g["d"] * vel[j, 2]) / g["k"]
        else:                                                      # k depth = half of c zdot
            ok = [n for n in mine if vel[n, 2] > 0.0]
            j = ok[0]; depth = 0.5 * g["d"] * vel[j, 2] / g["k"]
        q[i, 2] -= pos[j, 2] + depth
        pos, vel = vertex_kinematics(o, q[i], v[i])
        _, vf = o.contact()
        regimes.append(classify(pos, vel, vf))
    tau = np.random.default_rng(20261019).normal(0.0, 2.0, (B, 30))            # N m on every row, the base wrench included
    _cache.update(q0=q0, zcom=zcom, q=q, v=v, regimes=regimes, tau=tau)
    return _cache
