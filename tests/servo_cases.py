"""Shared cases of the joint-servo tests (test_servo.py on the CPU, test_gpu_servo.py on the GPU), computed with the CPU oracle alone and
cached per process; never written by a test.

Inputs: the 16 states and torques of plant_step_cases.contact_states().  Gains are per robot and joint, scaled by the joint's own inertia
at the state, m_j = 1 / (M^-1)_jj of the oracle's M: kd_j = U(0.05, 0.25) m_j / dt and kp_j = U(0.01, 0.05) m_j / dt^2.  On a joint alone
that is kd dt / m <= 0.25 and kp dt^2 / m <= 0.05 against classic RK4's stability interval (2.78 on the real axis): the reference is a
trajectory, not an explosion.  Setpoints: the state's joints moved by U(-0.05, 0.05) rad and U(-0.5, 0.5) rad/s.

The reference is plant_step_cases.rk4_tick over oracle_plant_xdot with trajectories.servo_torque applied to the stage's own state, 20
substeps.  Robot i draws from default_rng([SERVO_SEED, i, a]) for attempt a = 0, 1, ..: the first attempt whose reference passes every
condition of _attempt() -- the conditions test_servo.py asserts again -- is the case, `attempt` records which it was, and no state is left
out."""
import numpy as np

import ground_cases as gc
import plant_step_cases as pc
from linearmpchumanoid_amd.trajectories import servo_records, servo_torque

DT, B, N_SUB = pc.DT, pc.B, 20
SERVO_SEED = 20261201
MAX_ATTEMPTS = 8
PERTURB = 1e-12                   # relative perturbation of the start state
SENSITIVITY = 1e-9                # what it may move the end state by (relative): a hundredth of the GPU tolerance 1e-7

_cache = {}


def joint_inertias(o, q, v):
    """m_j = 1 / (M^-1)_jj of the 24 joints from the oracle's mass matrix at (q, v)."""
    o.set_prev_velocity(v)
    o.eval(q, v, 0.0)
    return 1.0 / np.diag(np.linalg.inv(o.terms()["M"]))[6:30]


def draw(o, q, v, i, a):
    """-> (record [48], setpoint [48]) of robot i, attempt a"""
    rng = np.random.default_rng([SERVO_SEED, i, a])
    m = joint_inertias(o, q, v)
    kd = rng.uniform(0.05, 0.25, 24) * m / DT
    kp = rng.uniform(0.01, 0.05, 24) * m / DT ** 2
    sp = np.concatenate([q[6:30] + rng.uniform(-0.05, 0.05, 24), v[6:30] + rng.uniform(-0.5, 0.5, 24)])
    return servo_records(1, kp, kd)[0], sp


def servo_steps(o, x, tau30, rec, sp, n, planes=None):
    """n RK4 substeps with the servo's torque re-formed at every stage -> (end state [60], regimes of the n * 4 evaluations [[8]]).
    planes None: the oracle's own contact (plant_step_cases.oracle_plant_xdot); a ground record [8]: ground_cases.ground_plant_xdot."""
    x = np.asarray(x, dtype=np.float64).copy()
    regimes = []

    def xdot_of(stage, s):
        tau = servo_torque(rec, sp, s[:30], s[30:], tau30)
        if planes is None:
            xd, parts = pc.oracle_plant_xdot(o, s[:30], s[30:], tau)
            pos, vel = pc.vertex_kinematics_of(parts["terms"], s[30:])
            regimes.append(pc.classify(pos, vel, parts["vf"]))
        else:
            xd, parts = gc.ground_plant_xdot(o, s[:30], s[30:], tau, planes)
            g = pc.GROUND
            regimes.append(list(gc.trajectories.ground_contact(parts["pos"], parts["vel"], planes, g["k"], g["d"], g["dt"], g["mu"])[1]))
        return xd

    with np.errstate(all="ignore"):
        for _ in range(n):
            x = pc.rk4_tick(x, DT, xdot_of)
    return x, regimes


def _attempt(o, S, i, a, planes=None):
    """One draw of robot i and its reference, or None where a condition fails: the 20-substep reference is finite; the start state moved
    by 1e-12 relative moves the end state by less than 1e-9 relative; both runs give every vertex the same regime at all 80 evaluations
    and no regime is undecided.  planes (a ground record [8], optional): the same draw and conditions on that ground."""
    q, v, tau = S["q"][i], S["v"][i], S["tau"][i]
    rec, sp = draw(o, q, v, i, a)
    x0 = np.concatenate([q, v])
    ref, regimes = servo_steps(o, x0, tau, rec, sp, N_SUB, planes=planes)
    if not np.isfinite(ref).all() or any("?" in r for r in regimes):
        return None
    sign = np.where(np.random.default_rng([SERVO_SEED, i, a, 1]).integers(0, 2, 60) == 1, 1.0, -1.0)
    moved, regimes_moved = servo_steps(o, x0 * (1.0 + PERTURB * sign), tau, rec, sp, N_SUB, planes=planes)
    sens = float(np.abs(moved - ref).max() / np.abs(ref).max())
    if not np.isfinite(moved).all() or not sens < SENSITIVITY or regimes_moved != regimes:
        return None
    return dict(rec=rec, sp=sp, ref=ref, moved=moved, regimes=regimes, regimes_moved=regimes_moved, sens=sens, attempt=a)


def servo_cases():
    """dict(q, v, tau [16,30] and zcom of contact_states(); rec [16,48], sp [16,48], ref [16,60] the 20-substep references, moved [16,60]
    those from the perturbed start, regimes / regimes_moved [16][80][8], sens [16], attempt [16])."""
    if _cache:
        return _cache
    S = pc.contact_states()
    o = pc.make_oracle()
    rows = []
    for i in range(B):
        for a in range(MAX_ATTEMPTS):
            r = _attempt(o, S, i, a)
            if r is not None:
                break
        else:
            raise RuntimeError("servo_cases: state %d found no attempt" % i)
        rows.append(r)
    _cache.update(q=S["q"], v=S["v"], tau=S["tau"], zcom=S["zcom"], q0=S["q0"],
                  **{k: np.stack([r[k] for r in rows]) for k in ("rec", "sp", "ref", "moved", "sens", "attempt")},
                  regimes=[r["regimes"] for r in rows], regimes_moved=[r["regimes_moved"] for r in rows])
    return _cache


_ground = {}


def ground_reference():
    """The 20-substep references of the same gains, setpoints and torques on the 16 tilted records of ground_cases.tilted_states(), with
    the contact forces of trajectories.ground_contact: dict(planes [16,8], ref [16,60])."""
    if _ground:
        return _ground
    S, T = servo_cases(), gc.tilted_states()
    o = pc.make_oracle()
    ref = [servo_steps(o, np.concatenate([S["q"][i], S["v"][i]]), S["tau"][i], S["rec"][i], S["sp"][i], N_SUB, planes=T["planes"][i])[0] for i in range(B)]
    _ground.update(planes=T["planes"], ref=np.stack(ref))
    return _ground
