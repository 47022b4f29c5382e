"""Target sets and start postures of the inverse-kinematics tests (test_ik_cases.py on the CPU, test_gpu_ik.py on the GPU): one
draw, shared, so that the oracle's iteration counts checked on the CPU are the ones the kernel is held to.

A foot target is [x y z | roll pitch yaw] (Kinematics::desiredOperationalState, invKinematics.cpp:11-25); the Euler angles are those
of R * Rf_q0 (invKinematics.cpp:256-267).  Every draw has a fixed seed.  A (target, start) pair whose stop decision hangs on rounding
(a criterion within a decade of the 1e-10 threshold before the last step) has no well-defined iteration count: test_ik_cases.py refuses
it, and the cure is another seed (TARGET_REDRAWS / START_REDRAWS below), never a tolerance at run time.

How the entries were chosen: each is the first redraw count, counting up from 0, at which the pair passes test_ik_cases.py; a target's
count is settled on start 0 (which has no draw of its own) before its starts are.  With rotated feet the reference's Jacobian is not
exact and the iteration converges linearly; for foot yaw the contraction per step is |yaw| itself (0.02 -> 0.020, 0.1 -> 0.098,
0.3 -> 0.33, measured on the oracle).  A criterion that skips the decade above 1e-10 needs a contraction below 0.1, so the rule above
admits yaw targets below about 0.1 rad only, and most of the +-0.3 rad range is redrawn (hence the large count of the yaw set, which
also asks for MIN_YAW on both feet so that the set is not left with yaws of a hundredth of a radian: 7 to 8 steps against 4 to 5)."""
import numpy as np

N_STARTS = 8
DEFAULT_COM = (-0.02, 0.0, 0.26)
DEFAULT_RF = (0.0, -0.05, 0.0, 0.0, 0.0, 0.0)
DEFAULT_LF = (0.0, 0.05, 0.0, 0.0, 0.0, 0.0)
SET_NAMES = ("default", "feet_staggered_raised", "feet_roll_pitch", "feet_yaw", "com_moved", "all_half")
TARGET_SEED = 20261101           # + set index
START_SEED = 20261201            # + 16 * set index + start index
REDRAW_STEP = 1000               # a redrawn target / start takes seed + REDRAW_STEP * (its entry below)
TARGET_REDRAWS = (0, 0, 2, 538, 0, 7)
START_REDRAWS = ((0, 0, 0, 0, 0, 0, 1, 0), (0, 1, 0, 0, 0, 0, 0, 0), (0, 1, 0, 1, 0, 0, 2, 1),      # [set][start]; start 0 is
                 (0, 5, 6, 0, 2, 3, 9, 9), (0, 1, 2, 0, 0, 0, 0, 0), (0, 2, 0, 1, 0, 0, 1, 8))      # initial_configuration(): no draw
MIN_YAW = 0.05                   # both feet of the yaw set are turned by at least this much
# the sets whose foot targets are rotated: omega_mat(eta) of a foot is not the identity there, and rot_to_euler is away from zero
ROTATED_SETS = (2, 3, 5)
# the CoM no posture reaches from initial_configuration(): the Newton iteration does not converge (test_gpu_ik.py)
UNREACHABLE_COM = (-0.02, 0.0, 0.45)


def initial_configuration():
    """initialConfiguration() of the reference (Robot.cpp:242-251)."""
    return np.array([-0.0185, 0, 0.282, 0, 0, 0, 0, 0, -0.5, 0.8, -0.3, 0, 0, 0, -0.5, 0.8, -0.3, 0,
                     1.6, 0, 0, 0, 0, -1.6, 0, 0, 0, 0, 0, 0], dtype=np.float64)


def _targets(s):
    """com [3], rf [6], lf [6] of set s; amp scales every variation (set 5: one half)."""
    rng = np.random.default_rng(TARGET_SEED + s + REDRAW_STEP * TARGET_REDRAWS[s])
    com, rf, lf = np.array(DEFAULT_COM), np.array(DEFAULT_RF), np.array(DEFAULT_LF)
    amp = 0.5 if s == 5 else 1.0
    if s in (1, 5):                                                # feet staggered and raised: x +-3 cm, y +-1 cm, z 0 .. 2 cm
        for f in (rf, lf):
            f[0] += amp * rng.uniform(-0.03, 0.03); f[1] += amp * rng.uniform(-0.01, 0.01); f[2] += amp * rng.uniform(0.0, 0.02)
    if s in (2, 5):                                                # foot roll / pitch +-0.1 rad
        for f in (rf, lf):
            f[3:5] += amp * rng.uniform(-0.1, 0.1, 2)
    if s in (3, 5):                                                # foot yaw +-0.3 rad
        for f in (rf, lf):
            f[5] += amp * rng.uniform(-0.3, 0.3)
    if s in (4, 5):                                                # CoM: x, y +-2 cm, z 0.23 .. 0.262 (0.26 - 0.03 .. 0.26 + 0.002)
        com[0:2] += amp * rng.uniform(-0.02, 0.02, 2)
        com[2] += amp * rng.uniform(-0.03, 0.002)
    return com, rf, lf


def _start(s, j):
    """Start 0 is initial_configuration(); the others move the legs by +-0.15 rad, arms and head by +-0.5 rad, base x, y by +-1 cm."""
    q = initial_configuration()
    if j == 0:
        return q
    rng = np.random.default_rng(START_SEED + 16 * s + j + REDRAW_STEP * START_REDRAWS[s][j])
    q[0:2] += rng.uniform(-0.01, 0.01, 2)
    q[6:18] += rng.uniform(-0.15, 0.15, 12)
    q[18:30] += rng.uniform(-0.5, 0.5, 12)
    return q


def ik_cases():
    """The six target sets: list of dict(name, com [3], rf [6], lf [6], starts [N_STARTS,30])."""
    out = []
    for s, name in enumerate(SET_NAMES):
        com, rf, lf = _targets(s)
        out.append(dict(name=name, com=com, rf=rf, lf=lf, starts=np.stack([_start(s, j) for j in range(N_STARTS)])))
    return out


# per-robot randomised link tables (the draw of test_gpu_terms.py's test_terms_with_per_robot_models, B = 4): robot i solves target set
# RANDOMISED_SET from start RANDOMISED_STARTS[i]; starts chosen so that no pair is ambiguous on its own model (test_ik_cases.py)
RANDOMISED_SET = 5
RANDOMISED_STARTS = (2, 3, 4, 5)


def randomised_links(nominal):
    """[4,28,13] raw link tables: masses x U(0.9, 1.1), centres of mass +-5 mm, from the nominal table [28,13]."""
    n = len(RANDOMISED_STARTS)
    raw = np.tile(np.asarray(nominal, dtype=np.float64), (n, 1, 1))
    rng = np.random.default_rng(20260004)
    raw[:, :, 0] *= rng.uniform(0.9, 1.1, (n, 28))
    raw[:, :, 1:4] += rng.uniform(-5e-3, 5e-3, (n, 28, 3)) * (raw[:, :, 0:1] > 0)
    return raw


def randomised_solutions(nominal):
    """Oracle(raw_links=raw[i]).ik of robot i's pair -> (raw, [dict(q, iters, crit)])."""
    from oracle.pyoracle import Oracle
    raw, c = randomised_links(nominal), ik_cases()[RANDOMISED_SET]
    return raw, [Oracle(do_ik=False, raw_links=raw[i]).ik(c["starts"][j], c["com"], c["rf"], c["lf"]) for i, j in enumerate(RANDOMISED_STARTS)]


# Tilted starts.  The targets' base attitude is zero, so from a start with a level base the attitude step is exactly zero in every Newton
# step and the base-attitude columns of the Jacobian -- the only ones the OmegaFoot product touches -- multiply zeros: on the six sets above
# an iteration without that product takes the same steps (measured on a kernel built without it).  It acts in the first step from a TILTED
# base.  These eight starts add roll, pitch, yaw of +-TILT rad to the draw of the others and solve target set TILTED_SET; each is the first
# redraw at which the oracle's count is well defined with AND without the product (Oracle.ik(foot_omega=False)) and the two counts differ.
TILTED_SET = 5
TILT = 0.3
TILTED_SEED = 20261301           # + start index + REDRAW_STEP * its entry below
TILTED_REDRAWS = (546, 160, 71, 40, 44, 618, 43, 469)


def tilted_starts():
    """[N_STARTS,30] start postures with a tilted base."""
    out = []
    for j in range(N_STARTS):
        rng = np.random.default_rng(TILTED_SEED + j + REDRAW_STEP * TILTED_REDRAWS[j])
        q = initial_configuration()
        q[0:2] += rng.uniform(-0.01, 0.01, 2)
        q[3:6] += rng.uniform(-TILT, TILT, 3)
        q[6:18] += rng.uniform(-0.15, 0.15, 12)
        q[18:30] += rng.uniform(-0.5, 0.5, 12)
        out.append(q)
    return np.stack(out)


def tilted_solutions(foot_omega=True):
    """Oracle.ik of the tilted starts on target set TILTED_SET -> [dict(q, iters, crit)]; foot_omega=False: without the OmegaFoot product."""
    from oracle.pyoracle import Oracle
    o, c = Oracle(do_ik=False), ik_cases()[TILTED_SET]
    return [o.ik(q, c["com"], c["rf"], c["lf"], foot_omega=foot_omega) for q in tilted_starts()]


_ORACLE = {}


def oracle_solutions():
    """Oracle.ik of every (target, start) pair, computed once per process and shared: [set][start] -> dict(q, iters, crit)."""
    if "nominal" not in _ORACLE:
        from oracle.pyoracle import Oracle
        o = Oracle(do_ik=False)
        _ORACLE["nominal"] = [[o.ik(c["starts"][j], c["com"], c["rf"], c["lf"]) for j in range(N_STARTS)] for c in ik_cases()]
    return _ORACLE["nominal"]
