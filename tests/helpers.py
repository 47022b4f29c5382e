"""Shared helpers for the parity tests (oracle = checker; HIP path = thing under test), and the one home of the tests' scaffolding:

  tolerances      rel_err, vec_err, close, close_on, TOL_REL, TOL_FLOOR, WEIGHT
  draws           perturbed_velocities, posture_sweep, sincos_quadrants
  oracles         oracle_system, make_oracle, start_posture, the cfg2 fixture, dense_terms_from_debug
  controllers     horizon_time, make_controller (dt, th given), horizon_controller (N, mpc_dt given), to_device
  bit identity    same_bits (one array), bits_differ (the fields of two rollout results)
  child processes child_env / run_probe (a fresh Python on a chosen build), bench_env / run_bench (bench.py)

Nothing here imports linearmpchumanoid_amd at module level, so the CPU tests can import it without the HIP library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyoracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL_REL = 1e-6      # north_star: 1e-6 relative on torques / forces
TOL_FLOOR = 1e-9    # absolute floor as a fraction of max|.| (near-zero entries such as n_z)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    return float(np.abs(a - b).max() / scale)


def vec_err(a, b):
    """max|a - b| / max|b| of the SAME vector (north_star / SURVEY 8d); inf when the reference is all-zero and the vectors differ."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    d = float(np.abs(a - b).max()) if a.size else 0.0
    den = float(np.abs(b).max()) if b.size else 0.0
    if den == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / den


def close_on(a, b, tol, scale):
    """max|a - b| <= tol * scale with an EXPLICIT physical scale: for quantities that are small differences of larger ingredients
    (velocity products at rest, PD references of a robot standing on its references), where max|b| of the vector itself is round-off of
    those ingredients.  The caller names the ingredient scale; there is no implicit 1.0."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return bool(np.abs(a - b).max() <= tol * float(scale))


def close(a, b, tol=TOL_REL, scale=None):
    """The parity rule of north_star / SURVEY 8d: max|a - b| <= tol * max|b| of the SAME vector -- relative, with no absolute 1.0 in
    the denominator.  `scale` (optional) is the max-abs entry of the quantity SET the vector belongs to (e.g. the robot's weight for
    a contact-force vector that is identically zero in flight): it adds SURVEY's absolute floor TOL_FLOOR * scale = 1e-9 * scale to the
    allowed error.  Without it an all-zero reference demands identical vectors.  NaN anywhere fails."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    d = np.abs(a - b).max()
    allowed = tol * np.abs(b).max()
    if scale is not None:
        allowed = max(allowed, TOL_FLOOR * float(scale))
    return bool(d <= allowed)


WEIGHT = 5.305 * 9.81    # m g of the nominal NAO [N] (Robot::getMass 5.305 kg): the scale of the contact-force set


def perturbed_velocities(B, seed=20260001):
    """BASELINE config 2 perturbation: dq[0:2] ~ U(-0.3,0.3) m/s, dq[6:30] ~ N(0,0.05^2) rad/s."""
    v = np.zeros((B, 30))
    for i in range(B):
        rng = np.random.default_rng(seed + i)
        v[i, 0:2] = rng.uniform(-0.3, 0.3, 2)
        v[i, 6:] = rng.normal(0.0, 0.05, 24)
    return v


SWEEP_BANDS = (0.3, 1.0, 3.1)    # half-widths [rad] of the posture sweep around the IK start posture
SWEEP_SEED = 20261016
SWEEP_TILT = 1.2                 # |roll|, |pitch| of the sweep's postures: the Euler-rate map of the integrator is singular at pitch = pi/2
# theta offsets of the 24 joints in the DH table (Robot.cpp:59-87): theta_i = q[6 + i] + DH_OFFSET[i]
DH_OFFSET = np.zeros(24)
DH_OFFSET[[1, 6, 7, 13, 18, 23]] = np.array([0.75, -0.5, 0.25, 0.5, 0.5, -0.5]) * np.pi


def posture_sweep(q0, B, band, seed=SWEEP_SEED, tilt=SWEEP_TILT):
    """B states away from the start posture q0, the same draw for the CPU and the GPU tests: joints q0 + U(-band, band) rad, roll and
    pitch U(-min(band, tilt), min(band, tilt)), yaw U(-band, band), base position q0 + U(-0.1, 0.1) m; velocities
    perturbed_velocities plus N(0, 0.2^2) on the base's z and angular components; a random previous velocity (Robot::v_).
    Returns q [B,30], v [B,30], v_prev [B,30]."""
    q = np.tile(np.asarray(q0, dtype=np.float64), (B, 1))
    v = perturbed_velocities(B, seed=seed + 1000003)
    vprev = perturbed_velocities(B, seed=seed + 2000003)
    lim = min(band, tilt)
    for i in range(B):
        rng = np.random.default_rng([seed, int(round(band * 1000)), i])
        q[i, 0:3] += rng.uniform(-0.1, 0.1, 3)
        q[i, 3:5] += rng.uniform(-lim, lim, 2)
        q[i, 5] += rng.uniform(-band, band)
        q[i, 6:] += rng.uniform(-band, band, 24)
        v[i, 2:6] += rng.normal(0.0, 0.2, 4)
    return q, v, vprev


def sincos_quadrants(q):
    """n = rint(theta * 2 / pi) of every angle the forward kinematics takes a sine and cosine of: [B,27] (24 joints with their DH
    offsets, then roll, pitch, yaw).  n & 3 selects the quadrant branch of a reduced-range sin / cos."""
    q = np.asarray(q, dtype=np.float64)
    theta = np.concatenate([q[:, 6:] + DH_OFFSET[None, :], q[:, 3:6]], axis=1)
    return np.rint(theta * (2.0 / np.pi)).astype(np.int64)


def oracle_system(dt, horizon_time, sim_time=2.0, raw_links=None):
    return Oracle(sim_time=sim_time, dt=dt, horizon_time=horizon_time, do_ik=True, raw_links=raw_links)


def horizon_time(N, mpc_dt):
    return N * mpc_dt + 1e-9                                       # int(th / mpc_dt) == N whatever the rounding of the quotient


def make_oracle(N, sim_time, mpc_dt):
    return Oracle(sim_time=sim_time, dt=mpc_dt, horizon_time=horizon_time(N, mpc_dt), do_ik=True)


def start_posture(o):
    """The LIPM height and the IK start posture of an oracle: what a handle and its first state are made from."""
    return dict(zcom=o.zcom, q0=o.robot()["q"].copy())


@pytest.fixture(scope="module")
def cfg2():
    """BASELINE config 2 constants: dt = 1 ms, N = 16.  Imported by the modules that use it; built once per importing module."""
    return dict(dt=1e-3, th=0.016, **start_posture(oracle_system(1e-3, 0.016)))


def make_controller(B, dt, th, zcom, **cfg):
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    return BatchedController(B, default_config(dt=dt, time_horizon=th, z_com=zcom, **cfg))


def horizon_controller(B, N, zcom, mpc_dt, dt, **cfg):
    """A handle whose preview is N samples of mpc_dt, integrated at dt."""
    return make_controller(B, dt, horizon_time(N, mpc_dt), zcom, mpc_dt=mpc_dt, **cfg)


def to_device(ctl, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(ctl.device)


def check_record_table(ctl, name, defaults, records, bad, words):
    """What lmh_set_<name> / lmh_get_<name> / lmh_<name>_per_instance (name: "actuators" | "servo" | "ground") owe on a handle of TWO robots
    with no table, whole records through the C calls, no launch: an empty table reads as `defaults` [width] for both robots; one shared
    record reads back through both; a table of two (records [2,width], two different good ones) reads back robot by robot; a refused set
    (bad [2,width]: robot 1 breaks the rule `words`; three records for two robots) leaves the shared and the per-robot table readable as
    they were; NULL clears."""
    import ctypes as C
    from linearmpchumanoid_amd import capi
    L, h = capi.lib(), ctl._h
    set_, get, per = getattr(L, "lmh_set_" + name), getattr(L, "lmh_get_" + name), getattr(L, "lmh_%s_per_instance" % name)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert ctl.B == 2 and records.shape == bad.shape == (2,) + defaults.shape and not same_bits(records[0], records[1])

    def reads(want0, want1, per_robot):
        got = np.full((2,) + defaults.shape, -7.0)
        assert all(get(h, i, ptr(got[i])) == 0 for i in (0, 1))
        return same_bits(got[0], want0) and same_bits(got[1], want1) and per(h) == per_robot

    def refused():
        three = np.concatenate([records, records[:1]])
        return (set_(h, ptr(bad), 2) == -2 and L.lmh_last_error().decode() == "robot 1: " + words
                and set_(h, ptr(three), 3) == -2 and L.lmh_last_error().decode().endswith("n_sets must be 1 or n_instances"))

    assert reads(defaults, defaults, 0), "defaults from an empty table"
    assert refused() and reads(defaults, defaults, 0), "a refused set leaves the empty table"
    assert set_(h, ptr(records[1].copy()), 1) == 0 and reads(records[1], records[1], 0), "a shared table through every robot"
    assert refused() and reads(records[1], records[1], 0), "a refused set leaves the shared table"
    assert set_(h, ptr(records), 2) == 0 and reads(records[0], records[1], 1), "a per-robot table robot by robot"
    assert refused() and reads(records[0], records[1], 1), "a refused set leaves the per-robot table"
    assert set_(h, None, 0) == 0 and reads(defaults, defaults, 0), "NULL clears"


def same_bits(a, b):
    """Two numpy arrays or two torch tensors (on any device) are the same shape, dtype and bytes: -0.0 is not 0.0, and a NaN equals only
    the same NaN pattern."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    import torch
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def bits_differ(a, b, rows=None, rows_b=None):
    """Names of the fields (state, out, status, log) of two rollout results that are not bit-identical: [] = the same computation.
    rows / rows_b select the robots of a / b."""
    ra = slice(None) if rows is None else rows
    rb = ra if rows_b is None else rows_b
    bad = [k for k in ("state", "out", "status") if not same_bits(a[k][ra], b[k][rb])]
    if not same_bits(a["log"][:, ra], b["log"][:, rb]):
        bad.append("log")
    return bad


RANK_VARS = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")     # what a launcher around the suite would hand down to bench.py


def child_env(variant=None, extra=None):
    """The environment of a child on a chosen build: this one's without LMH_VARIANT and LMH_DIAG, then LMH_VARIANT = variant when
    that is non-empty, then `extra`."""
    env = {k: v for k, v in os.environ.items() if k not in ("LMH_VARIANT", "LMH_DIAG")}
    if variant:
        env["LMH_VARIANT"] = variant
    env.update(extra or {})
    return env


def bench_env(extra=None):
    """The environment bench.py is started in: this one's without the rank variables, then `extra`."""
    env = {k: v for k, v in os.environ.items() if k not in RANK_VARS}
    env.update(extra or {})
    return env


def run_probe(code, variant="", timeout=900, env_extra=None, args=()):
    """`python -c code args...` from the repository root on the build `variant` ("" = the shipped library), which must exit with
    status 0: -> the last line of its output that starts with `{`, parsed as JSON.  A child, because capi chooses the library
    (LMH_VARIANT) when it is imported: a process that has loaded one build cannot run another."""
    r = subprocess.run([sys.executable, "-c", code, *args], env=child_env(variant, env_extra), cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def run_bench(argv, env_extra=None, expect_rc=0, timeout=900):
    """bench.py with argv, which must exit with expect_rc and print exactly one result line: -> that line, parsed."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=bench_env(env_extra), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == expect_rc, (r.returncode, r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def dense_terms_from_debug(d):
    """Rebuild the reference-shaped matrices from the kernel's compact debug record."""
    parent = [-1, 0, 1, 2, 3, 4, 5, 6, 0, 8, 9, 10, 11, 12, 13, 0, 15, 16, 17, 18, 0, 20, 21, 22, 23, 0, 25, 26]
    T = np.zeros((28, 4, 4)); T[:, :3, :] = d["T"]; T[:, 3, 3] = 1
    X = np.zeros((28, 6, 6))
    for i in range(28):
        A = d["XE"][i].T
        X[i, :3, :3] = A; X[i, 3:, 3:] = A; X[i, 3:, :3] = d["XB"][i]
    M = np.zeros((30, 30))
    M[:6, :] = d["Mtop"]; M[6:, :6] = d["Mtop"][:, 6:].T
    start = [0] * 6 + [6] * 6 + [12] * 5 + [17] * 5 + [22] * 2
    nl = [6] * 12 + [5] * 10 + [2] * 2
    for a in range(24):
        for b in range(nl[a]):
            M[6 + a, 6 + start[a] + b] = d["Hl"][a, b]
    J = np.zeros((12, 30))
    for ft in range(2):
        J[6 * ft:6 * ft + 6, :6] = d["Jc"][ft][:, :6]
        J[6 * ft:6 * ft + 6, 6 + 6 * ft:12 + 6 * ft] = d["Jc"][ft][:, 6:]
    return dict(T=T, X=X, M=M, J=J, parent=parent)
