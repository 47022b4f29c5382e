"""Shared cases of the rigid-contact plant and the joint servo over the postures of a fall (test_fall_rigid_cases.py on the CPU,
test_gpu_fall_rigid.py on the GPU): the two plant features that rigid_cases.py and servo_cases.py hold to the oracle on
plant_step_cases.contact_states() alone, within 5 degrees and 0.3 m/s of standing.

Inputs are fall_cases' and are not drawn again: fall_states(band), fall_planes(band), step_references(band)["x0"] / ["tau"] and
pitch_ladder().  Everything here is computed with the CPU oracle, the numpy statement trajectories.rigid_contact_acceleration and
servo_cases.servo_steps; no HIP library is imported.  Results are cached per process and never written by a test.

The flag margin.  The rigid plant's two informational flags are thresholds on the multiplier: f_z < 0 (pull) and hypot(f_x, f_y) > mu f_z
(slip).  The GPU's multiplier is held to the refined KKT solve by the forward bound 1e-12 cond(KKT) max|lambda|, so it may sit that far
from the statement's, with a floor of 1e-9 N (what the near-standing test uses); hypot(f_x, f_y) - mu f_z then moves by at most (1 + mu)
times that.  flag_margin is that distance in newtons, and a flag is compared only where every held foot decides it by more."""
import numpy as np

import fall_cases as fc
import plant_step_cases as pc
import rigid_cases as rc
import servo_cases as sc
from linearmpchumanoid_amd.trajectories import rigid_contact_acceleration

B, BANDS, STEP_N = fc.B, fc.BANDS, fc.STEP_N
MODES, KVS, MU = rc.MODES, rc.KVS, rc.MU
PERTURB = 1e-12                   # relative perturbation of x0 of the step references
SENSITIVITY = sc.SENSITIVITY      # what it may move the end state and the multiplier by
LAM_FLOOR = 50.0                  # [N] the multiplier's sensitivity is taken on max(|lambda|, 50 N): the robot's weight
# the two configurations of the step test: (name, kv, mode of robot i)
STEP_CONFIGS = (("a", 50.0, lambda i: 0), ("b", 0.0, lambda i: (i + 1) % 3))

_cache = {}
_shared = {}


def _oracle():
    if "o" not in _shared:
        _shared["o"] = pc.make_oracle()
    return _shared["o"]


def flag_margin(cond_kkt, lam):
    """[N] how far the project's forward tolerance lets hypot(f_x, f_y) - mu f_z (and so f_z) of a multiplier differ from the statement's."""
    return max(1e-9, 1e-12 * float(cond_kkt) * float(np.abs(lam).max())) * (1.0 + MU)


def decided(lam, rows, margin, mu=MU):
    """Which of the two flags the multiplier decides by more than margin on every held foot -> (pull decided, slip decided)."""
    held = [ft for ft in range(2) if 6 * ft in rows]
    pull = all(abs(lam[6 * ft + 5]) > margin for ft in held)
    slip = all(abs(np.hypot(lam[6 * ft + 3], lam[6 * ft + 4]) - mu * lam[6 * ft + 5]) > margin for ft in held)
    return pull, slip


def decided_on(lam, rows, b):
    """decided() with the margin of the case's own bounds record b (rigid_cases.bounds)."""
    return decided(lam, rows, flag_margin(b["cond"], lam))


def _statement_case(tm, tau30, mode, kv):
    info = {}
    a, lam, flags = rigid_contact_acceleration(tm["M"], tm["C"], tm["J"], tm["Jpqp"], tm["vhat"], tau30, mode, kv, contact_mu=MU, info=info)
    b = rc.bounds(tm, tau30, mode, kv, a, lam)
    margin = flag_margin(b["cond"], lam)
    return dict(a=a, lam=lam, flags=flags, info=info, bounds=b, margin=margin, decided=decided(lam, info["rows"], margin),
                condA=float(np.linalg.cond(info["A"])))


def rigid_fall_cases(band):
    """fall_states(band) under the rigid plant: dict(q, v, tau [16,30], zcom, q0, terms [16] the oracle's with vhat, and cases per
    (i, mode in MODES, kv in KVS) = dict(a, lam, flags, info of the statement, bounds = rigid_cases.bounds, margin = flag_margin [N],
    decided = (pull, slip), condA))."""
    if ("rigid", band) not in _cache:
        S, o = fc.fall_states(band), _oracle()
        terms = [rc.oracle_terms(o, S["q"][i], S["v"][i]) for i in range(B)]
        cases = {(i, m, kv): _statement_case(terms[i], S["tau"][i], m, kv) for i in range(B) for m in MODES for kv in KVS}
        _cache["rigid", band] = dict(q=S["q"], v=S["v"], tau=S["tau"], zcom=S["zcom"], q0=S["q0"], terms=terms, cases=cases)
    return _cache["rigid", band]


def rigid_ladder_cases():
    """fall_cases.pitch_ladder() under the rigid plant, both soles held, kv = 50: dict(q, v, tau [10,30], delta, sign, zcom, terms [10],
    cases [10] as rigid_fall_cases')."""
    if "ladder" not in _cache:
        Ld, o = fc.pitch_ladder(), _oracle()
        terms = [rc.oracle_terms(o, Ld["q"][n], Ld["v"][n]) for n in range(len(Ld["q"]))]
        _cache["ladder"] = dict(Ld, terms=terms, cases=[_statement_case(terms[n], Ld["tau"][n], 0, 50.0) for n in range(len(terms))])
    return _cache["ladder"]


def rigid_trace(o, x, tau30, mode, kv, n=STEP_N):
    """rigid_cases.oracle_rigid_steps (the same evaluations in the same order) that also records, at each of the 4 n evaluations, the
    statement's flags and which of the two its multiplier decides by more than flag_margin.
    -> dict(x [60], flags OR-ed, lam [12] of the first stage of the last substep, stages [4n] = (flags, pull decided, slip decided))."""
    x = np.asarray(x, dtype=np.float64).copy()
    stages, first = [], {}

    def xdot_of(stage, s):
        xd, lam, fl, parts = rc.oracle_rigid_xdot(o, s[:30], s[30:], tau30, mode, kv)
        tm = parts["terms"]
        margin = flag_margin(np.linalg.cond(rc.kkt_matrix(tm["M"], tm["J"], mode)), lam)
        stages.append((fl,) + decided(lam, parts["info"]["rows"], margin))
        if stage == 0:
            first["lam"] = lam
        return xd

    for _ in range(n):
        x = pc.rk4_tick(x, pc.DT, xdot_of)
    flags = 0
    for fl, _, _ in stages:
        flags |= fl
    return dict(x=x, flags=flags, lam=first["lam"], stages=stages)


def perturbation(band, i):
    """The relative perturbation [60] of x0 of state i of a band: 1e-12 with random signs."""
    return 1.0 + PERTURB * np.random.default_rng([fc.FALL_SEED, int(round(band * 1000)), i, 6]).choice([-1.0, 1.0], 60)


def rigid_step_references(band):
    """The rigid step test's references from fall_cases.step_references(band)'s x0 and tau, 20 substeps, in the two configurations of
    STEP_CONFIGS: dict(x0, tau, a = dict(kv, mode [16], x [16,60], lam [16,12], flags [16], stages [16][80], moved = the same from x0
    times perturbation(band, i)), b = ...)."""
    if ("step", band) not in _cache:
        T, o = fc.step_references(band), _oracle()
        R = dict(x0=T["x0"], tau=T["tau"])
        for name, kv, mode_of in STEP_CONFIGS:
            mode = np.array([mode_of(i) for i in range(B)], dtype=np.int32)
            runs = [[rigid_trace(o, x0, T["tau"][i], int(mode[i]), kv) for i, x0 in enumerate(xs)]
                    for xs in (T["x0"], [T["x0"][i] * perturbation(band, i) for i in range(B)])]
            pack = lambda rows: dict(x=np.array([r["x"] for r in rows]), lam=np.array([r["lam"] for r in rows]),
                                     flags=np.array([r["flags"] for r in rows], dtype=np.int32), stages=[r["stages"] for r in rows])
            R[name] = dict(pack(runs[0]), kv=kv, mode=mode, moved=pack(runs[1]))
        _cache["step", band] = R
    return _cache["step", band]


def servo_fall_cases(band):
    """The servo over a fall: per state of step_references(band) the first attempt a < servo_cases.MAX_ATTEMPTS of servo_cases.draw at
    x0 whose 20-substep references pass servo_cases._attempt's conditions on the flat ground and on the state's planes at once.
    dict(x0, tau, planes, zcom, rec [16,48], sp [16,48], ref_flat, ref_planes [16,60], attempt [16], flat / on_planes [16] the whole
    records of _attempt).  No state is left out."""
    if ("servo", band) not in _cache:
        T, P, o = fc.step_references(band), fc.fall_planes(band), _oracle()
        S = dict(q=T["x0"][:, :30], v=T["x0"][:, 30:], tau=T["tau"])
        rows = []
        for i in range(B):
            for a in range(sc.MAX_ATTEMPTS):
                flat = sc._attempt(o, S, i, a)
                planes = None if flat is None else sc._attempt(o, S, i, a, planes=P["planes"][i])
                if planes is not None:
                    break
            else:
                raise RuntimeError("fall_rigid_cases: servo state %d of band %g found no attempt" % (i, band))
            assert np.array_equal(flat["rec"], planes["rec"]) and np.array_equal(flat["sp"], planes["sp"])
            rows.append((flat, planes))
        _cache["servo", band] = dict(x0=T["x0"], tau=T["tau"], planes=P["planes"], zcom=fc.fall_states(band)["zcom"],
                                     rec=np.stack([f["rec"] for f, _ in rows]), sp=np.stack([f["sp"] for f, _ in rows]),
                                     ref_flat=np.stack([f["ref"] for f, _ in rows]), ref_planes=np.stack([p["ref"] for _, p in rows]),
                                     attempt=np.array([f["attempt"] for f, _ in rows]), flat=[f for f, _ in rows], on_planes=[p for _, p in rows])
    return _cache["servo", band]
