"""Cases of the per-robot / sequenced inverse kinematics (lmh_ik_batch): test_ik_batch_cases.py checks them on the CPU with the oracle
alone, test_gpu_ik_batch.py holds the kernel to them.  Everything is built from the target sets and starts of ik_cases.py.

The rule is that of ik_cases.py / test_ik_cases.py: a solution cannot pin a Jacobian, so every (robot, target) solve must take exactly the
oracle's number of Newton steps, and a solve whose stop decision hangs on rounding (a criterion in [1e-11, 1e-9] before the last step) has
no defined count and is not used.  well_defined() is that rule; the choices below (which robot solves which set, which chains, which
sweep indices) are the ones that pass it, and test_ik_batch_cases.py checks every one of them rather than assume it.  The oracle of a
sequence is Oracle.ik chained on its own previous solution."""
import numpy as np

from ik_cases import (DEFAULT_COM, DEFAULT_LF, DEFAULT_RF, N_STARTS, RANDOMISED_SET, RANDOMISED_STARTS, SET_NAMES, ik_cases,
                      initial_configuration, oracle_solutions, randomised_links)

STRIDE = 16                                                        # LMH_IK_TARGET_STRIDE: rf6 | lf6 | com(3) | pad
B = N_STARTS
# sequences: chains of set indices; robot j runs CHAINS[j % 4] from start j of the chain's first set
CHAINS = ((2, 0, 4), (1, 3, 2), (0, 4, 3), (1, 0, 5))
# per-robot models: robot i (link table i of randomised_links, start RANDOMISED_STARTS[i] of set RANDOMISED_SET) solves set MODEL_SETS[i]
MODEL_SETS = (2, 1, 4, 0)
# start-posture sweep from initial_configuration(): index i gives CoM height 0.235 + 0.0018 i and soles at y = -/+ (0.04 + 0.00125 i)
SWEEP_INDICES = (1, 2, 3, 4, 5, 6, 7, 8)
SWEEP_COM_XY = (-0.02, 0.0)


def sweep_zcom(i):
    return 0.235 + 0.0018 * i


def sweep_foot_y(i):
    return 0.04 + 0.00125 * i


def record(com=DEFAULT_COM, rf=DEFAULT_RF, lf=DEFAULT_LF):
    """One target record [16] in LmhIkTarget's order, pad zero."""
    r = np.zeros(STRIDE)
    r[0:6], r[6:12], r[12:15] = rf, lf, com
    return r


def set_record(s):
    c = ik_cases()[s]
    return record(c["com"], c["rf"], c["lf"])


def well_defined(r):
    """The rule of test_ik_cases.py on one Oracle.ik result: converged, and no criterion within a decade of the threshold before the
    last step."""
    if not (0 < r["iters"] < 200 and np.isfinite(r["q"]).all()):
        return False
    if not (len(r["crit"]) == r["iters"] + 1 and r["crit"][-1] <= 1e-10 and (r["crit"][:-1] > 1e-10).all()):
        return False
    return not [c for c in r["crit"][:-1] if 1e-11 <= c <= 1e-9]


def oracle_chain(o, q_start, records):
    """Oracle.ik on each record in turn, each from the previous solution -> [dict(q, iters, crit)]."""
    out, q = [], np.asarray(q_start, dtype=np.float64)
    for r in records:
        out.append(o.ik(q, r[12:15], r[0:6], r[6:12]))
        q = out[-1]["q"]
    return out


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _nominal_oracle():
    from oracle.pyoracle import Oracle
    return _once("oracle", lambda: Oracle(do_ik=False))


def per_robot_case():
    """Robot j solves set j % 6 from that set's start j: dict(starts [B,30], targets [B,16], sets [B], sol [B] of the pairs' oracle
    solutions -- the ones test_ik_cases.py pins)."""
    def make():
        cases, sol = ik_cases(), oracle_solutions()
        sets = [j % len(SET_NAMES) for j in range(B)]
        return dict(starts=np.stack([cases[s]["starts"][j] for j, s in enumerate(sets)]), targets=np.stack([set_record(s) for s in sets]),
                    sets=sets, sol=[sol[s][j] for j, s in enumerate(sets)])
    return _once("per_robot", make)


def chain_solutions():
    """[chain][start] -> oracle_chain from start `start` of the chain's first set, for all N_STARTS starts."""
    def make():
        o, cases = _nominal_oracle(), ik_cases()
        return [[oracle_chain(o, cases[ch[0]]["starts"][j], [set_record(s) for s in ch]) for j in range(N_STARTS)] for ch in CHAINS]
    return _once("chains", make)


def chain_case():
    """Robot j runs CHAINS[j % 4] from start j of its first set: dict(starts [B,30], targets [3,B,16], chains [B], sol [B][3])."""
    def make():
        cases, sol = ik_cases(), chain_solutions()
        ch = [j % len(CHAINS) for j in range(B)]
        return dict(starts=np.stack([cases[CHAINS[c][0]]["starts"][j] for j, c in enumerate(ch)]),
                    targets=np.stack([np.stack([set_record(CHAINS[c][k]) for c in ch]) for k in range(3)]),
                    chains=ch, sol=[sol[c][j] for j, c in enumerate(ch)])
    return _once("chain_case", make)


def models_case(nominal):
    """Per-robot link tables with per-robot targets: dict(raw [4,28,13], starts [4,30], targets [4,16], sets, sol [4]), each solution
    from an oracle built on the robot's own table."""
    def make():
        from oracle.pyoracle import Oracle
        raw, cases = randomised_links(nominal), ik_cases()
        starts = cases[RANDOMISED_SET]["starts"][list(RANDOMISED_STARTS)]
        targets = np.stack([set_record(s) for s in MODEL_SETS])
        sol = [oracle_chain(Oracle(do_ik=False, raw_links=raw[i]), starts[i], [targets[i]])[0] for i in range(len(raw))]
        return dict(raw=raw, starts=starts, targets=targets, sets=MODEL_SETS, sol=sol)
    return _once("models", make)


def sweep_record(i):
    y = sweep_foot_y(i)
    return record(com=(SWEEP_COM_XY[0], SWEEP_COM_XY[1], sweep_zcom(i)), rf=(0, -y, 0, 0, 0, 0), lf=(0, y, 0, 0, 0, 0))


def sweep_solution(i):
    """Oracle.ik from initial_configuration() to sweep index i (any i: the CPU test also looks at indices left out of the table)."""
    return _once(("sweep", i), lambda: oracle_chain(_nominal_oracle(), initial_configuration(), [sweep_record(i)])[0])


def sweep_case():
    """dict(starts [B,30], z_com [B], foot_y [B], targets [B,16], sol [B]) of SWEEP_INDICES."""
    idx = SWEEP_INDICES
    return dict(starts=np.tile(initial_configuration(), (len(idx), 1)), z_com=np.array([sweep_zcom(i) for i in idx]),
                foot_y=np.array([sweep_foot_y(i) for i in idx]), targets=np.stack([sweep_record(i) for i in idx]),
                sol=[sweep_solution(i) for i in idx])
