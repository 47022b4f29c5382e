"""CPU checks of tests/fp32_cases.py, the yardstick of the LMH_PRECISION_FP32 parity tests: the numpy statement of the fp32 set-up's
algebra reproduces the oracle's QP solution in float64 on every robot of every case; its float32 run has fp32-sized errors; and the
oracle's final free sets fall cleanly on one side of the kernel's pivot rule, which is what lets the GPU test assert the route flag on
every robot."""
import numpy as np
import pytest

import fp32_cases as fc
from helpers import WEIGHT, vec_err


def _contact(r):
    return r["F"] != 0


@pytest.mark.parametrize("name", fc.CASES)
def test_float64_algebra_reproduces_the_oracle(name):
    """setup_algebra(float64) on the oracle's own terms, with the oracle's final free set: tau and qdd at 1e-8 of their largest entry, f at
    1e-8 of the weight (the bars of test_independent_restatement between two codings of the QP), a = x[:30] and the row-space part of c
    beside them, every robot."""
    c = fc.case(name)
    assert c["q"].shape[0] <= 32
    worst, bad = {}, []
    for i, r in enumerate(c["ref"]):
        s = fc.algebra(name, i, np.float64)
        e, x = r["e"], r["qp"]["x"]
        errs = dict(tau=vec_err(s["tau"], e["tau"]), qdd=vec_err(s["qdd"], e["qpp"]), f=float(np.abs(s["f"] - e["f"]).max() / WEIGHT),
                    a=vec_err(s["a"], x[:30]), Gc=float(np.abs(r["G"] @ (s["c"] - x[42:74])).max() / (WEIGHT + np.abs(x[30:42]).max())))
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
            if not v < 1e-8:
                bad.append((i, k, v))
        assert np.abs(r["G"] @ x[42:74] - x[30:42]).max() < 1e-9 * (WEIGHT + np.abs(x[30:42]).max())     # G is the oracle's wrench map
        for ft in range(2):                                       # a foot without free coefficients: exactly no wrench
            if not (r["F"] >> (16 * ft)) & 0xFFFF:
                assert np.all(s["f"][6 * ft:6 * ft + 6] == 0.0)
    print("\n%s: float64 algebra vs oracle: " % name + ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert not bad, bad[:12]


@pytest.mark.parametrize("name", fc.CASES)
def test_float32_algebra_has_fp32_sized_errors(name):
    """The float32 run against the float64 run on the same inputs: above 1e-6 (it is not float64 in disguise) and below 5e-2 (it is a
    usable statement of what fp32 arithmetic delivers) on tau, every robot that has contact."""
    c = fc.case(name)
    worst, least = 0.0, np.inf
    for i, r in enumerate(c["ref"]):
        if not _contact(r):
            continue
        s64, s32 = fc.algebra(name, i, np.float64), fc.algebra(name, i, np.float32)
        assert s32["Y"].dtype == np.float32 and s32["W"].dtype == np.float32 and s32["a"].dtype == np.float32
        err = vec_err(s32["tau"], s64["tau"])
        worst, least = max(worst, err), min(least, err)
        assert 1e-6 < err < 5e-2, (name, i, err)
    print("\n%s: float32 vs float64 algebra, tau: %.2e .. %.2e" % (name, least, worst))


@pytest.mark.parametrize("name", fc.CASES)
def test_pivot_classes_of_the_oracle_sets(name):
    """Every foot of every oracle set is `full` in the cases that must stay on the fp32 push-through route and `deficient` in the posture
    sweeps; none is `unclear`.  flight has no free coefficient at all."""
    c = fc.case(name)
    classes = [fc.set_class(r["F"], r["G"]) for r in c["ref"]]
    print("\n%s: free sets %s | %s" % (name, " ".join("%08x" % r["F"] for r in c["ref"]), " ".join(classes)))
    assert "unclear" not in classes
    if name in fc.FULL_CASES:
        assert all(k == "full" for k in classes), classes
    elif name in fc.DEFICIENT_CASES:
        assert all(k == "deficient" for k in classes), classes
    else:
        assert name == "flight" and all(k == "empty" for k in classes), classes


def test_lowmu_has_sets_between_the_kernels_rule_and_a_tenth():
    """What `lowmu` is for: oracle sets that are full rank (ratio >= 1e-2, two orders above the kernel's 1e-4) and below 1e-1, so that a
    pivot rule of 1e-1 would send them down the fp64 route; the other full cases have none (0.71 .. 0.93)."""
    ratios = [fc.set_ratio(r["F"], r["G"]) for r in fc.case("lowmu")["ref"]]
    assert sum(fc.FULL_RATIO <= x < 0.09 for x in ratios) >= 3, ratios
    for name in fc.FULL_CASES:
        if name != "lowmu":
            assert min(fc.set_ratio(r["F"], r["G"]) for r in fc.case(name)["ref"]) > 0.5


def test_pivot_ratio_on_known_matrices():
    assert fc.pivot_ratio(np.eye(6)) == 1.0
    A = np.array([[1.0, 1.0], [1.0, 1.0]])
    assert fc.pivot_ratio(A) <= fc.DEFICIENT_RATIO
    assert abs(fc.pivot_ratio(np.array([[2.0, 1.0], [1.0, 2.0]])) - 0.75) < 1e-15
    G = np.zeros((12, 32)); G[:6, :6] = np.eye(6); G[6, 16] = 1.0
    assert fc.pivot_class(0x0001003F, G) == {0: "full", 1: "deficient"}
    assert fc.set_class(0, G) == "empty" and fc.set_class(0x3F, G) == "full" and fc.set_class(0x0001003F, G) == "deficient"


def test_warm_case_masks():
    c = fc.case("warm")
    assert c["config"]["warm_start"] == 1 and c["n_evals"] == 2 and len(c["masks"]) == 8
    assert c["masks"][0] == 0 and c["masks"][1] == 0xFFFFFFFF
    assert c["masks"][2] == c["ref"][0]["e"]["active_mask"] and c["masks"][3] == (~c["masks"][2]) & 0xFFFFFFFF
    assert len(set(c["masks"])) == 8
    assert all(r["F"] == c["ref"][0]["F"] for r in c["ref"]) and (c["q"] == c["q"][0]).all() and (c["v"] == c["v"][0]).all()
