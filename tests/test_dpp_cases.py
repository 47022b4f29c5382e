"""The references of the DPP-layer tests check themselves on the CPU: the lane-level emulators against plain numpy on inputs where every
partial result is exact, the plain fp64 restatements of the eliminations against one eighth of the bounds the GPU solves are held to, and
the harness library builds and exports every launcher (test_gpu_dpp.py runs it)."""
import ctypes

import numpy as np
import pytest

import dpp_cases as dc


def rows(x):
    return np.asarray(x).reshape(4, 16)


def test_fma_rounds_once():
    # (1 + 2^-52)(1 - 2^-53) = 1 + 2^-53 - 2^-105: the product rounded on its own is 1, the fused result keeps 2^-53 - 2^-105
    a, b = 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53
    assert dc.fma(a, b, -1.0) == 2.0 ** -53 * (1.0 - 2.0 ** -52) and a * b - 1.0 == 0.0
    assert dc.fma(2.0 ** 27 + 1.0, 2.0 ** 27 + 1.0, -2.0 ** 54) == 2.0 ** 28 + 1.0
    assert dc.fma(3.0, 5.0, 7.0) == 22.0


def test_permutations_are_the_headers():
    assert all(sorted(p) == list(range(64)) and np.array_equal(p[p], dc.LANES) and np.array_equal(p >> 4, dc.LANES >> 4)
               for p in dc.PERM.values())
    assert list(dc.PERM[0xB1][:4]) == [1, 0, 3, 2] and list(dc.PERM[0x4E][:4]) == [2, 3, 0, 1]
    assert list(dc.PERM[0x141][16:24]) == [23, 22, 21, 20, 19, 18, 17, 16] and list(dc.PERM[0x140][32:35]) == [47, 46, 45]
    t = dc.lane_tags()
    w = t.view(np.uint32).reshape(64, 2)
    assert len(set(w[:, 0])) == 64 and len(set(w[:, 1])) == 64 and np.all(np.isfinite(t)) and np.all(np.abs(t) >= 1.0)
    assert len(set(dc.lane_tags_f32())) == 64


def test_emulators_agree_with_numpy_where_every_partial_result_is_exact():
    rng = np.random.default_rng(dc.SEED)
    acc0, acc1, src, mm = (dc.exact_inputs(rng, 64) for _ in range(4))
    m = dc.exact_inputs(rng, (15, 64))
    s = rows(src)                                                                         # s[row, k] = lane k of DPP row `row`
    for j in (0, 7, 15):
        assert np.array_equal(dc.emu_fmac_one(acc0, src, mm, j), acc0 + np.repeat(s[:, j], 16) * mm)
    a = dc.exact_inputs(rng, (32, 64))
    for a0, b0, cnt in ((16, 0, 1), (16, 0, 11), (16, 0, 16), (1, 1, 15), (9, 9, 7)):
        want = a.copy()
        for k in range(cnt):
            want[a0 + k] += np.repeat(s[:, b0 + k], 16) * mm
        assert np.array_equal(dc.emu_fmac_range(a, src, mm, a0, b0, cnt), want)
    for c0, cnt, j in ((0, 16, 0), (0, 9, 13), (3, 12, 2)):
        want = a[:16].copy()
        want[c0:c0 + cnt] += np.repeat(a[c0:c0 + cnt].reshape(cnt, 4, 16)[:, :, j], 16, axis=1) * mm
        assert np.array_equal(dc.emu_fmac_self(a[:16], mm, c0, cnt, j), want)
    got = dc.emu_dots(acc0, acc1, src, m)
    dot = lambda acc, ks, lanes: acc + sum(np.repeat(s[:, ln], 16) * m[k] for k, ln in zip(ks, lanes))
    want = [dot(acc0, range(6), range(6)), dot(acc0, range(12), range(12)), dot(acc0, range(15), range(15)),
            dot(acc0, range(6), range(6)), dot(acc1, range(6), range(6, 12)),
            dot(acc0, range(0, 12, 2), range(0, 12, 2)), dot(acc1, range(1, 12, 2), range(1, 12, 2)),
            acc0 + np.repeat(s[:, 0::2].sum(axis=1), 16) * m[0], acc1 + np.repeat(s[:, 1::2].sum(axis=1), 16) * m[0]]
    assert np.array_equal(got, np.stack(want))
    assert np.array_equal(dc.emu_wave_sum(src), np.full(64, src.sum())) and dc.emu_wave_sum(src.astype(np.float32)).dtype == np.float32
    x = dc.full_mantissa(rng, 64)
    x[17] = np.nan
    assert np.array_equal(dc.emu_wave_max(x), np.full(64, np.nanmax(x)))
    f = dc.f32_exact_inputs(rng).astype(np.float64)
    assert np.array_equal(dc.emu_dot(f[0], f[1], f[2:], range(6)).astype(np.float32).astype(np.float64), dc.emu_dot(f[0], f[1], f[2:], range(6)))


def test_wave_sum_order_matters_on_full_mantissa_inputs():
    """The ordered emulation is a real constraint: a left-to-right sum of the same 64 numbers differs from it somewhere."""
    rng = np.random.default_rng(dc.SEED + 1)
    x = dc.full_mantissa(rng, (8, 64))
    assert any(dc.emu_wave_sum(v)[0] != np.add.reduce(v) for v in x)


def test_reference_solution_and_error_measures():
    rng = np.random.default_rng(dc.SEED + 2)
    A = dc.spd(rng, 12, 1e11)
    xs = rng.standard_normal((12, 2))
    B = (A.astype(np.longdouble) @ xs.astype(np.longdouble)).astype(np.float64)
    case = dict(A=A, B=B.T.copy(), live=dc.prefix(12), cond=1e11)
    x, kappa = dc.reference(case)
    assert 1e10 < kappa < 1e13
    res = np.abs(A.astype(np.longdouble) @ x - B).max()
    assert res <= 2.0 ** -60 * np.abs(A).sum(axis=1).max() * np.abs(x).max()              # a longdouble solution, not an fp64 one
    bwd, fwd = dc.errors(case, x.astype(np.float64))
    assert bwd <= 1.0 and fwd <= 1.0
    wrong = x.astype(np.float64) * (1.0 + 1e-3)
    assert dc.errors(case, wrong)[0] > dc.BWD and dc.errors(dict(case), np.full((12, 2), np.nan)) == (np.inf, np.inf)


TABLES = ([(name, dc.ldl_table, nm) for name, nm in dc.LDL_SHAPES.items()] + [("dpph_ldl_8_1_dadd", lambda n, m: dc.ldl_dadd_table(), (8, 1)),
          ("dpph_ldl2", lambda n, m: dc.ldl2_table(), (32, 1))] + [(name, dc.gj_table, nm) for name, nm in dc.GJ_SHAPES.items()])


@pytest.mark.parametrize("name,table,nm", TABLES, ids=[t[0] for t in TABLES])
def test_restatements_stay_within_an_eighth_of_the_bounds(name, table, nm):
    cases = table(*nm)
    N = nm[0]
    assert len(cases) >= N + 3 and {c["live"] for c in cases} >= {dc.prefix(n) for n in range(1, N + 1)}
    gj = name in dc.GJ_SHAPES
    worst_b = worst_f = 0.0
    for c in cases:
        idx = dc.live_idx(c)
        outside = [i for i in range(N) if i not in idx]
        assert not c["A"][outside].any() and not c["A"][:, outside].any() and not c["B"][:, outside].any()
        x, bad = (dc.gj_restatement(c["A"], c["B"], c["live"]) if gj else dc.ldl_restatement(c["A"], c["B"], c["live"], c.get("dadd", 0.0)))
        assert bad == 0 and not x[:, outside].any()
        bwd, fwd = dc.errors(c, x[:, idx].T)
        worst_b, worst_f = max(worst_b, 0.0 if gj else bwd), max(worst_f, fwd)
    print(f"{name}: restatement backward {worst_b:.3f} N u, forward {worst_f:.3f} kappa N u over {len(cases)} cases")
    assert worst_b <= dc.RESTATEMENT_SHARE * dc.BWD and worst_f <= dc.RESTATEMENT_SHARE * dc.FWD
    assert worst_f > 0.0                                                                  # the bound is looked at, not vacuous


def test_bad_pivot_cases_report_through_the_restatements():
    for N, M, nF, piv in ((16, 1, 16, (0, 8, 15)), (6, 6, 6, (0, 3, 5)), (32, 1, 24, (3, 16, 23))):
        cases, expect = dc.bad_pivot_cases(N, M, nF, piv, 1)
        got = [dc.ldl_restatement(c["A"], c["B"], c["live"])[1] != 0 for c in cases]
        assert got == expect and expect.count(True) == len(piv) + 2
        if N <= 16:
            assert [dc.gj_restatement(c["A"], c["B"], c["live"])[1] != 0 for c in cases] == expect
    for j in (0, 8, 15):                                                                  # the pivot met at j is the planted one
        A = dc.indefinite(np.random.default_rng(j), 16, j)
        a = np.tril(A).copy()
        for p in range(j):
            f = a[:, p] / a[p, p]
            for c in range(p + 1, 16):
                a[c:, c] -= f[c:] * a[c, p]
        assert abs(a[j, j] + 1.0) < 1e-12 and all(np.linalg.eigvalsh(A[:p, :p]).min() > 0.0 for p in range(1, j + 1))     # after j positive ones


def test_guard_cases_and_restatement():
    cases = dc.guard_cases()
    assert {c["use"] for c in cases} == {0, 1, 2, 3} and {c["rank5"] for c in cases} == {None, 0, 1}
    for c in cases:
        for f in range(2):
            K = dc.pinned(c["K"][f], int(c["dd"][f]))
            on = bool((c["use"] >> f) & 1)
            x, bad = dc.gj_restatement(K, np.eye(6), 0x3F, on=on, dmin=1e-12)
            assert bad == int(on and c["rank5"] == f)
            if on and c["rank5"] != f:
                assert np.abs(x.T @ K - np.eye(6)).max() < 1e-9
            assert 1e-4 < np.abs(c["K"][f]).max() < 30.0


def test_harness_builds_and_exports_every_launcher():
    lib = dc.harness()
    for name, spec in dc.LAUNCHERS.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(spec["ins"]) + len(spec["outs"]) + 2
    from linearmpchumanoid_amd import build as hipbuild
    assert hipbuild.DPP_HARNESS_SO != hipbuild.SO and "harness" in hipbuild.DPP_HARNESS_SO
