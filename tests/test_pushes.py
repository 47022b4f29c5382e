"""CPU tests of the timed velocity pushes (lmh_set_pushes): the host statement of the push table (trajectories.push_schedule), its
refusals -- the library's own, word for word -- the shared draw, and the constants and symbols of the C ABI.  No GPU here: what the
rollout kernel does with the table is tests/test_gpu_pushes.py."""
import os
import re

import numpy as np
import pytest

from linearmpchumanoid_amd import capi, trajectories as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_push_schedule_sorts_pads_and_broadcasts():
    ticks = np.array([[40, -1, 7, 12], [3, 2, 1, 0], [-1, -1, -1, -1]])
    dv = np.arange(3 * 4 * 30, dtype=np.float64).reshape(3, 4, 30) + 1.0
    rec = T.push_schedule(ticks, dv)
    assert rec.shape == (3, 4, T.PUSH_STRIDE) and rec.dtype == np.float64
    assert rec[0, :, 0].tolist() == [7, 12, 40, -1] and rec[1, :, 0].tolist() == [0, 1, 2, 3] and rec[2, :, 0].tolist() == [-1] * 4
    assert np.array_equal(rec[0, :3, 1:31], dv[0, [2, 3, 0]]) and np.array_equal(rec[1, :, 1:31], dv[1, ::-1])
    assert not rec[0, 3, 1:].any() and not rec[2, :, 1:].any()      # unused records: dv zero
    assert not rec[:, :, 31].any()                                  # the pad word
    # one schedule for every robot: [n] ticks and [n,30] increments give n_sets = 1
    shared = T.push_schedule([9, 4], dv[0, :2])
    assert shared.shape == (1, 2, T.PUSH_STRIDE) and shared[0, :, 0].tolist() == [4, 9]
    assert np.array_equal(shared[0, :, 1:31], dv[0, [1, 0]])
    assert T.push_schedule(ticks, dv, n_instances=3).shape[0] == 3
    assert T.push_schedule([9, 4], dv[0, :2], n_instances=3).shape[0] == 1
    with pytest.raises(ValueError):
        T.push_schedule(ticks, dv[:, :3])                            # shapes disagree


def _two_good_robots(n):
    tk = np.tile(np.arange(n, dtype=np.float64) * 10.0, (3, 1))
    return tk, np.zeros((3, n, 30))


@pytest.mark.parametrize("case,msg", [("fraction", T.PUSH_ERR_TICK), ("negative", T.PUSH_ERR_TICK), ("nan_tick", T.PUSH_ERR_TICK),
                                      ("huge", T.PUSH_ERR_TICK), ("repeat", T.PUSH_ERR_INCREASING), ("inf_dv", T.PUSH_ERR_DV),
                                      ("nan_dv", T.PUSH_ERR_DV)])
def test_push_schedule_refusals_name_the_robot(case, msg):
    tk, dv = _two_good_robots(3)
    if case == "fraction":
        tk[2, 1] = 10.5
    elif case == "negative":
        tk[2, 0] = -2.0
    elif case == "nan_tick":
        tk[2, 2] = np.nan
    elif case == "huge":
        tk[2, 2] = 2.0 ** 31
    elif case == "repeat":
        tk[2, 2] = tk[2, 0]
    elif case == "inf_dv":
        dv[2, 1, 0] = np.inf
    elif case == "nan_dv":
        dv[2, 0, 29] = np.nan
    with pytest.raises(ValueError) as e:
        T.push_schedule(tk, dv)
    assert str(e.value) == "robot 2: " + msg
    T.push_schedule(tk[:2], dv[:2])                                  # the two robots in front of it are fine


def test_push_table_refusals_that_sorting_cannot_produce():
    """push_schedule puts the unused records last, so a used record behind an unused one and descending ticks exist only in a table
    somebody wrote by hand: check_push_records (the rules of lmh_set_pushes on the records as they stand) refuses them."""
    tk, dv = _two_good_robots(3)
    rec = T.push_schedule(tk, dv)
    bad = rec.copy(); bad[1, 1, 0] = -1.0
    with pytest.raises(ValueError) as e:
        T.check_push_records(bad)
    assert str(e.value) == "robot 1: " + T.PUSH_ERR_ORDER
    bad = rec.copy(); bad[2, :, 0] = [20, 10, 30]
    with pytest.raises(ValueError) as e:
        T.check_push_records(bad)
    assert str(e.value) == "robot 2: " + T.PUSH_ERR_INCREASING
    # an unused record's dv is ignored, NaN included
    ok = rec.copy(); ok[0, 2, 0] = -1.0; ok[0, 2, 5] = np.nan
    T.check_push_records(ok)
    with pytest.raises(ValueError) as e:
        T.push_schedule(*_two_good_robots(T.MAX_PUSHES + 1))
    assert str(e.value) == T.PUSH_ERR_COUNT
    T.push_schedule(*_two_good_robots(T.MAX_PUSHES))
    with pytest.raises(ValueError) as e:
        T.push_schedule(tk, dv, n_instances=4)
    assert str(e.value) == T.PUSH_ERR_SETS


def test_refusal_words_are_the_librarys():
    src = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_capi.hip")).read()
    for msg in (T.PUSH_ERR_TICK, T.PUSH_ERR_ORDER, T.PUSH_ERR_INCREASING, T.PUSH_ERR_DV, T.PUSH_ERR_COUNT, T.PUSH_ERR_SETS):
        assert '"%s"' % msg in src, msg


def test_draw_pushes_is_deterministic_per_seed_and_per_robot():
    a = T.draw_pushes(16, 3, (0, 1000), 0.1, 77)
    b = T.draw_pushes(16, 3, (0, 1000), 0.1, 77)
    c = T.draw_pushes(16, 3, (0, 1000), 0.1, 78)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    big = T.draw_pushes(64, 3, (0, 1000), 0.1, 77)
    assert np.array_equal(big[0][:16], a[0]) and np.array_equal(big[1][:16], a[1])       # robot i does not depend on the batch
    assert np.array_equal(c[0][:15], a[0][1:]) and np.array_equal(c[1][:15], a[1][1:])   # one generator per robot: seed + i
    tk, dv = a
    assert tk.shape == (16, 3) and dv.shape == (16, 3, 30) and tk.dtype.kind == "i"
    assert (tk >= 0).all() and (tk < 1000).all() and all(len(set(r.tolist())) == 3 for r in tk)
    assert (np.abs(dv[:, :, 0:2]) <= 0.1).all() and dv[:, :, 0:2].any() and not dv[:, :, 2:].any()
    T.push_schedule(tk, dv)
    few = T.draw_pushes(4, 5, (10, 15), 0.1, 1)[0]
    assert all(sorted(r.tolist()) == [10, 11, 12, 13, 14] for r in few)
    with pytest.raises(ValueError):
        T.draw_pushes(4, 6, (10, 15), 0.1, 1)


def _define(path, name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(path).read(), flags=re.M)
    assert m, (path, name)
    return int(m.group(1))


def test_header_constants_are_the_bindings():
    hdr = os.path.join(ROOT, "include", "lmh.h")
    dev = os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_device.h")
    assert _define(hdr, "LMH_PUSH_STRIDE") == capi.PUSH_STRIDE == T.PUSH_STRIDE == _define(dev, "LMH_PUSH_STRIDE") == 32
    assert _define(hdr, "LMH_MAX_PUSHES") == capi.MAX_PUSHES == T.MAX_PUSHES == 16
    assert capi.PUSH_STRIDE >= 1 + 30                                # tick | dv[30]


def test_push_symbols_are_declared_and_exported(hip_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmh.h")).read(), flags=re.S)
    for name in ("lmh_set_pushes", "lmh_num_pushes", "lmh_pushes_per_instance", "lmh_get_pushes"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in capi.EXPORTS and hasattr(hip_lib, name), name
    # argument checks that need no device: a null handle is refused
    assert hip_lib.lmh_set_pushes(None, None, 0, 1) == -2
    assert hip_lib.lmh_num_pushes(None) == 0 and hip_lib.lmh_pushes_per_instance(None) == 0


def test_set_pushes_needs_both_arrays():
    with pytest.raises(ValueError) as e:
        T.push_schedule([1, 2], None)
    assert "dv" in str(e.value)
