"""The metrics record of lmh_rollout_metrics on the host: the layout constants against include/lmh.h, the exported symbols, and
linearmpchumanoid_amd.metrics -- the numpy statement of the record's definition that the GPU tests hold the kernel to.  No GPU."""
import os
import re

import numpy as np
import pytest

from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd import metrics as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def header_defines(prefix):
    src = open(os.path.join(ROOT, "include", "lmh.h")).read()
    return {n: int(v) for n, v in re.findall(r"#define\s+(" + prefix + r"\w*)\s+(\d+)\b", src)}


def sample(q=None, flags=0, tau=0.0, f=0.0, com=(0.0, 0.0), ref=(0.0, 0.0), B=1):
    """one trace sample [B,180] with the words the fold reads set (q: the first state words)"""
    s = np.zeros((B, capi.TRACE_STRIDE))
    if q is not None:
        q = np.atleast_2d(np.asarray(q, dtype=np.float64))
        s[:, :q.shape[1]] = q
    s[:, 96:120], s[:, 120:132] = tau, f
    s[:, 96 + 66], s[:, 96 + 67], s[:, 96 + 72], s[:, 96 + 75] = com[0], com[1], ref[0], ref[1]
    s[:, 178] = flags
    return s


def test_constants_agree_with_the_header_and_tile_the_record():
    d = header_defines("LMH_METRICS_")
    assert d.pop("LMH_METRICS_STRIDE") == capi.METRICS_STRIDE == 208
    assert {n[len("LMH_METRICS_OFF_"):].lower(): v for n, v in d.items()} == {n: o for n, (o, _) in capi.METRICS_FIELDS.items()}
    assert len(d) == len(capi.METRICS_FIELDS) == 13
    spans = sorted([(o, o + int(np.prod(s, dtype=np.int64))) for o, s in capi.METRICS_FIELDS.values()] + list(capi.METRICS_PADS))
    assert spans[0][0] == 0 and spans[-1][1] == capi.METRICS_STRIDE
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))      # no gap, no overlap


def test_the_two_symbols_are_exported(hip_lib):
    assert hasattr(hip_lib, "lmh_metrics_reset") and hasattr(hip_lib, "lmh_rollout_metrics")
    assert "lmh_metrics_reset" in capi.EXPORTS and "lmh_rollout_metrics" in capi.EXPORTS
    # a null handle is refused before anything else is looked at
    assert hip_lib.lmh_metrics_reset(None, None, 0.0, 0.0, None) == -2 and hip_lib.lmh_rollout_metrics(None, None, None, None, None, 1, None, None) == -2


def test_identity_record():
    r = hm.identity(3, 0.2, [0.5, 0.6, INF])
    f = {k: r[:, o] if s == () else r[:, o:o + s[0]] for k, (o, s) in capi.METRICS_FIELDS.items()}
    assert (f["count"] == 0).all() and (f["first_flag"] == -1).all() and (f["first_fall"] == -1).all()
    assert (f["z_min"] == 0.2).all() and f["tilt_max"].tolist() == [0.5, 0.6, INF]
    assert (f["xmin"] == INF).all() and (f["wmin"] == INF).all() and (f["xmax"] == -INF).all() and (f["wmax"] == -INF).all()
    for k in ("tau_maxabs", "tau_sq", "err_maxabs", "err_sq"):
        assert (f[k] == 0).all() and not np.signbit(f[k]).any()
    assert all((r[:, a:b] == 0).all() for a, b in capi.METRICS_PADS)
    with pytest.raises(ValueError):
        hm.identity(2, NAN, 0.5)
    with pytest.raises(ValueError):
        hm.identity(2, 0.1, [0.5, NAN])


def test_a_nan_pose_is_down_and_thresholds_compare_as_stated():
    q = np.zeros(6)
    q[2] = 0.3
    never = hm.identity(1)
    for bad in (2, 3, 4):
        p = q.copy()
        p[bad] = NAN
        tr = np.stack([sample(q), sample(p), sample(q)])
        assert hm.fold_trace(never, tr)[0, 2] == 1                  # -inf / inf thresholds: only a NaN pose is down
    tr = np.stack([sample(q)] * 3)
    assert hm.fold_trace(never, tr)[0, 2] == -1
    assert hm.fold_trace(hm.identity(1, 0.3, INF), tr)[0, 2] == -1  # q[2] >= Z_MIN: up
    assert hm.fold_trace(hm.identity(1, np.nextafter(0.3, 1), INF), tr)[0, 2] == 0
    for word in (3, 4):
        for v in (0.5, -0.5):
            p = q.copy()
            p[word] = v
            tr = np.stack([sample(q), sample(q), sample(p)])
            assert hm.fold_trace(hm.identity(1, -INF, 0.5), tr)[0, 2] == -1     # |.| <= TILT_MAX: up
            assert hm.fold_trace(hm.identity(1, -INF, np.nextafter(0.5, 0)), tr)[0, 2] == 2
    p = q.copy()
    p[5] = 3.0                                                      # yaw does not count
    assert hm.fold_trace(hm.identity(1, -INF, 0.5), np.stack([sample(p)]))[0, 2] == -1


def test_nans_are_ignored_by_the_extrema_and_poison_the_sums():
    xs = [1.0, NAN, -2.0, 3.0, NAN]
    tr = np.stack([sample(q=[x], tau=x, f=x, com=(x, 0.0)) for x in xs])
    r = hm.fold_trace(hm.identity(1), tr)
    from linearmpchumanoid_amd.controller import BatchedController
    f = BatchedController.split_metrics(r)
    assert f["xmin"][0, 0] == -2.0 and f["xmax"][0, 0] == 3.0 and f["wmin"][0, 0] == -2.0 and f["wmax"][0, 11] == 3.0
    assert f["tau_maxabs"][0, 0] == 3.0 and f["err_maxabs"][0, 0] == 3.0 and f["err_maxabs"][0, 1] == 0.0
    assert np.isnan(f["tau_sq"][0]).all() and np.isnan(f["err_sq"][0, 0]) and f["err_sq"][0, 1] == 0.0
    assert f["count"][0] == 5 and f["first_fall"][0] == -1          # word 0 is not a pose word the fall looks at
    # the extrema are np.fmin / np.fmax of the samples (values; a tie of +0 and -0 keeps the accumulator's)
    rng = np.random.default_rng(3)
    tr = np.zeros((40, 2, capi.TRACE_STRIDE))
    tr[:, :, :60] = rng.normal(size=(40, 2, 60))
    tr[rng.integers(0, 40, 30), rng.integers(0, 2, 30), rng.integers(0, 60, 30)] = NAN
    g = BatchedController.split_metrics(hm.fold_trace(hm.identity(2), tr))
    assert np.array_equal(g["xmin"], np.fmin.reduce(tr[:, :, :60], axis=0)) and np.array_equal(g["xmax"], np.fmax.reduce(tr[:, :, :60], axis=0))
    z = hm.fold_trace(hm.identity(1), np.stack([sample(q=[0.0]), sample(q=[-0.0])]))
    assert not np.signbit(z[0, 8]) and not np.signbit(z[0, 68])


def test_flag_bits_16_and_32_do_not_count():
    tr = np.stack([sample(flags=fl) for fl in (0, 16, 32, 48, 16 | 4, 1)])
    assert hm.fold_trace(hm.identity(1), tr)[0, 1] == 4
    assert hm.fold_trace(hm.identity(1), tr[:4])[0, 1] == -1
    for bit in (1, 2, 4, 8):
        assert hm.fold_trace(hm.identity(1), np.stack([sample(), sample(flags=bit)]))[0, 1] == 1


def test_folding_in_two_parts_is_folding_the_whole_and_sums_run_in_tick_order():
    rng = np.random.default_rng(11)
    B, n = 3, 50
    tr = rng.normal(size=(n, B, capi.TRACE_STRIDE)) * np.exp(rng.normal(size=(n, B, 1)) * 8.0)      # magnitudes far apart: the order of a sum shows
    tr[:, :, 178] = 0.0
    tr[37, 1, 178] = 4.0
    tr[:, :, 2] = np.abs(tr[:, :, 2]) + 1.0
    tr[20, 2, 2] = 0.5
    r0 = hm.identity(B, 0.75, INF)
    whole = hm.fold_trace(r0, tr)
    parts = hm.fold_trace(hm.fold_trace(r0, tr[:23]), tr[23:])
    assert whole.tobytes() == parts.tobytes()
    assert np.array_equal(r0, hm.identity(B, 0.75, INF))            # the record given is not written
    assert whole[:, 0].tolist() == [n] * B and whole[:, 1].tolist() == [-1, 37, -1] and whole[:, 2].tolist() == [-1, -1, 20]
    acc = np.zeros((B, 24))
    for s in tr:
        acc += s[:, 96:120] * s[:, 96:120]
    assert whole[:, 176:200].tobytes() == acc.tobytes()
    backwards = np.zeros((B, 24))
    for s in tr[::-1]:
        backwards += s[:, 96:120] * s[:, 96:120]
    assert backwards.tobytes() != acc.tobytes()                     # ... and the draw is one where the order matters
    e = np.zeros(B)
    for s in tr:
        d = s[:, 96 + 67] - s[:, 96 + 75]
        e += d * d
    assert whole[:, 203].tobytes() == e.tobytes()
    with pytest.raises(ValueError):
        hm.fold_trace(r0, tr[:, :2])


def test_split_metrics_and_summarise_on_a_known_record():
    from linearmpchumanoid_amd.controller import BatchedController
    rec = np.arange(2 * 208, dtype=np.float64).reshape(2, 208)
    f = BatchedController.split_metrics(rec)
    assert f["count"].dtype == np.int64 and [int(f[k][1]) for k in ("count", "first_flag", "first_fall")] == [208, 209, 210]
    assert f["z_min"][0] == 3 and f["tilt_max"][0] == 4 and f["xmin"].shape == (2, 60) and f["xmin"][0, 0] == 8 and f["xmax"][0, 59] == 127
    assert f["wmin"][0, 0] == 128 and f["wmax"][0, 11] == 151 and f["tau_maxabs"][0, 0] == 152 and f["tau_sq"][0, 23] == 199
    assert f["err_maxabs"][0].tolist() == [200, 201] and f["err_sq"][1].tolist() == [208 + 202, 208 + 203]
    r = hm.identity(2, 0.2, 0.5)
    r[:, 0] = [400, 0]
    r[0, 1], r[0, 2] = 99, 249
    r[0, 176:200] = 2.0
    r[0, 152:176] = np.arange(24)
    r[0, 202:204] = [4.0, 16.0]
    r[0, 8 + 2] = 0.21
    s = hm.summarise(r, 1e-3)
    assert s["ticks"].tolist() == [400, 0] and s["effort"][0] == 1e-3 * 48.0 and s["effort"][1] == 0.0
    assert s["rms_error"][0].tolist() == [0.1, 0.2] and np.isnan(s["rms_error"][1]).all()
    assert s["peak_torque"].tolist() == [23.0, 0.0] and s["min_base_height"].tolist() == [0.21, INF]
    assert s["t_first_flag"][0] == 100 * 1e-3 and s["t_first_fall"][0] == 250 * 1e-3 and np.isnan(s["t_first_flag"][1]) and np.isnan(s["t_first_fall"][1])
