"""The per-robot metrics record of lmh_rollout_metrics (include/lmh.h) on the host, in numpy: the identity record, the DEFINITION of the
record as a fold of an every-tick trace, and the figures a sweep ranks its robots by.

fold_trace is what the kernel is held to bit for bit (tests/test_gpu_metrics.py), and it is of use on its own to a caller who holds a
trace (lmh_rollout_trace with trace_every = 1, or a file read back with BatchedController.read_trace).  Nothing here touches the device.
"""
import numpy as np

from . import capi

_F = capi.METRICS_FIELDS
# where the folded words are inside one trace sample [state(96) | out(80) | status(4)]
_OUT = capi.STATE_STRIDE
_S_X, _S_W, _S_TAU = slice(0, 60), slice(_OUT + 24, _OUT + 36), slice(_OUT, _OUT + 24)
_S_COM, _S_REF, _S_FLAGS = (_OUT + 66, _OUT + 67), (_OUT + 72, _OUT + 75), _OUT + capi.OUT_STRIDE + 2
COUNTED_FLAGS = capi.FLAG_QP_MAXITER | capi.FLAG_NONFINITE | capi.FLAG_ZMP_RANGE | capi.FLAG_NOT_SPD      # 15: not the informational ones


def _view(rec, name):
    o, s = _F[name]
    return rec[..., o] if s == () else rec[..., o:o + s[0]]


def identity(B, z_min=-np.inf, tilt_max=np.inf):
    """What lmh_metrics_reset writes: [B,208]; z_min / tilt_max scalars or arrays of length B."""
    z, a = np.broadcast_to(np.asarray(z_min, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(tilt_max, dtype=np.float64), (B,))
    if np.isnan(z).any() or np.isnan(a).any():
        raise ValueError("a threshold is NaN")
    rec = np.zeros((B, capi.METRICS_STRIDE), dtype=np.float64)
    _view(rec, "first_flag")[...] = -1.0
    _view(rec, "first_fall")[...] = -1.0
    _view(rec, "z_min")[...] = z
    _view(rec, "tilt_max")[...] = a
    for lo, hi in (("xmin", "xmax"), ("wmin", "wmax")):
        _view(rec, lo)[...] = np.inf
        _view(rec, hi)[...] = -np.inf
    return rec


def _fmin(acc, v):
    """IEEE fmin with the accumulator first: a NaN in v is ignored (acc is never one); of two zeros of different sign acc's is kept"""
    with np.errstate(invalid="ignore"):
        return np.where(v < acc, v, acc)


def _fmax(acc, v):
    with np.errstate(invalid="ignore"):
        return np.where(v > acc, v, acc)


def fold_trace(record, trace):
    """Fold the samples trace[s] (s in order; [n, B, 180], every tick of a launch: trace_every = 1) into a copy of record [B, 208] and
    return it -- the definition of include/lmh.h (lmh_rollout_metrics), word for word.  fold(fold(r, a), b) == fold(r, a ++ b)."""
    rec = np.array(record, dtype=np.float64, copy=True)
    trace = np.asarray(trace, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[1] != capi.METRICS_STRIDE or trace.ndim != 3 or trace.shape[1:] != (rec.shape[0], capi.TRACE_STRIDE):
        raise ValueError("record [B,208] and trace [n,B,180] expected")
    count, first_flag, first_fall = _view(rec, "count"), _view(rec, "first_flag"), _view(rec, "first_fall")
    z_min, tilt_max = _view(rec, "z_min"), _view(rec, "tilt_max")
    with np.errstate(invalid="ignore", over="ignore"):
        for s in trace:
            down = ~(s[:, 2] >= z_min) | ~(np.abs(s[:, 3]) <= tilt_max) | ~(np.abs(s[:, 4]) <= tilt_max)      # a NaN pose is down
            flagged = (s[:, _S_FLAGS].astype(np.int64) & COUNTED_FLAGS) != 0
            first_fall[...] = np.where((first_fall < 0) & down, count, first_fall)
            first_flag[...] = np.where((first_flag < 0) & flagged, count, first_flag)
            for lo, hi, sl in (("xmin", "xmax", _S_X), ("wmin", "wmax", _S_W)):
                _view(rec, lo)[...] = _fmin(_view(rec, lo), s[:, sl])
                _view(rec, hi)[...] = _fmax(_view(rec, hi), s[:, sl])
            err = np.stack([s[:, _S_COM[0]] - s[:, _S_REF[0]], s[:, _S_COM[1]] - s[:, _S_REF[1]]], axis=1)
            for mx, sq, v in (("tau_maxabs", "tau_sq", s[:, _S_TAU]), ("err_maxabs", "err_sq", err)):
                _view(rec, mx)[...] = _fmax(_view(rec, mx), np.abs(v))
                _view(rec, sq)[...] = _view(rec, sq) + v * v                # product and sum rounded separately, in tick order
            count += 1.0
    return rec


def summarise(record, dt):
    """The figures of a record [.., 208] for a control step dt [s]: effort dt * sum_j sum_t tau_j^2, rms_error [.., 2] of the CoM against
    the preview's first sample (x, y), peak_torque max_j max_t |tau_j|, min_base_height, ticks, and t_first_flag / t_first_fall in
    seconds from the reset (the END of the tick that raised it; NaN = never).  Records without a tick give NaN for the RMS."""
    rec = np.asarray(record, dtype=np.float64)
    count, ff, fl = _view(rec, "count"), _view(rec, "first_flag"), _view(rec, "first_fall")
    with np.errstate(invalid="ignore", divide="ignore"):
        rms = np.sqrt(_view(rec, "err_sq") / count[..., None])
    return dict(ticks=count.astype(np.int64), effort=dt * _view(rec, "tau_sq").sum(axis=-1), rms_error=rms,
                peak_torque=_view(rec, "tau_maxabs").max(axis=-1), min_base_height=_view(rec, "xmin")[..., 2],
                t_first_flag=np.where(ff < 0, np.nan, (ff + 1.0) * dt), t_first_fall=np.where(fl < 0, np.nan, (fl + 1.0) * dt))
