"""Per-robot controller parameters (include/lmh.h, lmh_set_params) without a GPU: the three entry points are exported, the record
layout of the header and of capi.PARAM_FIELDS agree, and the Python side refuses bad fields before it would call the library."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lmh.h")).read()


def test_library_exports_the_three_entry_points(hip_lib):
    from linearmpchumanoid_amd import capi
    for name in ("lmh_set_params", "lmh_params_per_instance", "lmh_get_params"):
        assert hasattr(hip_lib, name), name
        assert name in capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, _header()), f"{name} is not declared in include/lmh.h"


def test_record_layout_of_the_header_matches_param_fields():
    from linearmpchumanoid_amd import capi
    src = _header()
    stride = int(re.search(r"#define\s+LMH_PARAM_STRIDE\s+(\d+)", src).group(1))
    offs = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+LMH_PARAM_OFF_(\w+)\s+(\d+)", src)}
    assert stride == capi.PARAM_STRIDE == 20
    assert offs == capi.PARAM_FIELDS
    assert sorted(offs.values()) == list(range(19))                # dense, the pad alone is left over
    # the record keeps lmh_config's own order of these fields
    cfg_order = [n for n, _ in capi.LmhConfig._fields_ if n in capi.PARAM_FIELDS]
    assert cfg_order == sorted(capi.PARAM_FIELDS, key=capi.PARAM_FIELDS.get)


def _config():
    """an lmh_config filled by hand (no library call): field k of the per-robot ones holds 10 + k"""
    from linearmpchumanoid_amd import capi
    cfg = capi.LmhConfig()
    for name, off in capi.PARAM_FIELDS.items():
        setattr(cfg, name, 10.0 + off)
    return cfg


def test_records_broadcast_scalars_and_keep_the_config():
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import param_records
    cfg = _config()
    B = 5
    rec = param_records(cfg, B, mu=0.4, kp_joints=np.arange(B) + 100.0)
    assert rec.shape == (B, capi.PARAM_STRIDE) and rec.dtype == np.float64
    assert (rec[:, capi.PARAM_FIELDS["mu"]] == 0.4).all()
    assert np.array_equal(rec[:, capi.PARAM_FIELDS["kp_joints"]], np.arange(B) + 100.0)
    for name, off in capi.PARAM_FIELDS.items():
        if name not in ("mu", "kp_joints"):
            assert (rec[:, off] == getattr(cfg, name)).all(), name
    assert (rec[:, 19] == 0.0).all()


@pytest.mark.parametrize("fields, word", [
    (dict(kp_knees=1.0), "unknown"),                               # no such field
    (dict(dt=1e-3), "unknown"),                                    # a per-handle field
    (dict(mu=[0.5, 0.6]), "length"),                               # B = 4
    (dict(w_joints=np.ones((4, 1))), "length"),
    (dict(kd_feet=float("nan")), "finite"),
    (dict(w_force=[1.0, 1.0, float("inf"), 1.0]), "finite"),
])
def test_python_side_refusals_come_before_the_library_call(monkeypatch, fields, word):
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController

    class Lib:                                                     # stands in for the library: any call through it is a failure
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")

    ctl = BatchedController.__new__(BatchedController)             # no device is needed up to the refusal
    ctl.B, ctl.cfg, ctl._h = 4, _config(), None
    monkeypatch.setattr(capi, "lib", lambda: Lib())
    with pytest.raises(ValueError, match=word):
        ctl.set_params(**fields)
