"""The scaffolding in tests/helpers.py that the GPU tests stand on, checked on the CPU: the environment and the result of a child
process, bit identity, and the horizon time.  The children import nothing of the project."""
import numpy as np
import pytest
import torch

from helpers import RANK_VARS, bench_env, child_env, horizon_time, run_probe, same_bits


@pytest.fixture
def parent_env(monkeypatch):
    monkeypatch.setenv("LMH_VARIANT", "x")
    monkeypatch.setenv("LMH_DIAG", "1")
    monkeypatch.setenv("RANK", "3")


@pytest.mark.parametrize("variant", ["", None, "poison"])
def test_child_env_chooses_the_build_and_drops_the_diagnostics(parent_env, variant):
    env = child_env(variant)
    assert "LMH_DIAG" not in env
    assert env.get("LMH_VARIANT") == (variant or None)
    assert env["RANK"] == "3" and env["PATH"]                       # everything else is inherited


def test_child_env_extra_wins_over_the_inherited_value(parent_env):
    env = child_env("poison", {"RANK": "5", "LMH_DIAG": "2", "NEW": "y"})
    assert env["RANK"] == "5" and env["LMH_DIAG"] == "2" and env["NEW"] == "y" and env["LMH_VARIANT"] == "poison"
    assert child_env("poison", {"LMH_VARIANT": "noedge"})["LMH_VARIANT"] == "noedge"


def test_bench_env_has_no_rank_variables(parent_env, monkeypatch):
    for k in RANK_VARS:
        monkeypatch.setenv(k, "1")
    env = bench_env({"LMH_BENCH_DEVICE": "0"})
    assert set(RANK_VARS) == {"RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"} and not set(RANK_VARS) & set(env)
    assert env["LMH_BENCH_DEVICE"] == "0" and env["LMH_VARIANT"] == "x"        # the build is not bench_env's business


def test_run_probe_returns_the_last_json_line():
    assert run_probe("print('noise'); print('{\"a\": 1}'); print('{\"a\": 2}')", timeout=60) == {"a": 2}


def test_run_probe_fails_with_the_childs_stderr():
    with pytest.raises(AssertionError, match="boom"):
        run_probe("import sys; sys.stderr.write('boom'); sys.exit(3)", timeout=60)


@pytest.mark.parametrize("variant", ["", "poison"])
def test_run_probe_child_sees_the_requested_build(parent_env, variant):
    code = "import json, os, sys; print(json.dumps({'v': os.environ.get('LMH_VARIANT'), 'd': os.environ.get('LMH_DIAG'), 'argv': sys.argv[1:]}))"
    assert run_probe(code, variant, timeout=60, args=("7",)) == {"v": variant or None, "d": None, "argv": ["7"]}


def test_same_bits():
    a = np.array([0.0, 1.5, -2.0, 3.0])
    assert same_bits(a, a.copy())
    assert same_bits(a.reshape(2, 2).T, np.ascontiguousarray(a.reshape(2, 2).T))      # a strided view against its packed copy
    assert not same_bits(np.array([0.0]), np.array([-0.0]))
    n = np.array([1.0, np.nan])
    assert same_bits(n, n.copy())
    assert not same_bits(n, np.array([1.0, -np.nan]))               # another NaN pattern
    assert not same_bits(a, a.astype(np.float32))
    assert not same_bits(a, a.reshape(2, 2))
    assert not same_bits(a, a + np.array([0.0, 0.0, 0.0, 2.0 ** -51]))


def test_same_bits_on_torch_tensors():
    t = torch.tensor([[0.0, float("nan")], [-1.0, 2.0]], dtype=torch.float64)
    assert same_bits(t, t.clone())
    assert same_bits(t.T, t.T.contiguous())
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bits(t, t.float()) and not same_bits(t, t.reshape(4))
    s = torch.tensor([3, 0, 7], dtype=torch.int32)
    assert same_bits(s, s.clone()) and not same_bits(s, s.long())


@pytest.mark.parametrize("mpc_dt", [1e-3, 1e-2])
def test_horizon_time_gives_back_its_horizon(mpc_dt):
    for N in range(1, 65):
        assert int(horizon_time(N, mpc_dt) / mpc_dt) == N, N
