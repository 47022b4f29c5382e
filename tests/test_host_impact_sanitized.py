"""CPU test of the plastic impact's host layer (lmh_plant_impact_rigid and lmh_rollout_zoh_rigid_impact) under the address and
undefined-behaviour sanitizers: tests/host/impact_host_main.cpp is a program of its own, compiled together with lmh_capi.hip (the kernel
launchers are stubs that abort) exactly as test_host_zoh_rigid_sanitized.py compiles its program, and run as a child process.  It reaches
no HIP runtime function; nothing is loaded into Python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_impact_refuses_without_a_handle_under_sanitizers(tmp_path):
    exe = tmp_path / "impact_host_main"
    sanitize = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *sanitize,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "impact_host_main.cpp"),
                           os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_capi.hip"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "all impact host-layer checks held" in run.stdout
    assert "Sanitizer" not in run.stdout and "runtime error" not in run.stdout, run.stdout
