"""CPU test of the C ABI's host layer under the address and undefined-behaviour sanitizers: tests/host/capi_host_main.cpp is a program of
its own, compiled together with lmh_capi.hip (the kernel launchers are stubs that abort, lmh_kernels.hip is not compiled) and run as a
child process.  It reaches no HIP runtime function, so it does the same on a machine with a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_layer_refusals_and_record_files_under_sanitizers(tmp_path):
    """lmh_create's refusals keep their text and their order (one row per rule of validate_config, rows that break two rules), every entry
    point refuses a null handle in its own words, and summary / log / trace files round-trip and are refused when damaged: wrong magic,
    version, dtype or width, a truncated header, a payload that does not match the header, a buffer too small, zero ticks."""
    exe = tmp_path / "capi_host_main"
    sanitize = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *sanitize,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "capi_host_main.cpp"),
                           os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_capi.hip"), "-o", str(exe)])
    records = tmp_path / "records"
    records.mkdir()
    run = subprocess.run([str(exe), str(records)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "all host-layer checks held" in run.stdout
    assert "Sanitizer" not in run.stdout and "runtime error" not in run.stdout, run.stdout
