"""The flow planner and the cluster form's back-off (ikflow_amd/csrc/flow_plan.h) on the host: tests/flow_plan_host.cpp includes the header
alone - it names no HIP symbol - is built with plain g++ and the address and undefined-behaviour sanitizers and runs as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flow_plan_host_program(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "flow_plan_host")
    # (the sanitizer runtimes are linked statically, see test_device_buf_host.py)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "ikflow_amd", "csrc"), os.path.join(ROOT, "tests", "flow_plan_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "flow_plan_host ok" in r.stdout, r.stdout + r.stderr
