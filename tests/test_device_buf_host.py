"""The handle's owning buffer types (ikflow_amd/csrc/device_buf.h) on the host: tests/device_buf_host.cpp fakes the six HIP names the
header uses, is built with the address and undefined-behaviour sanitizers and runs as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_buf_host_program(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "device_buf_host")
    # the sanitizer runtimes are linked statically: a shared libasan refuses to start when anything else is preloaded into the child
    # (it must come first in the initial library list), and the environment the suite runs in may preload a library of its own
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "ikflow_amd", "csrc"), os.path.join(ROOT, "tests", "device_buf_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "device_buf_host ok" in r.stdout, r.stdout + r.stderr
