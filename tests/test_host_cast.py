"""The C++ host shell's stand-alone test program of the cast layer behind the cost layer (cloud_merger_amd/host/cast_tests.cpp),
run as tests/test_host_mcl.py runs its program: on the CPU the NodeConfig keys cast / cast_bearings / cast_range / cast_plain
and their refusals, among them a file with cast 1 and no cost layer, and both walks of csrc/cm_cast_math.hpp (the code the
kernel compiles) against a walk written with `/`; with "gpu", a node run through two frames with cast 1 whose cast_rays() and
cast_info() equal what the library returns for the same calls, in both modes."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/cast_tests"], check=True)
    return os.path.join(HOST, "bin", "cast_tests")


def test_config_keys_and_the_arithmetic(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
