"""The C++ host shell's stand-alone test program of the localisation layer's beam model
(cloud_merger_amd/host/mclbeam_tests.cpp), run as tests/test_host_mcl.py runs its program: the NodeConfig keys mcl_beam /
mcl_beam_model / mcl_beam_mix / mcl_beam_plain and their refusals on the CPU, among them a file with mcl_beam 1 and no mcl 1,
both extended walks of csrc/cm_cast_math.hpp (the code the kernel compiles) against a walk written with `/`, and, with "gpu", a
node run through three frames in both walk modes whose mcl_info() and mcl_beam_info() equal what the library returns for the
same calls."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/mclbeam_tests"], check=True)
    return os.path.join(HOST, "bin", "mclbeam_tests")


def test_config_keys_and_arithmetic(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
