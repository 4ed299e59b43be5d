"""The C++ host shell's stand-alone test program of the cost layer over the occupancy map (cloud_merger_amd/host/cost_tests.cpp),
run as tests/test_host_map.py runs its program: the NodeConfig keys map_inflation / map_inflate_unknown on the CPU and, with
"gpu", a node that integrates two frames with the layer updated behind each, equal to known cells and to what the library
returns for the same frames."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/cost_tests"], check=True)
    return os.path.join(HOST, "bin", "cost_tests")


def test_config_keys(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
