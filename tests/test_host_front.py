"""The C++ host shell's stand-alone test program of the frontier layer behind the plan layer (cloud_merger_amd/host/front_tests.cpp),
run as tests/test_host_plan.py runs its program: the NodeConfig keys map_frontier / map_frontier_max_cost / map_frontier_scales /
map_goal_vehicle on the CPU and, with "gpu", a node that integrates a frame with the plan to the vehicle's own cell and the
frontiers updated behind it, equal to a table worked out by hand and to what the library returns for the same frame."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/front_tests"], check=True)
    return os.path.join(HOST, "bin", "front_tests")


def test_config_keys(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
