"""The C++ host shell's stand-alone test program of the rollout layer behind the plan layer (cloud_merger_amd/host/traj_tests.cpp),
run as tests/test_host_plan.py runs its program: the NodeConfig keys traj / traj_limits / traj_footprint / traj_scales /
traj_allow_unknown and the footprint lattice with its cap on the CPU and, with "gpu", a node that integrates a frame with the cost
layer, the plan and the rollout evaluated behind it in the frame epilogue, equal to scores worked out by hand and to what the
library returns for the same frame; the empty results and error() texts for a goal or a vehicle outside the window."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/traj_tests"], check=True)
    return os.path.join(HOST, "bin", "traj_tests")


def test_config_keys_and_lattice(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
