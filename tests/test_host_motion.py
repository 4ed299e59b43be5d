"""The C++ host shell's ego-motion compensation (cloud_merger_amd/host/motion_tests.cpp): the NodeConfig keys
motion_compensation / time_field on the CPU, and on the GPU a node that fuses two moving sensors — one with a per-point time
field — publishing the compensated cloud with the stamp it is expressed at."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def motion_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/motion_tests"], check=True)
    return os.path.join(HOST, "bin", "motion_tests")


def test_motion_config_keys(motion_bin, tmp_path):
    r = subprocess.run([motion_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_compensates_moving_sensors(motion_bin, tmp_path):
    r = subprocess.run([motion_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
