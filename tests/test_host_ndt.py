"""The C++ host shell's frame-to-frame registration by NDT (cloud_merger_amd/host/ndt_tests.cpp): the NodeConfig key
align_method and the start-up refusal of ndt without the occupancy flag on the CPU, and on the GPU a node that reports the
motion between two frames."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def ndt_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/ndt_tests"], check=True)
    return os.path.join(HOST, "bin", "ndt_tests")


def test_ndt_config_keys(ndt_bin, tmp_path):
    r = subprocess.run([ndt_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_ndt_alignment(ndt_bin, tmp_path):
    r = subprocess.run([ndt_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
