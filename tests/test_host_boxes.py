"""The C++ host shell's oriented boxes (cloud_merger_amd/host/box_tests.cpp): the NodeConfig keys cluster_box_angles /
cluster_box_criterion / cluster_box_d_min on the CPU, and on the GPU a node that reports the boxes of its clusters."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def box_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/box_tests"], check=True)
    return os.path.join(HOST, "bin", "box_tests")


def test_box_config_keys(box_bin, tmp_path):
    r = subprocess.run([box_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_boxes(box_bin, tmp_path):
    r = subprocess.run([box_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
