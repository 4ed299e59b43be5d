"""The C++ host shell's 2-D grid map (cloud_merger_amd/host/grid_tests.cpp): the NodeConfig keys grid_cell / grid_origin /
grid_size / grid_z_band / grid_obstacle_height / grid_min_points on the CPU, and on the GPU a node that reports the table and
the occupancy image of its frame, equal to what the library returns for the same frame."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def grid_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/grid_tests"], check=True)
    return os.path.join(HOST, "bin", "grid_tests")


def test_grid_config_keys(grid_bin, tmp_path):
    r = subprocess.run([grid_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_the_grid(grid_bin, tmp_path):
    r = subprocess.run([grid_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
