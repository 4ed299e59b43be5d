"""The C++ host shell's free-space ray casting (cloud_merger_amd/host/ray_tests.cpp): the NodeConfig keys grid_raycast /
grid_min_pass / grid_ray_range on the CPU, and on the GPU a node that reports the ray table and the cleared image of its frame,
equal to known cells and to what the library returns for the same frame."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def ray_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/ray_tests"], check=True)
    return os.path.join(HOST, "bin", "ray_tests")


def test_ray_config_keys(ray_bin, tmp_path):
    r = subprocess.run([ray_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_the_rays(ray_bin, tmp_path):
    r = subprocess.run([ray_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
