"""The C++ host shell's normal estimation (cloud_merger_amd/host/normals_tests.cpp): the NodeConfig keys normals_k /
normals_viewpoint on the CPU, and on the GPU a node that reports the normals of its voxel cloud."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def normals_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/normals_tests"], check=True)
    return os.path.join(HOST, "bin", "normals_tests")


def test_normals_config_keys(normals_bin, tmp_path):
    r = subprocess.run([normals_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_normals(normals_bin, tmp_path):
    r = subprocess.run([normals_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
