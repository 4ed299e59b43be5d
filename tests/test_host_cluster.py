"""The C++ host shell's cluster extraction (cloud_merger_amd/host/cluster_tests.cpp): the NodeConfig keys cluster_tolerance /
cluster_min_size / cluster_max_size on the CPU, and on the GPU a node that reports the clusters of its voxel cloud."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def cluster_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/cluster_tests"], check=True)
    return os.path.join(HOST, "bin", "cluster_tests")


def test_cluster_config_keys(cluster_bin, tmp_path):
    r = subprocess.run([cluster_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_clusters(cluster_bin, tmp_path):
    r = subprocess.run([cluster_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
