"""The C++ host shell's frame-to-frame registration (cloud_merger_amd/host/align_tests.cpp): the NodeConfig keys align_prev /
align_max_corr / align_normals_k / align_max_iterations on the CPU, and on the GPU a node that reports the motion between two
frames."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def align_bin():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/align_tests"], check=True)
    return os.path.join(HOST, "bin", "align_tests")


def test_align_config_keys(align_bin, tmp_path):
    r = subprocess.run([align_bin, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_reports_alignment(align_bin, tmp_path):
    r = subprocess.run([align_bin, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
