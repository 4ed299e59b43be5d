"""The C++ host shell's stand-alone test program of the search layer behind the cost layer
(cloud_merger_amd/host/msearch_tests.cpp), run as tests/test_host_match.py runs its program: the NodeConfig keys match_search /
match_search_window / match_search_depth / match_search_capacity and their refusals on the CPU (`match` and `match_search`
together included) and, with "gpu", a node that integrates a first frame under a set pose, receives the second with a set_pose
70 cells off and integrates it under the matched pose, equal to the shift worked out by hand and to what the library returns for
the same calls."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/msearch_tests"], check=True)
    return os.path.join(HOST, "bin", "msearch_tests")


def test_config_keys(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
