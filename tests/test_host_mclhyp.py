"""The C++ host shell's stand-alone test program of the localisation layer's hypotheses and recovery
(cloud_merger_amd/host/mclhyp_tests.cpp), run as tests/test_host_mclbeam.py runs its program: the NodeConfig keys mcl_hyp /
mcl_hyp_bins / mcl_hyp_max / mcl_recovery / mcl_kld and their refusals on the CPU, among them a file with mcl_hyp 1 and no
mcl 1, cm_mcl_kld_bound by hand, and, with "gpu", a node run through three frames whose mcl_info(), mcl_hypotheses() and
mcl_hyp_info() equal what the library returns for the same calls."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/mclhyp_tests"], check=True)
    return os.path.join(HOST, "bin", "mclhyp_tests")


def test_config_keys_and_the_kld_bound(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
