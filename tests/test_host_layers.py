"""The stand-alone test program of the layer table behind the occupancy map (cloud_merger_amd/host/layers_tests.cpp), run as
tests/test_host_cast.py runs its program. It has no GPU part: csrc/cm_map_layers.hpp holds no HIP, and the program drives its
state machine on the CPU — every layer through an absent ancestor at each depth, its own configure call, an integration, a
load, a cost update, a plan update, a merge, the localisation layer's three causes, a failed producer and a fresh result —
and compares each refusal with a literal string. tests/test_map_layer_texts.py walks the library through the same causes."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")


@pytest.fixture(scope="module")
def program():
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", "bin/layers_tests"], check=True)
    return os.path.join(HOST, "bin", "layers_tests")


def test_every_layer_through_every_cause(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
