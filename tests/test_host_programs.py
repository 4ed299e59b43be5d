"""The C++ host shell's stand-alone test programs (cloud_merger_amd/host/<name>_tests.cpp), one per by-product of the node:
each checks its NodeConfig keys on the CPU and, with "gpu", a node that runs the by-product on the GPU."""
import os
import subprocess

import pytest

from cloud_merger_amd import build as cm_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cloud_merger_amd", "host")

PROGRAMS = [
    # keys motion_compensation / time_field; a node that fuses two moving sensors, one with a per-point time field, and
    # publishes the compensated cloud with the stamp it is expressed at
    "motion",
    # keys cluster_tolerance / cluster_min_size / cluster_max_size; a node that reports the clusters of its voxel cloud
    "cluster",
    # keys cluster_box_angles / cluster_box_criterion / cluster_box_d_min; a node that reports the boxes of its clusters
    "box",
    # keys grid_cell / grid_origin / grid_size / grid_z_band / grid_obstacle_height / grid_min_points; a node that reports the
    # table and the occupancy image of its frame, equal to what the library returns for the same frame
    "grid",
    # keys grid_raycast / grid_min_pass / grid_ray_range; a node that reports the ray table and the cleared image of its frame,
    # equal to known cells and to what the library returns for the same frame
    "ray",
    # keys normals_k / normals_viewpoint; a node that reports the normals of its voxel cloud
    "normals",
    # keys align_prev / align_max_corr / align_normals_k / align_max_iterations; a node that reports the motion between two frames
    "align",
    # key align_method and the start-up refusal of ndt without the occupancy flag; a node that reports that motion by NDT
    "ndt",
    # no keys of its own; blocking, pipelined and deferred nodes with every by-product on publish the same messages and tables
    "epilogue",
]


@pytest.fixture(scope="module", params=PROGRAMS)
def program(request):
    cm_build.build()
    subprocess.run(["make", "-C", HOST, "-s", f"bin/{request.param}_tests"], check=True)
    return os.path.join(HOST, "bin", f"{request.param}_tests")


def test_config_keys(program, tmp_path):
    r = subprocess.run([program, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_on_gpu(program, tmp_path):
    r = subprocess.run([program, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
