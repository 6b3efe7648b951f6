"""The local-map part of include/plvs_hip.hpp: tests/host/track_local_smoke.cpp compiles against nothing but the C ABI, refuses the
requests the entries refuse without touching the GPU, and on the GPU prints the same bits as the Python mirror."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "track_local_smoke.cpp")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")


def build(out):
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", out], check=True)


def test_track_local_cpp_mirror_compiles_and_refuses_bad_requests(tmp_path):
    exe = str(tmp_path / "track_local_smoke")
    build(exe)
    r = subprocess.run([exe, "--args-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "args_only ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_track_local_cpp_mirror_matches_python_mirror(tmp_path):
    from plvs_amd import frame
    from plvs_amd.orbmatcher import FrameView
    exe = str(tmp_path / "track_local_smoke")
    build(exe)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    said = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l}
    f32 = np.float32
    cam = dict(K4=[517.306408, 516.469215, 318.643040, 255.313989], mbf=40.0, bounds4=[0, 640, 0, 480], Rcw=np.eye(3, dtype=f32).reshape(-1),
               tcw=[0.1, -0.05, 0.2], Ow=[-0.1, 0.05, -0.2], viewing_cos_limit=0.5, log_scale_factor=f32(np.log(f32(1.2))), n_levels=8,
               line_log_scale_factor=f32(np.log(f32(1.2))), n_line_levels=3)
    points = dict(skip=[0, 0, 0, 0, 0, 1], pos=np.array([0.2, 0.1, 3.0, 0.0, 0.0, -2.0, -9.0, 0.0, 3.0, 0.1, 0.1, 4.0, 0.3, -0.2, 2.5, 0.2, 0.1, 3.0], f32),
                  normal=np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1], f32), min_dist=[0.5, 0.5, 0.5, 0.2, 0.5, 0.5],
                  max_dist=[5.0, 5.0, 20.0, 2.0, 5.0, 5.0], desc=np.full((6, 32), 0x5a, np.uint8))
    lines = dict(skip=[0, 0], start=np.array([-0.5, 0.2, 3.0, 0.5, 0.0, 3.0], f32), end=np.array([0.5, 0.3, 3.5, 0.9, 0.4, -1.0], f32),
                 normal=np.array([0, 0, 1, 0, 0, 1], f32), max_dist=[3.2, 1.6])
    got = frame.is_in_frustum(cam, points, lines)
    bits = lambda a: ["%08x" % v for v in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)]      # noqa: E731
    ints = lambda a: [str(int(v)) for v in a]      # noqa: E731
    assert said["n_to_match"] == [str(got["n_in_view_points"]), str(got["n_in_view_lines"])]
    assert got["n_in_view_points"] >= 1 and got["n_in_view_lines"] >= 1 and list(got["points"]["in_view"][:2]) == [1, 0]
    P, Ls = got["points"], got["lines"]
    assert said["point_in_view"] == ints(P["in_view"]) and said["level"] == ints(P["level"])
    for name, key in (("proj_x", "proj_x"), ("proj_y", "proj_y"), ("proj_xr", "proj_xr"), ("track_depth", "track_depth"), ("view_cos", "view_cos")):
        assert said[name] == bits(P[key]), name
    assert said["line_in_view"] == ints(Ls["in_view"]) and said["line_level"] == ints(Ls["level"])
    for name, key in (("line_proj", "proj"), ("line_proj_xr", "proj_xr"), ("line_view_cos", "view_cos")):
        assert said[name] == bits(Ls[key]), name
    # the search: the frame the program builds around the projection of map point 0
    x = np.array([P["proj_x"][0] + f32(0.5), 600.0], f32)
    y = np.array([P["proj_y"][0] - f32(0.5), 20.0], f32)
    fdesc = np.full((2, 32), 0x5a, np.uint8)
    fdesc[0, 0] = 0x5b
    sf = np.array([1.0, 1.2, 1.44, 1.728, 2.0736, 2.48832, 2.985984, 3.5831808], f32)
    F = FrameView(x, y, np.array([P["level"][0], 0], np.int32), np.array([-1, -1], f32), fdesc, 0.0, 0.0, 0.1, 0.1, sf)
    found = frame.search_local_map(cam, F, None, points, None, th=1.0, far_points=False, th_far=0.0, nn_ratio=0.8)
    assert said["nmatches"] == [str(found["nmatches_points"]), "0"] and said["assigned_points"] == ints(found["assigned_points"])
    assert found["nmatches_points"] == 1 and list(found["assigned_points"]) == [0, -1]
