"""The motion-model part of include/plvs_hip.hpp: tests/host/track_motion_smoke.cpp compiles against nothing but the C ABI, refuses the
requests the entry refuses without touching the GPU, and on the GPU gives the golden assignments of tests/track_motion_scenario.py."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import track_local_scenario as L
from tests import track_motion_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "track_motion_smoke.cpp")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build(out):
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", out], check=True)


def write_inputs(path, inp):
    fr, P, pts, ln = inp["frame"], inp["poses"], inp["points"], inp["lines"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()      # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()        # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a, np.uint8).tobytes()         # noqa: E731
    kl = np.ascontiguousarray(fr["keylines"])
    assert kl.dtype.itemsize == 68
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", len(fr["x"]), len(pts["valid"]), len(kl), len(ln["valid"]), S.N_LEVELS, S.N_LINE_LEVELS))
        f.write(f32(fr["x"]) + f32(fr["y"]) + i32(fr["octave"]) + f32(fr["u_right"]) + u8(fr["desc"]) + f32(fr["cur_angle"]) + f32(S.SCALE_FACTORS))
        f.write(kl.tobytes() + u8(fr["line_desc"]) + f32(fr["u_right_start"]) + f32(fr["u_right_end"]) + f32(S.LINE_SCALE_FACTORS) + f32(S.LINE_INV_SIGMA2))
        f.write(f32(P["q_cw"]) + f32(P["tcw"]) + f32(P["Rcw"]) + f32(P["Ow"]) + f32(P["q_lw"]) + f32(P["tlw"]) + f32([P["mb"], P["mbf"]]) + f32(P["bounds4"])
                + f32(P["K4"]) + f32([L.MAX_DIAG, L.GRID_W_INV, L.GRID_H_INV]))
        f.write(u8(pts["valid"]) + f32(pts["pos"]) + i32(pts["octave"]) + f32(pts["angle"]) + u8(pts["desc"]) + u8(pts["has_obs"]))
        f.write(u8(ln["valid"]) + f32(ln["start"]) + f32(ln["end"]) + f32(ln["max_dist"]) + i32(ln["octave"]) + f32(ln["angle"]) + u8(ln["desc"]) + u8(ln["has_obs"]))


def test_track_motion_cpp_mirror_compiles_and_refuses_bad_requests(tmp_path):
    exe = str(tmp_path / "track_motion_smoke")
    build(exe)
    r = subprocess.run([exe, "--args-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "args_only ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_track_motion_cpp_mirror_gives_the_golden_assignments(tmp_path):
    exe = str(tmp_path / "track_motion_smoke")
    build(exe)
    g = np.load(os.path.join(GOLDEN, "track_motion_reference.npz"))
    with open(os.path.join(GOLDEN, "track_motion_reference_facts.json")) as f:
        facts = json.load(f)["facts"]
    runs = [(S.inputs(), ("15", "1", "0", "0"), g[S.search_key(15.0, 1, 0, "neither")], g[S.line_key(1, 0, "neither")],
             dict(nmatches_points=facts["nmatches"][S.search_key(15.0, 1, 0, "neither")], nmatches_lines=facts["nmatches"][S.line_key(1, 0, "neither")],
                  larger_line_search_used=0, th_used=15.0, point_retries=0, line_retries=0))]
    for kind in ("few_points", "few_lines"):
        runs.append((S.policy_inputs(kind), ("15", "1", "20", "10"), g[f"policy_{kind}_assigned_points"], g[f"policy_{kind}_assigned_lines"], facts["policy"][kind]))
    for k, (inp, args, want_p, want_l, want) in enumerate(runs):
        path = str(tmp_path / f"inputs{k}.bin")
        write_inputs(path, inp)
        r = subprocess.run([exe, path, *args], check=True, capture_output=True, text=True)
        said = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l}
        assert said["assigned_points"] == [str(int(v)) for v in want_p] and said["assigned_lines"] == [str(int(v)) for v in want_l]
        assert said["nmatches"] == [str(want["nmatches_points"]), str(want["nmatches_lines"])]
        assert said["flags"] == ["0", "0", str(want["larger_line_search_used"]), "%g" % want["th_used"]]
        assert said["stats"] == [str(1 + want["point_retries"]), str(want["point_retries"]), str(want["line_retries"]), "0"]
        if k == 0:
            assert said["proj_valid_points"] == [str(int(v)) for v in g["p_proj_valid"]]
            assert said["u"] == ["%08x" % v for v in g["p_u"].view(np.uint32)]
            assert said["line_proj"] == ["%08x" % v for v in g["l_proj6"].reshape(-1).view(np.uint32)]
