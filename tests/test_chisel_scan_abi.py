"""The scan integrate at the boundary (no GPU): the built library exports the two entry points, the header still compiles
as C99 with the new struct in use, and the C++ mirror compiles with the new members of PointCloudMapChisel."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")
SYMBOLS = ("plvs_hip_tsdf_chisel_integrate_scan", "plvs_hip_tsdf_chisel_integrate_scans_dev")


def test_library_exports_the_scan_entry_points():
    path = os.path.join(LIB_DIR, "libplvs_hip.so")
    assert os.path.exists(path), "build it first: make -C plvs_amd/csrc (or __graft_entry__.build())"
    import torch  # noqa: F401  (same load order as the product: torch's HIP runtime first)
    lib = ctypes.CDLL(path)
    for s in SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
    lib.plvs_hip_abi_version.restype = ctypes.c_int
    assert lib.plvs_hip_abi_version() == 1          # appended to, not re-versioned


def test_python_struct_matches_the_header():
    from plvs_amd.tsdf import ScanCamera
    assert ctypes.sizeof(ScanCamera) == 32 and [f[0] for f in ScanCamera._fields_] == \
        ["fx", "fy", "cx", "cy", "width", "height", "near_plane", "far_plane"]


def test_header_is_plain_c_with_the_scan_entry_points(tmp_path):
    src = """#include "plvs_hip.h"
int main(void) {
  plvs_scan_camera cam = {1.0f, 1.0f, 0.5f, 0.5f, 4, 4, 0.1f, 5.0f};
  float depth[16] = {0};
  unsigned char bgr[48] = {0};
  float Twc[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  /* a null handle is an argument error, not a crash */
  int a = plvs_hip_tsdf_chisel_integrate_scan(0, depth, 16, bgr, 12, 3, &cam, Twc, 0, 0.05f);
  int b = plvs_hip_tsdf_chisel_integrate_scans_dev(0, depth, bgr, 3, &cam, Twc, 1, 0, 0.05f, 0);
  return (a == PLVS_ERR_INVALID_ARG && b == PLVS_ERR_INVALID_ARG && sizeof(plvs_scan_camera) == 32) ? 0 : 1;
}
"""
    c = str(tmp_path / "scan_abi.c")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-c", c, "-o",
                    str(tmp_path / "scan_abi.o")], check=True)
    subprocess.run(["gcc", str(tmp_path / "scan_abi.o"), "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "scan_abi")], check=True)
    subprocess.run([str(tmp_path / "scan_abi")], check=True)      # (argument checks only: no device is touched)


def test_cpp_mirror_compiles_with_the_scan_members(tmp_path):
    src = """#include "plvs_hip.hpp"
int use(PLVS2hip::PointCloudMapChisel& m, const PLVS2hip::Image32F& depth, const PLVS2hip::Image8U& color,
        const PLVS2hip::SE3f& Twc) {
  m.SetDepthCameraModel(517.3f, 516.5f, 318.6f, 255.3f, 640, 480);
  m.InsertDepthScanColor(depth, color, Twc, 42u);
  m.InsertDepthScanColor(depth, color, Twc, 42u, 4);
  PLVS2hip::PointCloudMapChisel::Input d;
  d.type = PLVS2hip::PointCloudMapChisel::Input::kColorAndDepthImages;
  d.imgDepth = depth;
  d.imgColor = color;
  d.Twc = Twc;
  m.InsertData(d);
  return m.UpdateMap();
}
"""
    c = str(tmp_path / "scan_mirror.cpp")
    open(c, "w").write(src)
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INC, "-c", c, "-o",
                    str(tmp_path / "scan_mirror.o")], check=True)
