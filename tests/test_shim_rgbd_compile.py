"""CPU: the RGB-D drop-in (shim/Frame_rgbd_orbfe.cc, orbfe_glue::frame_rgbd in shim/orbfe_glue.h)
compiles with -Werror against include/orbfe.h and the stand-in headers of tests/shim_stubs/, the way
tests/test_shim_compile.py compiles the other shims; a drift of orbfe_frame_rgbd's signature or of
orbfe_rgbd_params fails it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "shim", "Frame_rgbd_orbfe.cc")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _gxx(src, include, extra=()):
    return subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                           "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", include, "-I",
                           os.path.join(ROOT, "shim"), *extra, src], capture_output=True, text=True, timeout=120)


def test_rgbd_shim_compiles():
    r = _gxx(SRC, os.path.join(ROOT, "include"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_glue_frame_rgbd_instantiates(tmp_path):
    """The OpenCV-free glue alone, instantiated with plain stand-in types as the C-ABI consumer does."""
    src = tmp_path / "use_glue.cpp"
    src.write_text("""
#include <cstdint>
#include <vector>
#include "orbfe_glue.h"
struct Key { float a[5]; int b[2]; };
struct Rows { std::vector<uint8_t> v; uint8_t* rows(int cap) { v.resize((size_t)cap * 32); return v.data(); }
              void keep(int n) { v.resize((size_t)n * 32); } };
int run(orbfe_extractor* h, const uint8_t* img, const uint16_t* depth) {
    std::vector<Key> k, ku; Rows d; std::vector<float> ur, dp;
    const float dist[5] = {0.1f, 0, 0, 0, 0};
    const orbfe_rgbd_params p = orbfe_glue::rgbd_params(500, 500, 320, 240, dist, 5, 40.f, 1.f / 5000.f);
    return orbfe_glue::frame_rgbd(h, img, 640, 480, 640, depth, ORBFE_DEPTH_U16, 1280, p, k, ku, d, ur, dp);
}
""")
    r = _gxx(str(src), os.path.join(ROOT, "include"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_rgbd_shim_compile_catches_abi_drift(tmp_path):
    """The check bites: against a copy of orbfe.h whose orbfe_frame_rgbd lacks depth_out, or whose
    orbfe_rgbd_params lacks depth_factor, the shim fails to compile."""
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for k, (old, new, word) in enumerate([
            ("int cap, int* n, float* uright, float* depth_out);", "int cap, int* n, float* uright);", "orbfe_frame_rgbd"),
            ("    float depth_factor;\n} orbfe_rgbd_params;", "} orbfe_rgbd_params;", "depth_factor")]):
        assert hdr.count(old) == 1
        inc = tmp_path / f"include{k}"
        inc.mkdir()
        (inc / "orbfe.h").write_text(hdr.replace(old, new))
        r = _gxx(SRC, str(inc))
        assert r.returncode != 0 and word in r.stderr
