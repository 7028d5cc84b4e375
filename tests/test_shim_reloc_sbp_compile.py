"""CPU: the relocalisation drop-in (shim/Relocalization_orbfe.cc with SearchByProjectionCandidates, the
batched SearchByProjection(F, KF) of one candidates sweep) compiles with -Werror against include/orbfe.h
and the stand-in headers of tests/shim_stubs/, the
way tests/test_shim_rgbd_compile.py compiles the RGB-D shim; a drift of
orbfe_search_by_projection_kf_batch's signature fails it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "shim", "Relocalization_orbfe.cc")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _gxx(src, include, extra=()):
    return subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                           "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", include, "-I",
                           os.path.join(ROOT, "shim"), *extra, src],
                          capture_output=True, text=True, timeout=120)


def test_reloc_shim_compiles():
    r = _gxx(SRC, os.path.join(ROOT, "include"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_reloc_shim_declares_the_batched_search():
    hdr = open(os.path.join(ROOT, "shim", "Relocalization_orbfe.h")).read()
    assert "SearchByProjectionCandidates(" in hdr
    assert "orbfe_search_by_projection_kf_batch(" in open(SRC).read()


def test_reloc_shim_compile_catches_abi_drift(tmp_path):
    """The check bites: against a copy of orbfe.h whose batch entry point lacks kf_idx, or whose
    orbfe_kf_camera lacks Ow, the shim fails to compile."""
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    for k, (old, new, word) in enumerate([
            ("const orbfe_map_point_3d* const* pts, const int32_t* const* kf_idx,\n",
             "const orbfe_map_point_3d* const* pts,\n", "orbfe_search_by_projection_kf_batch"),
            ("    float Ow[3];                     /* camera centre for the distance / viewing checks */\n", "", "Ow")]):
        assert hdr.count(old) == 1
        inc = tmp_path / f"include{k}"
        inc.mkdir()
        (inc / "orbfe.h").write_text(hdr.replace(old, new))
        r = _gxx(SRC, str(inc))
        assert r.returncode != 0 and word in r.stderr
