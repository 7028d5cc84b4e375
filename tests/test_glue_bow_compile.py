"""CPU: orbfe_glue::compute_bow (shim/orbfe_glue.h), the OpenCV-free body behind Frame::ComputeBoW,
instantiates with std::map stand-ins for DBoW2::BowVector / DBoW2::FeatureVector under -Werror, the
way tests/test_shim_rgbd_compile.py compiles the RGB-D glue; a drift of orbfe_frame_compute_bow's
signature fails it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

USE = """
#include <cstdint>
#include <map>
#include <vector>
#include "orbfe_glue.h"
typedef std::map<unsigned, double> BowVector;                        // DBoW2::BowVector
typedef std::map<unsigned, std::vector<unsigned> > FeatureVector;    // DBoW2::FeatureVector
int run(const orbfe_vocabulary* voc, const orbfe_frame& F, BowVector& bow, FeatureVector& fv) {
    return orbfe_glue::compute_bow(voc, &F, 4, bow, fv);
}
int run_current(orbfe_extractor* left, uint64_t id, const orbfe_vocabulary* voc, const orbfe_frame& host, BowVector& bow,
                FeatureVector& fv) {
    return orbfe_glue::on_current_frame(left, id, host, [&](const orbfe_frame* F) {
        return orbfe_glue::compute_bow(voc, F, 4, bow, fv);
    });
}
"""


def _gxx(src, include):
    return subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", include, "-I",
                           os.path.join(ROOT, "shim"), src], capture_output=True, text=True, timeout=120)


def test_glue_compute_bow_instantiates(tmp_path):
    src = tmp_path / "use_bow.cpp"
    src.write_text(USE)
    r = _gxx(str(src), os.path.join(ROOT, "include"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_glue_compute_bow_catches_abi_drift(tmp_path):
    """The check bites: against a copy of orbfe.h whose orbfe_frame_compute_bow lacks fv_n it fails."""
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    old = ("int orbfe_frame_compute_bow(const orbfe_vocabulary* voc, const orbfe_frame* F, int32_t levelsup,\n"
           "                            uint32_t* bow_word_ids, double* bow_weights, int32_t* bow_n,\n"
           "                            uint32_t* fv_node_ids, int32_t* fv_offsets, uint32_t* fv_indices, int32_t* fv_n);")
    assert hdr.count(old) == 1
    inc = tmp_path / "include"
    inc.mkdir()
    (inc / "orbfe.h").write_text(hdr.replace(old, old.replace(", int32_t* fv_n);", ");")))
    src = tmp_path / "use_bow.cpp"
    src.write_text(USE)
    r = _gxx(str(src), str(inc))
    assert r.returncode != 0 and "orbfe_frame_compute_bow" in r.stderr
