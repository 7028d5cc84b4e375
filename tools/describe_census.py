#!/usr/bin/env python3
"""Timing-only k_describe ablation build (outputs INVALID): a patched copy of the kernel source,
compiled to variants/liborbfe_descabl.so, so the product source carries no ablation hooks.
  descabl: every slot of a dword-aligned level takes the interior staging path; a slot whose patch
           touches the border has its centre clamped into the interior first (wrong pixels, same
           number of slots, no border staging of any kind). Its k_describe time against the product's
           is the ceiling of what border staging can cost.
usage: python tools/describe_census.py"""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_ros_amd", "csrc")

A1 = "    const int px0 = d.x - DP_R, py0 = d.y - DP_R;\n    d.gx0 = px0 & ~3;\n"
B1 = ("    if ((d.pitch & 3) == 0 && ((((uintptr_t)d.im) & 3) == 0) && L.w >= 64 && L.h >= DP_N) {\n"
      "        d.x = min(max(d.x, DP_R), L.w - DP_R - 10);\n"
      "        d.y = min(max(d.y, DP_R), L.h - DP_R - 1);\n"
      "    }\n")


def patched(src: str) -> str:
    assert src.count(A1) == 1, A1
    return src.replace(A1, B1 + A1)


def main():
    os.makedirs(os.path.join(ROOT, "variants"), exist_ok=True)
    src = open(os.path.join(CSRC, "orbfe_kernels.hip")).read()
    with tempfile.TemporaryDirectory() as d:
        # the sources include ../../include/orbfe.h
        shutil.copytree(CSRC, os.path.join(d, "pkg", "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
        open(os.path.join(d, "pkg", "csrc", "orbfe_kernels.hip"), "w").write(patched(src))
        out = os.path.join(ROOT, "variants", "liborbfe_descabl.so")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                        "-o", out, os.path.join(d, "pkg", "csrc", "orbfe_engine.hip")], check=True)
        print(out)


if __name__ == "__main__":
    main()
