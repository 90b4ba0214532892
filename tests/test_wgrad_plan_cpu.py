"""The exact-f32 weight-gradient plan against the list of kernel instances the library builds (csrc/wgrad_plan.hpp): host code,
compiled and run on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_gradient_plan_reaches_exactly_the_listed_instances(tmp_path):
    """tools/wgrad_plan_check.cpp walks wgrad_plan over Nout 1..1024 x K 1..4096 (plain form) and every shape the DMA form takes:
    every ok plan lands on a (kernel, tiles per wave, prefetch class) that wgrad.hip instantiates, and each of the 17 listed
    instances is reached by some shape."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "wgrad_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mr-gnas_amd", "csrc"),
                            os.path.join(ROOT, "tools", "wgrad_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "17 instances, 0 shapes without an instance, 0 instances never reached" in run.stdout, run.stdout[-2000:]
