"""Shared by the tests that compile a header of csrc/ into a small host program (test_band_plan_cpu.py,
test_stream_source_cpu.py): where the sources are, and the host compiler of the ROCm toolchain that the library's Makefile
needs anyway."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acids_transforms_amd", "csrc")


def host_compiler():
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    for root in filter(None, roots):
        for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++", "bin/amdclang++"):
            if os.path.exists(os.path.join(root, sub)):
                return os.path.join(root, sub)
    pytest.fail("no host compiler of the ROCm toolchain found under %s" % [r for r in roots if r])


def build(main_cpp, exe):
    """Compiles tests/<main_cpp> against csrc/ into exe, warnings as errors, no HIP runtime."""
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", main_cpp), "-o", exe], check=True)
    return exe
