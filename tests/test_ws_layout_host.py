"""csrc/workspace.h under AddressSanitizer and UBSan: tests/host/ws_layout_check.cpp is a stand-alone host program (its own main,
nothing loaded into Python) that walks layouts measuring and carving and touches every byte it was handed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.mark.skipif(not (os.path.exists(CXX) or shutil.which(CXX)), reason="host compiler missing")
def test_ws_layout_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ws_layout_check")
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "open3d-ml_amd", "csrc"),
                            os.path.join(HERE, "host", "ws_layout_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "ws_layout_check ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
