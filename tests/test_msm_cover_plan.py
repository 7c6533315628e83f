"""Sanitizer leg of the exact-cover window plan, host only: the plan header (csrc/zl_msm_cover_plan.h: the split, the digits, the placement of a digit in the
uniform bucket sets and the plan's proof obligation) walked by a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
(tests/c/msm_cover_plan.cpp).  No device, no library, nothing loaded into this process."""
import os
import subprocess

from openzl_amd import build as zb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_msm_cover_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "msm_cover_plan"
    cxx = os.path.join(zb._LLVM, "clang++")  # the host compiler beside hipcc: the program holds no device code
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "openzl_amd", "csrc"), os.path.join(ROOT, "tests", "c", "msm_cover_plan.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "msm_cover_plan: OK" in out.stdout, (out.stdout, out.stderr)
