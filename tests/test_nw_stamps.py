"""CPU: the HIP-free half of the timed NW executes' device-side stamps
(nw_stamps.hpp: which plans are stamped, the stamp pool's slot bookkeeping,
the complemented-begin decoding, ticks to ms, the totals behind
saln_nw_plan_kernel_time) through a stand-alone program
(tests/host/nw_stamps_check.cpp).  Header-only: no library, no HIP include
path.  The device half is tests/test_nw_timing_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stamp_bookkeeping_and_decoding(tmp_path):
    exe = str(tmp_path / "nw_stamps_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "sequencealigning_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "nw_stamps_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok"
