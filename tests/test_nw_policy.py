"""CPU: the NW variant policy (nw_policy.cpp: choose_variant, fill_path,
stripe_packed, stripe_rows_k, the all-vs-all launch geometry) over a fixed
grid of schemes, query widths and db lengths (tests/host/nw_policy_dump.cpp),
compiled against the in-tree libsaln.so, byte for byte against
tests/golden/nw_policy_grid.txt.  The fixture is the output of the same
program linked against the library as it was before the policy moved out of
nw_kernels.hip: a decision that differs is a behaviour change, to be made on
purpose and with the fixture regenerated from the commit that makes it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policy_grid_equals_fixture(tmp_path):
    lib = os.path.join(ROOT, "sequencealigning_amd")
    exe = str(tmp_path / "nw_policy_dump")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(lib, "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "nw_policy_dump.cpp"), "-L" + lib, "-lsaln",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,/opt/rocm/lib:{lib}", "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "nw_policy_grid.txt"), "rb") as f:
        want = f.read()
    if r.stdout != want:
        got_l, want_l = r.stdout.split(b"\n"), want.split(b"\n")
        diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want_l, got_l)) if w != g][:10]
        assert False, f"{len(got_l)} lines vs {len(want_l)}; first differing (line, want, got): {diff}"
