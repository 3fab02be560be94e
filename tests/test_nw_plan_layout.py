"""CPU: the NW plan layout (nw_plan_layout.cpp: variants and plan order, mask
packs, op-stream and boundary-column offsets, the stripe layout and work list,
the speculative tables, the refusals) over a fixed set of small batches
(tests/host/nw_plan_layout_dump.cpp), compiled against the in-tree libsaln.so,
byte for byte against tests/golden/nw_plan_layout.txt.  The fixture is the
output of the same program over plan_create as it was before the layout moved
out of nw_host.cpp (that function's body with its device calls cut, behind
nw_plan_layout()'s interface), not the output of the module: an offset that
differs is a behaviour change, to be made on purpose and with the fixture
regenerated from the commit that makes it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_layout_equals_fixture(tmp_path):
    lib = os.path.join(ROOT, "sequencealigning_amd")
    exe = str(tmp_path / "nw_plan_layout_dump")
    # no HIP include path: the module's headers must not need one
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(lib, "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "nw_plan_layout_dump.cpp"), "-L" + lib,
                    "-lsaln", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,/opt/rocm/lib:{lib}",
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "nw_plan_layout.txt"), "rb") as f:
        want = f.read()
    if r.stdout != want:
        got_l, want_l = r.stdout.split(b"\n"), want.split(b"\n")
        diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want_l, got_l)) if w != g][:10]
        assert False, f"{len(got_l)} lines vs {len(want_l)}; first differing (line, want, got): {diff}"
