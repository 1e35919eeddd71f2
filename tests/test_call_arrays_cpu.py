"""The counting of CallArrays (pnec_amd/csrc/pnec_internal.hpp), without a GPU.

An entry point of the C ABI lists each of its arrays once; in HOST space CallPlan (pnec_amd/csrc/pnec_call_plan.hpp, no
HIP) turns that list into the regions of the two staging buffers and their totals.  tools/call_arrays_host.cc replays
the list of every entry point at small sizes (1 and 3 pairs, 1 and 2 poses per pair, per-correspondence lengths that are
no multiple of 8, one point, one and three pyramid levels with and without a shared `prev`, detection with and without
current points) and checks that the regions are disjoint, in order and hold their copies, that the totals with every
array given are the ones the entry points wrote out by hand before CallArrays existed, never more with arrays left out,
and that kept and preloaded outputs take room and travel as documented.  Built for the host under the address and
undefined-behaviour sanitizers and run as a program of its own: nothing is loaded into Python.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the entry points that stage through CallArrays, as tools/call_arrays_host.cc names their lists
LISTS = ("solve", "cost_function", "pose_covariance", "residuals", "triangulate", "relative_scale", "patch_covariance",
         "image_pyramid_level", "patch_track", "detect_keypoints", "front_stage", "ransac_eigensolver", "solve_pipeline")


def test_every_entry_points_list_is_counted_as_it_was_by_hand(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = str(tmp_path / "call_arrays_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "call_arrays_host.cc"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "call arrays: every list counted" in r.stdout and "FAIL" not in r.stdout
    lines = r.stdout.splitlines()
    for name in LISTS:
        assert any(line.startswith("ok   " + name + "(") for line in lines), name


def test_the_planning_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "pnec_amd", "csrc", "pnec_call_plan.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", "<vector>"], includes
