"""libjxl_amd/csrc/host/jxh_lane_plan.h, the launch plan of jxlhip_run_entropy_batch's lane kernel, on the CPU:
tests/c/lane_plan_kats.cc built as a stand-alone program with AddressSanitizer + UBSan.
  (a) kats: on hand-made section tables every listed section is in exactly one unit, largest first with equal sizes in group
      order; min_lanes follows the ceiling rule; the waves of a unit share its lanes evenly and stay adjacent in the workgroup
      map; the three regimes of lanes per wave, the decision table of the table forms with every override, and the bounds of
      the six-byte form give the numbers worked out in the program; the device buffer is aligned for the kernel's reads and
      packed into exactly its size; the LDS layout gives the offsets the hand-written trip has as immediates; an empty group
      list, an absent pass, one section and 65 535 frames do not overflow;
  (b) plan: the plan of real streams as text (tests/test_gpu_lane_plan.py holds the HIP layer to it)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_programs = {}


def lane_plan_program(tmp_path_factory, sanitize=True):
    """The program, built once per session: under the sanitizers for the tests here; plain for the GPU test, which only wants
    what it prints."""
    if sanitize not in _programs:
        out = os.path.join(str(tmp_path_factory.mktemp("lane_plan")), "lane_plan_kats")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
        subprocess.run(["g++", "-std=c++17", "-O0"] + flags + ["-Wall", "-Wno-unused-function", "-Wno-subobject-linkage",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "lane_plan_kats.cc"), "-o", out, "-lpthread"],
                       check=True)
        _programs[sanitize] = out
    return _programs[sanitize]


def plan_of(program, files, cus, lanes=None):
    """What the program plans for the streams in `files`: (the [pack] numbers as a dict of strings, wg_unit, wg_est, wave_lanes)."""
    r = subprocess.run([program, "plan"] + list(files) + ["--cus", str(cus)] + (["--lanes", str(lanes)] if lanes else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert [l.split()[0] for l in lines] == ["pack", "wg_unit", "wg_est", "wave_lanes"], r.stdout[-3000:]
    words = lines[0].split()[1:]
    return (dict(zip(words[0::2], words[1::2])),) + tuple([int(v) for v in l.split()[1:]] for l in lines[1:])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return lane_plan_program(tmp_path_factory)


def test_the_rules_of_the_plan_on_hand_made_tables(program):
    r = subprocess.run([program, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "lane plan kats passed" in r.stdout


def test_the_plan_of_real_streams(built, program, tmp_path):
    """Mode plan on streams of the parser's: a frame of six sections alone spreads over a lane per section; with a frame of
    two histogram sets and one of two passes there are five units, in the dense regime a workgroup each."""
    J = built
    files = []
    for i, kw in enumerate((dict(), dict(num_histograms=2), dict(num_passes=2))):
        files.append(os.path.join(str(tmp_path), "f%d.jxl" % i))
        open(files[-1], "wb").write(J.encode_rgb8(J.synth_image(520, 300, seed=40 + i), **kw))
    pack, unit, est, wave_lanes = plan_of(program, files[:1], 256)
    assert pack == {"units": "1", "sections": "6", "lanes(min)": pack["lanes(min)"], "lanes/wave": "1", "workgroups": "6", "lds": pack["lds"],
                    "tables": "lds8"}
    assert unit == [0] * 6 and len(set(est)) == 1 and wave_lanes == [1] * 6
    pack, unit, est, wave_lanes = plan_of(program, files, 256, lanes=64)
    assert (pack["units"], pack["sections"], pack["lanes/wave"], pack["workgroups"]) == ("5", "24", "64", "5")
    assert sorted(unit) == list(range(5)) and est == sorted(est, reverse=True) and sum(wave_lanes) == 24
