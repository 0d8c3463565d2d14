"""libjxl_amd/csrc/host/jxh_modular_launch_plan.h, the launch plan of jxlhip_modular_run_batch, on the CPU:
tests/c/modular_launch_plan_kats.cc built as a stand-alone program with AddressSanitizer + UBSan. The program holds the
loops of the HIP layer as they were before the header (stream order, LDS caps, kernel form, lanes, LDS and grid; the pass
geometry; the grids of the transform / output launches) and compares field for field.
  (a) kats: synthetic descriptors. 0, 1, 4096, 4097, 8193, 8194 and 131104 streams (the first count at 64 lanes) over frames
      of uneven size, under every legal and several illegal overrides; equal sample counts across frames keep frame, then
      stream order; trees of 0, 1, 2048 and 2049 nodes and tables of 8192 and 8193 words, alone and mixed, give the largest
      cap that fits; WP and REFS each set by one stream of the last frame; block counts of 65535, 65536 and 131071, heights
      of 4096 and 4097, a row pass 5000 high, an unsqueeze launch and an empty list expand to grids that cover every block
      once and exceed no limit;
  (b) real: the thirteen streams of test_kats.modular_upload_streams through MakeModPlan and BuildModStreams with fake
      bases, each alone and all as one set;
  (c) plan: the plan of real streams as text (tests/test_gpu_modular_launch_plan.py holds the HIP layer to it)."""
import os
import subprocess

import pytest

from test_kats import modular_upload_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_programs = {}


def modular_launch_plan_program(tmp_path_factory, sanitize=True):
    """The program, built once per session: under the sanitizers for the tests here; plain for the GPU test, which only wants
    what it prints."""
    if sanitize not in _programs:
        out = os.path.join(str(tmp_path_factory.mktemp("modular_launch_plan")), "modular_launch_plan_kats")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
        subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-Wall", "-Wno-unused-function", "-Wno-subobject-linkage",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "modular_launch_plan_kats.cc"), "-o", out, "-lpthread"],
                       check=True)
        _programs[sanitize] = out
    return _programs[sanitize]


def plan_of(program, files, lanes=None):
    """What the program plans for the frames in `files`: the words of the [modular pack] line as a dict of strings."""
    r = subprocess.run([program, "plan"] + (["--lanes", str(lanes)] if lanes else []) + list(files), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    words = r.stdout.split()
    assert words[:2] == ["modular", "pack"], r.stdout[-3000:]
    return dict(zip(words[2::2], words[3::2]))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return modular_launch_plan_program(tmp_path_factory)


def test_the_rules_of_the_plan_on_synthetic_descriptors(program):
    r = subprocess.run([program, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "modular launch plan kats passed" in r.stdout


def test_the_plan_of_real_streams(built, program, tmp_path):
    """Mode real on the thirteen streams; mode plan on three of them: a plain frame alone is one stream per wave without the
    weighted predictor; beside the frame with it and the one whose tree reads the previous channel the form has both."""
    J = built
    files = {}
    for name, args, data in modular_upload_streams(J):
        files[name] = os.path.join(str(tmp_path), name + ".jxl")
        open(files[name], "wb").write(data)
        if args:
            files[name] += ":" + args[0]
    r = subprocess.run([program, "real"] + list(files.values()), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "modular launch plan real passed: 13 frames" in r.stdout
    pack = plan_of(program, [files["plain"]])
    assert pack == {"streams": pack["streams"], "lanes": "1", "workgroups": pack["streams"], "lds": pack["lds"], "tree_cap": pack["tree_cap"],
                    "table_cap": pack["table_cap"], "form": "plain"}
    assert int(pack["lds"]) == 128 + 16 * int(pack["tree_cap"]) + 4 * int(pack["table_cap"]) + 256
    three = [files[k] for k in ("plain", "rct_wp_alpha", "predictors_prev_channel_lz77")]
    both = plan_of(program, three, lanes=64)
    alone = [plan_of(program, [f]) for f in three]
    assert [p["form"] for p in alone] == ["plain", "wp", "refs"] and both["form"] == "wp+refs"
    assert int(both["streams"]) == sum(int(p["streams"]) for p in alone) and both["lanes"] == "64"
    assert int(both["workgroups"]) == (int(both["streams"]) + 63) // 64
    assert int(both["tree_cap"]) == max(int(p["tree_cap"]) for p in alone) and int(both["table_cap"]) == max(int(p["table_cap"]) for p in alone)
