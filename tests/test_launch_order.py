"""libjxl_amd/csrc/host/jxh_launch_order.h, the order in which jxlhip_run_entropy_batch emits the lane kernel's workgroups,
on the CPU: tests/c/launch_order_kats.cc built as a stand-alone program with AddressSanitizer + UBSan.
  (a) kats: the order is a permutation, estimates are non-increasing along it, equal estimates keep frame order, the waves
      of a unit stay adjacent and ascending; one unit, one section, zero-byte sections and 65 535 frames do not overflow; the
      queue replay gives a hand-worked case of five sections on two lanes;
  (b) slots: the finishing times of eight 1024 x 768 streams (seeds 177-184, d1.0, from their true token counts) go through
      two launches of 20 workgroups on 24 slots; dispatched by the estimate the second launch ends no later than in frame
      order."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("launch_order")), "launch_order_kats")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    os.path.join(ROOT, "tests", "c", "launch_order_kats.cc"), "-o", out], check=True)
    return out


def test_the_order_and_the_queue_replay(program):
    r = subprocess.run([program, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "launch order kats passed" in r.stdout


def test_the_estimated_order_frees_the_slots_no_later_than_frame_order(built, program, tmp_path):
    import jxlo
    import launch_order_streams as S
    J = built
    path = os.path.join(str(tmp_path), "streams.txt")
    with open(path, "w") as f:
        for seed in S.SEEDS:
            rows = S.sections_of(J, jxlo, 1024, 768, seed)
            assert len(rows) == 12 and (rows[:, 2] > 0).all()
            f.write("stream %d\n" % len(rows) + "".join("%d %d %d\n" % tuple(r) for r in rows.tolist()))
    r = subprocess.run([program, "slots", path], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count("the second launch ends at") == 3
