"""jxlhip_run_entropy_batch feeds the launch planner (libjxl_amd/csrc/host/jxh_lane_plan.h) what the frames say: for the
twelve mixed frames of tests/test_gpu_entropy_order.py, in the sparse regime and under JXLHIP_LANES=64, the workgroup order
and estimates that jxlhip_debug_entropy_order reports and the numbers of the [pack] line are those the stand-alone program of
tests/test_lane_plan.py plans for the same streams and the device's CU count."""
import os
import re

import pytest
import torch

from test_gpu_entropy_order import _streams
from test_lane_plan import lane_plan_program, plan_of

pytestmark = pytest.mark.gpu


def test_the_launch_is_what_the_planner_says_for_these_streams(built, tmp_path_factory, tmp_path, monkeypatch, capfd):
    J = built
    program = lane_plan_program(tmp_path_factory, sanitize=False)
    streams = _streams(J)
    files = []
    for i, s in enumerate(streams):
        files.append(os.path.join(str(tmp_path), "f%02d.jxl" % i))
        open(files[-1], "wb").write(s)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = [J.Frame(s) for s in streams]
    ctxs = [J.HipContext() for _ in streams]
    try:
        for name in ("JXLHIP_WG_ORDER", "JXLHIP_LANES", "JXLHIP_GALIAS", "JXLHIP_A6"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("JXLHIP_PACK_DEBUG", "1")
        for lanes in (None, "64"):
            if lanes:
                monkeypatch.setenv("JXLHIP_LANES", lanes)
            for c, f in zip(ctxs, frames):
                c.upload(f)
            capfd.readouterr()
            J.run_entropy_batch(ctxs)
            unit, est = ctxs[0].entropy_order()
            for c in ctxs:
                c.sync()
            said = re.findall(r"^\[pack\] (.*)$", capfd.readouterr().err, re.M)
            assert len(said) == 1, said
            words = said[0].split()
            said = dict(zip(words[0::2], words[1::2]))
            assert said.pop("waves/wg") == "1"
            pack, want_unit, want_est, wave_lanes = plan_of(program, files, cus, lanes)
            print(lanes, pack)
            assert said == pack
            assert unit.tolist() == want_unit and est.tolist() == want_est
            assert len(wave_lanes) == len(want_unit) == int(pack["workgroups"])
            assert (pack["lanes/wave"] == "64") == (lanes is not None)
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()
