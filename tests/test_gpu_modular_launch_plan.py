"""jxlhip_modular_run_batch feeds the launch planner (libjxl_amd/csrc/host/jxh_modular_launch_plan.h) what the frames say
and launches what it plans: five frames that disagree on size, channels, the weighted predictor and the previous-channel
properties decode exactly as one set, in both orders and at 1 (the planner's own choice), 4 and 64 streams per wave, and
the numbers of the [modular pack] line are those the stand-alone program of tests/test_modular_launch_plan.py plans for the
same streams; the plan is made once per set and again when a frame, the set or JXLHIP_MOD_LANES changes."""
import os
import re

import numpy as np
import pytest

from local_streams import lossless_image as _lossless_image
from test_modular_launch_plan import modular_launch_plan_program, plan_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed(built, tmp_path_factory):
    """The five frames: (image, stream, file of the stream). decode_lossless is the single-context decode (one context,
    jxlhip_modular_run, no override): it returns the image here, so a batch that returns the image equals it too."""
    J = built
    spec = [((40, 30), 1, 0),
            ((300, 280), 3, J.LOSSLESS_RCT | J.LOSSLESS_WP),
            ((64, 64), 4, J.LOSSLESS_PREV_CHANNEL),
            ((300, 280), 3, J.LOSSLESS_SQUEEZE | J.LOSSLESS_RCT),
            ((520, 260), 3, J.LOSSLESS_LOCAL_RCT | J.LOSSLESS_LOCAL_PALETTE)]
    d = tmp_path_factory.mktemp("mixed_modular")
    forced = os.environ.pop("JXLHIP_MOD_LANES", None)
    try:
        out = []
        for i, ((w, h), channels, flags) in enumerate(spec):
            img = _lossless_image(J, w, h, channels, seed=60 + i)
            data = J.encode_lossless(img, flags, seed=i)
            assert np.array_equal(J.decode_lossless(data, num_channels=channels), img), i
            path = os.path.join(str(d), "m%d.jxl" % i)
            open(path, "wb").write(data)
            out.append((img, data, path))
        return out
    finally:
        if forced is not None:
            os.environ["JXLHIP_MOD_LANES"] = forced


class _Set:
    """Contexts with a frame each; run() decodes them as one batch and returns the [modular pack] lines the call printed."""

    def __init__(self, J, capfd):
        self.J, self.capfd, self.ctxs, self.frames, self.imgs = J, capfd, [], [], []

    def put(self, k, item):
        """Frame `item` into context k (a new one behind the last)."""
        img, data, _ = item
        if k == len(self.ctxs):
            self.ctxs.append(self.J.HipContext())
            self.frames.append(None)
            self.imgs.append(None)
        f = self.J.ModFrame(data)
        self.ctxs[k].set_output_format(2, img.shape[2])
        self.ctxs[k].upload_modular(f)
        if self.frames[k] is not None:
            self.frames[k].close()
        self.frames[k], self.imgs[k] = f, img

    def run(self, order):
        self.capfd.readouterr()
        self.J.run_modular_batch([self.ctxs[k] for k in order])
        for k in order:
            r, status, _ = self.ctxs[k].modular_status()
            assert r == 0 and not any(status), (k, status)
            got = self.ctxs[k].pixels()
            assert got.shape == self.imgs[k].shape and np.array_equal(got, self.imgs[k]), "frame %d: %d samples differ" % (k, int((got != self.imgs[k]).sum()))
        said = re.findall(r"^\[modular pack\] (.*)$", self.capfd.readouterr().err, re.M)
        return [dict(zip(s.split()[0::2], s.split()[1::2])) for s in said]

    def close(self):
        for c in self.ctxs:
            c.close()
        for f in self.frames:
            f.close()


@pytest.mark.parametrize("lanes", [None, 4, 64])
def test_a_mixed_set_is_launched_as_planned_and_decodes_exactly(built, mixed, tmp_path_factory, monkeypatch, capfd, lanes):
    program = modular_launch_plan_program(tmp_path_factory, sanitize=False)
    monkeypatch.setenv("JXLHIP_PACK_DEBUG", "1")
    if lanes:
        monkeypatch.setenv("JXLHIP_MOD_LANES", str(lanes))
    else:
        monkeypatch.delenv("JXLHIP_MOD_LANES", raising=False)
    s = _Set(built, capfd)
    try:
        for k, item in enumerate(mixed):
            s.put(k, item)
        # all five in their order and reversed; without the previous-channel frame; without the weighted predictor's too
        for order, form in (([0, 1, 2, 3, 4], "wp+refs"), ([4, 3, 2, 1, 0], "wp+refs"), ([0, 1, 3, 4], "wp"), ([0, 3, 4], "plain")):
            said = s.run(order)
            want = plan_of(program, [mixed[k][2] for k in order], lanes)
            print(lanes, order, want)
            assert said == [want]
            assert want["form"] == form and want["lanes"] == str(lanes or 1)
    finally:
        s.close()


def test_the_plan_is_made_once_per_set_and_again_when_something_changed(built, mixed, tmp_path_factory, monkeypatch, capfd):
    program = modular_launch_plan_program(tmp_path_factory, sanitize=False)
    monkeypatch.setenv("JXLHIP_PACK_DEBUG", "1")
    monkeypatch.delenv("JXLHIP_MOD_LANES", raising=False)
    s = _Set(built, capfd)
    try:
        for k in range(3):
            s.put(k, mixed[k])
        first = plan_of(program, [mixed[k][2] for k in (0, 1, 2)])
        assert s.run([0, 1, 2]) == [first]
        assert s.run([0, 1, 2]) == []  # the same set: the plan is re-used
        s.put(1, mixed[3])  # another frame into one of its contexts
        assert s.run([0, 1]) == [plan_of(program, [mixed[0][2], mixed[3][2]])]  # a shorter set
        changed = plan_of(program, [mixed[k][2] for k in (0, 3, 2)])
        assert changed != first and s.run([0, 1, 2]) == [changed]  # the first set again, over the new frame
        assert s.run([0, 1, 2]) == []
        monkeypatch.setenv("JXLHIP_MOD_LANES", "4")
        forced = plan_of(program, [mixed[k][2] for k in (0, 3, 2)], 4)
        assert forced["lanes"] == "4" and s.run([0, 1, 2]) == [forced]
        assert s.run([0, 1, 2]) == []
        monkeypatch.delenv("JXLHIP_MOD_LANES")
        assert s.run([0, 1, 2]) == [changed]
    finally:
        s.close()
