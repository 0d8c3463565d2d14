"""The Modular kernels held to the reading of tests/modular_np.py: k_modular_streams in its four forms, k_modular_rct,
k_modular_unsqueeze and k_modular_palette decode the cases of tests/modular_cases.py from hand-made descriptors
(tests/modular_desc.py) through the public entry points jxlhip_modular_upload / _run / _status / _download_buffer, and every
channel buffer must equal the reading's exactly. No front-end of the product takes part: the bytes are the reading's
writer's, the bit position of the sample data is the one it reported, trees, weighted-predictor values and alias entries are
the reading's own. tests/test_modular_np.py holds the same cases on both CPU front-ends and builds these descriptors
without a device.

The expected channels come from modular_cases.build(), which runs the Python model once per case and session."""
import re

import pytest

import modular_cases as C
import modular_desc as D

pytestmark = pytest.mark.gpu

PLAIN = tuple("pred%d" % p for p in range(14) if p != 6) + ("static_s3", "static_s5", "rects")
WP = ("pred6", "props") + tuple(n for n in C.NAMES if n.startswith("wp_"))
# name -> (cases, the form of k_modular_streams<WP, REFS> the launch must take, cases placed at x0 in {1, 3}, y0 = 2)
STREAM_SETS = {
    "plain": (PLAIN, "plain", ("rects", "pred13", "static_s5")),
    "wp": (WP, "wp", ("wp_distinct_leaf", "props")),
    "refs": (("prev", "pred1"), "refs", ("prev",)),
    "wp+refs": (("prev_wp", "pred2"), "wp+refs", ()),
    # two streams of one tree and code: at 64 lanes the wave stages both in LDS (the sets above mix trees in a wave: global)
    "wp shared": (("props", "props"), "wp", ()),
    "refs shared": (("prev", "prev", "prev"), "refs", ("prev",)),
}
TRANSFORMS = tuple(n for n in C.GPU_NAMES if n.split("_")[0] in ("rct", "squeeze", "palette"))
PLACED_TRANSFORMS = ("rct_perm3", "rct_wrap6", "squeeze_17x9", "squeeze_5x3", "palette_nb3_8", "palette_rct")


def decode(J, frame, capfd):
    """Uploads and runs the frame; -> the words of the [modular pack] line. Status, end bits and every buffer are checked."""
    desc, keep = frame.descriptor()
    ctx = J.HipContext()
    try:
        capfd.readouterr()
        ctx.upload_modular_desc(desc, len(frame.streams), 4, 4)
        ctx.run_modular()
        r, status, end_bits = ctx.modular_status()
        assert r == 0 and not any(status), status
        assert end_bits == frame.end_bits  # the writer's length, stream by stream
        frame.check(ctx)
        said = re.findall(r"^\[modular pack\] (.*)$", capfd.readouterr().err, re.M)
        assert len(said) == 1, said
        return dict(zip(said[0].split()[0::2], said[0].split()[1::2]))
    finally:
        ctx.close()
        del keep


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("name", list(STREAM_SETS))
def test_stream_kernel_forms_return_the_readings_channels(built, monkeypatch, capfd, name, lanes):
    names, form, placed = STREAM_SETS[name]
    monkeypatch.setenv("JXLHIP_PACK_DEBUG", "1")
    monkeypatch.setenv("JXLHIP_MOD_LANES", str(lanes))
    frame = D.Frame()
    for n in names:
        frame.add(C.build(n), placed=n in placed)
    if name.endswith("shared"):
        assert len(frame.trees) == 1 and len(frame.streams) == len(names)
    else:
        assert len(frame.trees) == len(names)
    said = decode(built, frame, capfd)
    assert said["form"] == form and said["lanes"] == str(lanes) and said["streams"] == str(len(names))
    assert said["workgroups"] == str(len(names) if lanes == 1 else 1)


def test_transform_kernels_return_the_readings_channels(built, monkeypatch, capfd):
    """Every RCT type (and the two that wrap), unsqueeze in both directions with in_place both ways and the default list,
    and the palettes, from single-leaf predictor-0 streams in ONE frame: operations of one level and kind of different
    streams share a launch, some on rectangles at non-zero ox / oy."""
    monkeypatch.setenv("JXLHIP_PACK_DEBUG", "1")
    monkeypatch.delenv("JXLHIP_MOD_LANES", raising=False)
    frame = D.Frame()
    for n in TRANSFORMS:
        case = C.build(n)
        assert case.tree == [(-1, 0, 0, 0, 1)]
        frame.add(case, placed=n in PLACED_TRANSFORMS)
    kinds = [o["kind"] for o in frame.ops]
    assert kinds.count(0) == 41 + 2 + 1 and kinds.count(1) == 4 and kinds.count(2) >= 12 and kinds.count(3) >= 12
    assert sorted(set(o["param"] for o in frame.ops if o["kind"] == 0)) == list(range(1, 42))  # (type 0 is no operation)
    assert sum(1 for o in frame.ops if o["level"] == 0 and o["kind"] == 0) >= 8  # one launch, many blocks
    assert any(any(o["ox"]) for o in frame.ops if o["kind"] == 0) and any(any(o["ox"]) for o in frame.ops if o["kind"] in (2, 3))
    said = decode(built, frame, capfd)
    assert said["form"] == "plain" and said["streams"] == str(len(TRANSFORMS))
