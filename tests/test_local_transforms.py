"""CPU tests of Modular frames whose GROUP streams carry transforms of their own (palette, RCT, Squeeze in the group
header: what the reference encoder writes per group at its default effort, lib/jxl/enc_modular.cc:1424-1521). Lossless
frames: the yardstick is the stream writer's INPUT; the oracle (unchanged, it undoes any transform list generically) is
the second reading; the host plan is held to the launch schedule it promises. No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def streams(built):
    import local_streams
    return local_streams.cases(built)


def _oracle_pixels(data, channels):
    import jxlo
    got = jxlo.Decoded(data, dumps=False).rgb8
    if channels == 1:  # (the oracle shows a grey image as R = G = B)
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        return got[..., :1]
    if channels == 2:
        assert got.shape[2] == 4 and np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        return got[..., (0, 3)]
    return got


def test_oracle_returns_the_writers_input(streams):
    """Every writer mode through the unchanged oracle: the new writer is right."""
    for name, img, data, _ in streams:
        got = _oracle_pixels(data, img.shape[2])
        assert got.shape == img.shape, name
        assert np.array_equal(got, img), "%s: %d samples differ" % (name, int((got != img).sum()))


def test_host_plan_parses_and_levels_are_chain_depth_not_group_count(built, streams):
    """The host plan accepts every such stream (it used to raise "group-local palette / squeeze"), and the number of launch
    levels is the depth of the deepest group's chain: 1 for an RCT in every group at 4 groups and at 135."""
    J = built
    for name, img, data, levels in streams:
        f = J.ModFrame(data)
        info = dict(f.info)
        f.close()
        assert info["num_local_ops"] > 0 and info["num_local_ops"] <= info["num_ops"], name
        assert info["local_levels"] <= info["launch_levels"] <= info["num_ops"], name
        if levels is not None:
            assert info["launch_levels"] == levels and info["local_levels"] == levels, (name, info)
    by_name = {name: (img, data) for name, img, data, _ in streams}
    # Squeeze: 5 horizontal + 5 vertical halvings of a 256 x 256 group, preceded by the two chroma steps: 12 dependent
    # steps, although the group's list has 34 operations and the frame 6 groups
    f = J.ModFrame(by_name["squeeze"][1])
    assert f.info["local_levels"] == 12 and f.info["launch_levels"] == 12 and f.info["num_local_ops"] > 6 * 12
    f.close()
    # a global Squeeze in front: the frame's own steps are one level each as before, the local chains stay short
    f = J.ModFrame(by_name["global_squeeze_local_squeeze"][1])
    assert f.info["launch_levels"] == f.info["local_levels"] + (f.info["num_ops"] - f.info["num_local_ops"])
    assert f.info["local_levels"] <= 12
    f.close()
    img = np.random.default_rng(4).integers(0, 256, (2160, 3840, 3), dtype=np.uint8)
    f = J.ModFrame(J.encode_lossless(img, J.LOSSLESS_LOCAL_RCT))
    assert f.info["num_local_ops"] == 135 and f.info["launch_levels"] == 1
    f.close()
    # without group transforms nothing changes: the frame's own list, one level per entry
    f = J.ModFrame(J.encode_lossless(img[:300, :700], J.LOSSLESS_RCT | J.LOSSLESS_SQUEEZE))
    assert f.info["num_local_ops"] == 0 and f.info["local_levels"] == 0 and f.info["launch_levels"] == f.info["num_ops"]
    f.close()


@pytest.mark.parametrize("bits", [8, 16])
def test_implicit_palette_colours_against_an_independent_table(built, bits):
    """palette_np (NumPy, from the format's text) says which colours the indices 1...189 and -143...-1 of a one-entry
    palette mean, at 8 and at 16 bits. An image of exactly those must pass the writer's implicit-only mode (which refuses
    any other colour beyond its single explicit entry: a wrong table in the writer shows there) and come back from the
    oracle unchanged (a wrong table in a decoder changes pixels)."""
    import jxlo
    import local_streams
    import palette_np
    J = built
    idx, colors = palette_np.implicit_colors(1, bits)
    assert len(idx) == 189 + 143 and idx[0] == 1 and idx[188] == 189 and idx[189] == -1 and idx[-1] == -143
    top = (1 << bits) - 1
    assert colors[:189].min() >= 0 and colors[:189].max() <= top  # the cubes lie in range; [188] is the 5-cube's last corner
    assert colors[188].tolist() == [top, top, top] and colors[0].tolist() == [1 << (bits - 3)] * 3
    img, usable = local_streams.implicit_image(bits)
    assert usable > 189  # some negative-index entries are positive offsets an unsigned image can hold
    data = J.encode_lossless_samples(img, bits, flags=J.LOSSLESS_LOCAL_IMPLICIT)
    o = jxlo.Decoded(data, dumps=True)
    assert o.info["bits"] == bits
    assert np.array_equal(o.buffer("modular").reshape(3, img.shape[0], img.shape[1]), np.moveaxis(img, -1, 0))
    o.close()
    f = J.ModFrame(data)
    assert f.info["launch_levels"] == 1 and f.info["num_local_ops"] == 4
    f.close()
    other = img.copy()
    other[0, 0] = np.array([9, 9, 200]) * (1 << (bits - 8))  # a second colour that is not implicit
    with pytest.raises(J.JxlAmdError):
        J.encode_lossless_samples(other, bits, flags=J.LOSSLESS_LOCAL_IMPLICIT)


def _bits(data, pos, n):
    return sum(((data[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i for i in range(n))


def _set_bits(data, pos, n, value):
    for i in range(n):
        byte, bit = (pos + i) >> 3, (pos + i) & 7
        data[byte] = (data[byte] & ~(1 << bit)) | (((value >> i) & 1) << bit)


@pytest.mark.parametrize("what", ["nb_deltas", "predictor"])
def test_group_palette_with_deltas_or_predictor_is_refused(built, streams, what):
    """Still outside the GPU path (a serial chain per channel): a group header whose palette has delta entries or a predictor
    ends in JxlAmdError with the message the global form has, not in a plan. The header is patched by hand: group 0 of
    'palette_some_groups' starts use_global_tree 1, default WP 1, one transform (2 bits), id 1 (2), begin_c 0 (2 + 3),
    num_c 3 (2), nb_colors (2 + 8), nb_deltas 0 (2), predictor 0 (4)."""
    J = built
    data = bytearray(next(d for name, _, d, _ in streams if name == "palette_some_groups"))
    f = J.ModFrame(bytes(data))
    off, size = f.section(2 + 1 + 0)  # one DC group: sections are DC global, DC group 0, AC groups
    f.close()
    at = off * 8
    assert size > 8 and _bits(data, at, 15) == 0b000100000010111 and _bits(data, at + 15, 8) == 12 and _bits(data, at + 23, 6) == 0
    if what == "predictor":
        _set_bits(data, at + 25, 4, 5)
    else:  # selector 1 = 1 + 8 bits; the predictor then follows those
        _set_bits(data, at + 23, 2, 1)
        _set_bits(data, at + 25, 8, 0)
        _set_bits(data, at + 33, 4, 0)
    with pytest.raises(J.JxlAmdError, match="palette with delta entries / predictor"):
        J.ModFrame(bytes(data))


def test_host_plan_under_sanitizers_on_damaged_local_transform_streams(built, streams, tmp_path):
    """tests/c/host_fuzz.cc (AddressSanitizer + UBSan around the host parsers) over the new streams, each damaged 60 times
    (seeded): every run ends in jxh::Error or success, with no sanitizer report. The 2300 x 2100 stream stays out (16 MB per
    copy); the DC-group transforms it has are parsed clean in the tests above."""
    import local_streams
    J = built
    out = os.path.join(str(tmp_path), "host_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", os.path.join(ROOT, "tests", "c", "host_fuzz.cc"), "-o", out], check=True)
    files = []
    small = [(n, d) for n, _, d, _ in streams if not n.startswith("two_dc_groups")]
    img, _ = local_streams.implicit_image(8)
    small.append(("implicit", J.encode_lossless_samples(img, 8, flags=J.LOSSLESS_LOCAL_IMPLICIT)))
    for name, d in small:
        files.append(os.path.join(str(tmp_path), name + ".jxl"))
        open(files[-1], "wb").write(d)
    r = subprocess.run([out, "60"] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "refused" in r.stdout
