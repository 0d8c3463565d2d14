"""GPU tests (-m gpu) of Modular frames whose group streams carry a palette, an RCT or a Squeeze of their own. Lossless
frames: the HIP path must return the stream writer's INPUT exactly (tests/test_local_transforms.py holds the writer against
the oracle on the CPU). No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def streams(built):
    import local_streams
    return local_streams.cases(built)


def _decode(J, data, channels, data_type=2):
    """decode_lossless, with every stream's status word checked to be zero."""
    f = J.ModFrame(data)
    c = J.HipContext()
    try:
        c.set_output_format(data_type, channels)
        c.upload_modular(f)
        c.run_modular()
        r, status, _ = c.modular_status()
        assert r == 0 and not any(status), [(i, s) for i, s in enumerate(status) if s]
        return c.pixels()
    finally:
        c.close()
        f.close()


def test_every_local_transform_stream_returns_the_input(built, streams):
    J = built
    for name, img, data, _ in streams:
        out = _decode(J, data, img.shape[2])
        assert out.shape == img.shape, name
        assert np.array_equal(out, img), "%s: %d samples differ" % (name, int((out != img).sum()))
    by_name = {name: (img, data) for name, img, data, _ in streams}
    img, data = by_name["palettes_then_rct"]  # the writer formats: exact multiples of the 8-bit samples
    assert np.array_equal(_decode(J, data, 3, data_type=3), img.astype(np.uint16) * 257)
    img, data = by_name["rgba_everything"]
    got = _decode(J, data, 4, data_type=0)
    assert got.dtype == np.float32 and np.array_equal(got, img.astype(np.float32) * np.float32(1.0 / 255))


@pytest.mark.parametrize("bits", [8, 16])
def test_implicit_palette_colours_on_gpu(built, bits):
    """An image of nothing but implicit palette colours (indices 1...189 and the negative ones an unsigned image can hold,
    by tests/palette_np.py) coded with ONE explicit entry per group: the kernel's tables against the independent one."""
    import local_streams
    J = built
    img, _ = local_streams.implicit_image(bits)
    data = J.encode_lossless_samples(img, bits, flags=J.LOSSLESS_LOCAL_IMPLICIT)
    if bits == 8:
        assert np.array_equal(_decode(J, data, 3), img.astype(np.uint8))
    else:
        assert np.array_equal(_decode(J, data, 3, data_type=3), img.astype(np.uint16))


def test_batch_of_frames_with_different_chain_depths(built, streams):
    """No group transforms / an RCT per group / palettes + RCT / Squeeze, as ONE set: the launch levels mix across frames."""
    J = built
    by_name = {name: (img, data) for name, img, data, _ in streams}
    plain = J.synth_image(700, 300, seed=8)
    members = [(plain, J.encode_lossless(plain, J.LOSSLESS_RCT | J.LOSSLESS_SQUEEZE)), by_name["rct_types_by_seed_ragged"],
               by_name["palettes_then_rct"], by_name["squeeze"]]
    frames = [J.ModFrame(d) for _, d in members]
    assert len({f.info["local_levels"] for f in frames}) == 4
    ctxs = [J.HipContext() for _ in members]
    try:
        for c, f in zip(ctxs, frames):
            c.upload_modular(f)
        J.run_modular_batch(ctxs)
        for c, (img, _) in zip(ctxs, members):
            r, status, _ = c.modular_status()
            assert r == 0 and not any(status)
            assert np.array_equal(c.pixels(), img)
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()


def test_4k_local_palettes_and_rct(built):
    """3840 x 2160: flat groups (at most 64 colours) get an all-channel palette, the others an RCT; alone and three frames
    as one set."""
    J = built
    rng = np.random.default_rng(12)
    img = J.synth_image(3840, 2160, seed=41)
    table = rng.integers(0, 256, (48, 3), dtype=np.uint8)
    for gy in range(9):
        for gx in range(15):
            if (gx + 2 * gy) % 3 == 0:  # a flat group: a chart, a margin
                a = img[gy * 256:(gy + 1) * 256, gx * 256:(gx + 1) * 256]
                a[...] = table[rng.integers(0, 48, a.shape[:2]) % (4 + 4 * ((gx + gy) % 12))]
    data = J.encode_lossless(img, J.LOSSLESS_LOCAL_PALETTE | J.LOSSLESS_LOCAL_RCT, palette_colors=64)
    f = J.ModFrame(data)
    assert f.info["launch_levels"] <= 2 and f.info["num_local_ops"] >= 135
    f.close()
    assert np.array_equal(_decode(J, data, 3), img)
    frames = [J.ModFrame(data) for _ in range(3)]
    ctxs = [J.HipContext() for _ in range(3)]
    try:
        for c, f in zip(ctxs, frames):
            c.upload_modular(f)
        J.run_modular_batch(ctxs)
        for c in ctxs:
            r, status, _ = c.modular_status()
            assert r == 0 and not any(status)
            assert np.array_equal(c.pixels(), img)
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()


def test_local_transforms_through_the_decoder_api(built, streams, tmp_path):
    """The JxlDecoder boundary (plain-C replay program), container and chunked input."""
    import replay_util as R
    img, data = next((i, d) for n, i, d, _ in streams if n == "palettes_then_rct")
    rc, events, out, px = R.run(R.container(data), tmp_path, "u8", 3, "chunk=5000")
    assert rc == 0 and events[-2:] == ["FULL_IMAGE", "SUCCESS"], out
    assert np.array_equal(np.frombuffer(px, np.uint8).reshape(img.shape), img)


def test_guard_bands_stay_clean_and_results_do_not_depend_on_their_fill(built, streams, monkeypatch):
    """JXLHIP_GUARD=1: every device buffer between guard bands, fresh allocations filled with JXLHIP_GUARD_BYTE. A palette, a
    Squeeze and a ragged-size case: guards intact, the same (right) output under both fills -- no operation reads a
    private buffer before its stream wrote it, none leaves its rectangle."""
    J = built
    monkeypatch.setenv("JXLHIP_GUARD", "1")
    picked = [(n, i, d) for n, i, d, _ in streams if n in ("palettes_then_rct", "global_squeeze_local_squeeze", "rct_types_by_seed_ragged",
                                                          "rgba_everything")]
    assert len(picked) == 4
    for byte in ("0xA5", "0xFF"):
        monkeypatch.setenv("JXLHIP_GUARD_BYTE", byte)
        for name, img, data in picked:
            f = J.ModFrame(data)
            c = J.HipContext()
            try:
                c.set_output_format(2, img.shape[2])
                c.upload_modular(f)
                c.run_modular()
                c.sync()
                assert c.check_guards() == 0, (name, byte, c.check_guards())
                assert np.array_equal(c.pixels(), img), (name, byte)
            finally:
                c.close()
                f.close()


def test_damaged_group_sections_are_contained(built, streams):
    """Bytes flipped behind the headers, inside the group sections: wrong indices, wrong residuals. They end as status words
    (or as JxlAmdError where the damage reaches a header), never outside a buffer: palette indices are bounded by the
    lookup's own case split, the operations' rectangles were validated at upload. The context decodes a good frame after."""
    J = built
    good_img, good = next((i, d) for n, i, d, _ in streams if n == "palettes_then_rct")
    rng = np.random.default_rng(5)
    on_device = flagged = 0
    for name in ("palettes_then_rct", "squeeze", "rgba_everything"):
        img, clean = next((i, d) for n, i, d, _ in streams if n == name)
        data = bytearray(clean)
        for pos in rng.integers(len(data) // 2, len(data) - 8, 40):
            data[int(pos)] ^= 0x5A
        try:
            f = J.ModFrame(bytes(data))
        except J.JxlAmdError:
            continue
        c = J.HipContext()
        try:
            c.set_output_format(2, img.shape[2])
            c.upload_modular(f)
            c.run_modular()
            on_device += 1
            r, status, _ = c.modular_status()
            if r != 0 and any(status):
                flagged += 1
            else:  # (flips that a stream never reads, padding for one, change nothing: then nothing may have changed)
                assert np.array_equal(c.pixels(), img), "%s: damage changed samples without a status word" % name
            c.set_output_format(2, 3)
            g = J.ModFrame(good)
            c.upload_modular(g)
            c.run_modular()
            r, status, _ = c.modular_status()
            assert r == 0 and not any(status)
            assert np.array_equal(c.pixels(), good_img)
            g.close()
        finally:
            c.close()
            f.close()
    # the test is about the device: it must not turn into a parser test unnoticed when a stream changes
    assert on_device >= 1 and flagged >= 1, (on_device, flagged)
