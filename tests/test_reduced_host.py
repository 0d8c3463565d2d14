"""The reduced decode (the image at 1/8 scale from the frame's DC image) on the CPU: the reduced parse of
libjxl_amd/csrc/host/jxh_frame.h against the whole parse and the oracle, its refusals, and the host plan of
libjxl_amd/csrc/host/jxh_reduced_plan.h under AddressSanitizer + UBSan (tests/c/reduced_kats.cc, a stand-alone program).
Nothing here touches a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import replay_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (width, height, encoder settings); "rgba": an encode_rgba8 stream (an extra channel beside the colour)
STREAMS = {
    "default": (403, 277, dict()),
    "d3_epf3": (403, 277, dict(distance=3.0, epf_iters=3)),
    "no_smoothing_cmap": (403, 277, dict(skip_dc_smoothing=1, custom_cmap=1)),
    "two_dc_groups": (2300, 300, dict(custom_lf=1, custom_cmap=1)),
    "one_section": (64, 48, dict()),
    "one_block": (8, 8, dict()),
    "rgba": (264, 200, dict()),
}


def _encode(J, name):
    w, h, kw = STREAMS[name]
    img = J.synth_image(w, h, seed=5)
    if name == "rgba":
        return J.encode_rgba8(np.dstack([img, J.synth_image(w, h, seed=6)[..., :1]]), **kw)
    return J.encode_rgb8(img, **kw)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_reduced_parse_reads_the_same_integers_from_the_dc_sections_alone(built, name):
    """Frame(data[:need], reduced=True) holds the coded DC integers and precision shifts of the whole parse; in float32 NumPy
    q_y * (step_y * 2^-e) is the oracle's Y plane bit for bit (dc_unsmoothed, or dc where nothing is smoothed); need - 1 bytes
    are "truncated frame" for every stream of more than one section; `need` lies in front of every AC section the oracle
    located (the AC global section lies between) and, for a frame coded as one section, is the frame's end: the oracle
    exports no offsets of the DC sections, so `need` is not held to an independent reading of the TOC beyond that, and that
    `need` bytes suffice (the first line). No encoder here writes a permuted TOC. The same inside a `jxlc` container cut at
    `need`."""
    import jxlo
    J = built
    data = _encode(J, name)
    need = J.frame_dc_extent(data)
    full = J.Frame(data)
    red = J.Frame(data[:need], reduced=True)
    try:
        q_full, ep_full = full.dc_quantised()
        q_red, ep_red = red.dc_quantised()
        xb, yb = full.info["xsize_blocks"], full.info["ysize_blocks"]
        assert red.reduced_size() == full.reduced_size() == (xb, yb) == ((STREAMS[name][0] + 7) // 8, (STREAMS[name][1] + 7) // 8)
        assert q_red.shape == (3, yb, xb) and np.array_equal(q_red, q_full) and np.array_equal(ep_red, ep_full)
        assert len(ep_red) == full.info["num_dc_groups"] == ((xb + 255) // 256) * ((yb + 255) // 256)
        assert red.end == full.end == len(data)
        one_section = full.info["num_groups"] == 1 and full.info["num_passes"] == 1
    finally:
        full.close()
        red.close()
    o = jxlo.Decoded(data, ac_export=not one_section and name != "rgba")
    try:
        raw = o.buffer("dc_unsmoothed")
        raw = (o.buffer("dc") if raw is None else raw).reshape(3, yb, xb)
        if name == "no_smoothing_cmap":
            assert o.buffer("dc_unsmoothed") is None, "the stream must skip the smoothing"
        # the Y step from the oracle's own reading of the quantiser headers, in float32 like the reference (the oracle reports
        # dc_step itself only where it smooths: there the two agree exactly)
        h = o.quant_header
        step_y = (np.float32(65536.0) / np.float32(h["global_scale"])) / np.float32(h["quant_dc"]) * np.float32(h["dc_quant"][1])
        if o.buffer("dc_unsmoothed") is not None:
            assert step_y == np.float32(o.dc_params["dc_step"][1])
        first_ac = None if one_section or name == "rgba" else min(s[1] for p in o.ac_tables["sections"] for s in p)
    finally:
        o.close()
    shift = np.repeat(np.repeat(ep_red.reshape((yb + 255) // 256, (xb + 255) // 256), 256, 0), 256, 1)[:yb, :xb]
    mul = np.float32(1) / np.exp2(shift & 3).astype(np.float32)
    y = q_red[1].astype(np.float32) * (step_y * mul).astype(np.float32)
    assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), raw[1].view(np.uint32))
    assert np.abs(q_red[1]).max() > 0
    if one_section:
        assert need == len(data)
    else:
        assert need < len(data)
        with pytest.raises(J.JxlAmdError, match="truncated frame$"):
            J.Frame(data[:need - 1], reduced=True)
        if first_ac is not None:
            assert need < first_ac
    # a prefix too short for the headers and the TOC: come back with more; any longer prefix says the same `need`
    with pytest.raises(J.JxlAmdError, match="truncated frame header"):
        J.frame_dc_extent(data[:8])
    assert J.frame_dc_extent(data[:need]) == need
    # inside a jxlc box cut at its own `need`: the box's declared end lies beyond the buffer
    boxed = R.container(data, pieces=1)
    need_b = J.frame_dc_extent(boxed)
    assert need_b - need == len(boxed) - len(data)  # (the boxes in front of the codestream)
    assert J.frame_dc_extent(boxed[:need_b]) == need_b
    f = J.Frame(boxed[:need_b], reduced=True)
    try:
        assert np.array_equal(f.dc_quantised()[0], q_full)
    finally:
        f.close()
    if not one_section:
        with pytest.raises(J.JxlAmdError, match="truncated frame$"):
            J.Frame(boxed[:need_b - 1], reduced=True)
    with pytest.raises(J.JxlAmdError, match="truncated frame header"):
        J.frame_dc_extent(boxed[:40])
    # the whole parse still refuses a box cut short (its rule did not move)
    if not one_section:
        with pytest.raises(J.JxlAmdError, match="bad box size"):
            J.Frame(boxed[:need_b])


def _refused_streams(J):
    rng = np.random.default_rng(3)
    img = J.synth_image(96, 64, seed=7)
    base, top = J.synth_image(128, 96, seed=31), J.synth_image(48, 32, seed=32)
    ramp = np.tile(np.linspace(0, 255, 48).astype(np.uint8), (32, 1))[..., None]
    opaque = np.full((96, 128, 1), 255, np.uint8)
    atlas = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    patches = [dict(x0=4, y0=6, xsize=20, ysize=16, positions=[(50, 30, 1, 0)])]

    def with_splines():
        J.set_splines([dict(points=[(10, 12), (40, 50), (80, 20)], color=[[40] + [0] * 31, [300, 10] + [0] * 30, [0] * 32], sigma=[12] + [0] * 31)])
        try:
            return J.encode_rgb8(img)
        finally:
            J.set_splines(None)

    def second_frame_alone(make):
        """The image header of make()'s two-frame stream followed by its second frame (frames are byte-aligned): a codestream
        whose first frame is the regular, last frame that carries the flag the two-frame encoders put on their second."""
        def spliced():
            data = make()
            header = J._enc_lib().jxlenc_last_header_bytes()  # (of the second encode: both frames were coded behind the same header)
            first = J.ModFrame(data) if J.frame_is_modular(data) else J.Frame(data)
            try:
                assert header < first.end < len(data) and not first.is_last
                return data[:header] + data[first.end:]
            finally:
                first.close()
        return spliced

    first = "the first frame is not a regular, full-canvas, last frame"
    patched = lambda: J.encode_patched(J.synth_image(128, 96, seed=4), atlas, patches, atlas_vardct=True)  # noqa: E731
    dc_framed = lambda: J.encode_with_dc_frame(J.synth_image(128, 128, seed=2), dc_vardct=True)  # noqa: E731
    return [
        ("lossless", lambda: J.encode_lossless(img), "a Modular frame has no DC image"),
        ("animation", lambda: J.encode_animation([img, img[::-1].copy()], [1, 1]), first),
        ("layers", lambda: J.encode_layers([dict(img=np.dstack([base, opaque]), save_as=1),
                                            dict(img=np.dstack([top, ramp]), x0=20, y0=30, mode=2, alpha_mode=2, source=1)]), first),
        # (as the encoders write them, these two begin with the reference frame and the DC frame ...)
        ("patched", patched, first),
        ("dc_frame_vardct", dc_framed, first),
        ("dc_frame_modular", lambda: J.encode_with_dc_frame(J.synth_image(128, 128, seed=2)), "a Modular frame has no DC image"),
        # (... and with that frame cut out, the frame that carries the flag stands first)
        ("patches_flag", second_frame_alone(patched), "the frame has patches"),
        ("use_dc_frame", second_frame_alone(dc_framed), "the frame takes its DC image from a DC frame (kUseDcFrame)"),
        ("splines", with_splines, "the frame has splines"),
        ("upsampled", lambda: J.encode_rgb8(img, upsampling=2), "the frame is upsampled"),
        ("ycbcr_420", lambda: J.encode_rgb8(img, color_transform=2, chroma_subsampling=4), "the frame is chroma-subsampled"),
        ("not_xyb", lambda: J.encode_rgb8(img, color_transform=1), "the image is not XYB-encoded"),
        ("preview", lambda: J.encode_with_preview(img, J.synth_image(32, 24, seed=8)), "the first frame is a preview"),
    ]


def test_reduced_parse_refusals_each_with_its_own_text(built):
    """One stream per rule, each refused with the rule's own text and before any DC group is decoded (a whole stream and its
    first 200 bytes are refused alike: the decision needs the headers only). The patches flag and kUseDcFrame stand on the
    second frame of the streams the encoders write; with the frame in front cut out (image header + second frame) they stand
    on a first frame that passes the first-frame rule, and their own rules answer. Nine rules, nine distinct texts, all
    raised. A reduced frame is refused by the full uploads, and a whole frame that the reduced parse would refuse is refused
    by jxlamd_frame_upload_reduced with the same reason, before the context is looked at; no device is involved."""
    import ctypes
    J = built
    L = J.lib()
    fake = ctypes.c_void_p(1)  # (never dereferenced: every call below is refused before it looks at the context)
    L.jxlamd_frame_upload_reduced.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    seen = set()
    for name, make, text in _refused_streams(J):
        data = make()
        for piece in (data, data[:200]):
            with pytest.raises(J.JxlAmdError, match="reduced decode: " + re.escape(text)):
                J.Frame(piece, reduced=True)
        seen.add(text)
        if "Modular" not in text:
            assert J.frame_dc_extent(data) > 0, name  # (the extent of a VarDCT frame is a matter of its TOC alone)
        # the whole parse of the same first frame, handed to the reduced upload: the same rule
        if name in ("patches_flag", "splines", "upsampled", "ycbcr_420", "not_xyb", "animation"):
            whole = J.Frame(data)
            try:
                assert L.jxlamd_frame_upload_reduced(whole._h, fake) == 1, name
                reason = L.jxlamd_last_error().decode()
                assert reason.startswith("reduced decode of a whole frame: "), reason
                assert {"patches_flag": "patches", "splines": "splines", "upsampled": "upsampled", "ycbcr_420": "chroma-subsampled",
                        "not_xyb": "not XYB-encoded", "animation": "not a regular, full-canvas, last frame"}[name] in reason
            finally:
                whole.close()
    assert len(seen) == 9
    red = J.Frame(_encode(J, "default"), reduced=True)
    try:
        assert L.jxlamd_frame_upload(red._h, None) != 0  # (a NULL context: refused before it is looked at)
        assert L.jxlamd_frame_upload(red._h, fake) == 1 and b"reduced decode" in L.jxlamd_last_error()
        assert L.jxlamd_frame_upload_band(red._h, fake, 0, 1) == 1 and b"jxlamd_frame_upload_reduced" in L.jxlamd_last_error()
    finally:
        red.close()


def _build_kats(tmp_path):
    out = os.path.join(str(tmp_path), "reduced_kats")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "reduced_kats.cc"), "-o", out], check=True)
    return out


def test_reduced_plan_under_sanitizers(tmp_path):
    """Every ReducedRule refuses the one change that breaks it (the rules the program exercised are the header's enum, all
    of it), extents near 2^32 included; a context's block placed into a heap block of exactly its size stays inside it; for
    sets of 1, 2 and 7 frames, a 1x1-block frame among them, the tile origins are strictly increasing, cover every tile
    exactly once and stay inside the stated bound: the program's own checks."""
    exe = _build_kats(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("exercised:")]
    assert len(line) == 1, r.stdout
    header = open(os.path.join(ROOT, "libjxl_amd", "csrc", "host", "jxh_reduced_plan.h")).read()
    rules = re.findall(r"^  kReducedRule(\w+),", header, re.M)
    assert "Count" not in rules and len(rules) == 8 and set(line[0].split()[1:]) == set(rules), sorted(set(rules) ^ set(line[0].split()[1:]))
    assert "sets: 1 2 7" in r.stdout and r.stdout.strip().endswith("ok")
    # the plan stays free of HIP
    assert "hip_runtime" not in header and "__device__" not in header
