"""CPU tests of the product's host side: the C-ABI library loads and exports every declared symbol, the host
front-end (csrc/host) agrees with the oracle on everything it parses, the API fails loudly without a GPU, and the
multi-rank sharding/aggregation logic works under gloo with world_size 2.  No compute calls need a GPU here."""
import ctypes
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions(header):
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(jxlhip_\w+|jxlamd_\w+|Jxl[A-Z]\w+)\s*\(", src))
    # typedef'd callback types are not exported functions
    typedefs = set(re.findall(r"\(\*\s*(\w+)\s*\)", src))
    return sorted(n for n in names - typedefs if not n.endswith("Callback"))


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    headers = ["jxl_amd_hip.h", "jxl_amd.h", "jxl/decode.h", "jxl/thread_parallel_runner.h", "jxl/resizable_parallel_runner.h"]
    missing = []
    total = 0
    for h in headers:
        for name in _declared_functions(os.path.join(ROOT, "include", h)):
            total += 1
            if not hasattr(lib, name):
                missing.append((h, name))
    assert total > 60
    assert not missing, missing


def test_streams_with_an_embedded_icc_profile_parse(built):
    """want_icc streams: the host front-end decodes the profile (the reference's own vector: tests/test_kats.py pins the
    decoder), finds the frame behind it, and the oracle, which only skips the profile, decodes the same pixels."""
    import jxlo
    J = built
    g = os.path.join(ROOT, "tests", "golden")
    coded = open(os.path.join(g, "ref_icc_test_profile.enc"), "rb").read()
    want = open(os.path.join(g, "ref_icc_test_profile.icc"), "rb").read()
    icc, bits = J.icc_decode(coded)
    assert icc == want and len(coded) * 8 - 8 < bits <= len(coded) * 8
    with pytest.raises(J.JxlAmdError):
        J.icc_decode(coded[:100])
    img = J.synth_image(200, 120, seed=8)
    plain = J.encode_rgb8(img)
    J.set_embedded_icc(coded)
    try:
        data, lossless = J.encode_rgb8(img), J.encode_lossless(img, J.LOSSLESS_RCT)
    finally:
        J.set_embedded_icc(None)
    assert len(data) > len(plain) + 380
    f = J.Frame(data)
    assert f.info["xsize"] == 200 and f.info["ysize"] == 120
    f.close()
    a, b = jxlo.Decoded(plain, dumps=False), jxlo.Decoded(data, dumps=False)
    assert np.array_equal(a.rgb8, b.rgb8)
    c = jxlo.Decoded(lossless, dumps=False)
    assert np.array_equal(c.rgb8, img)
    m = J.ModFrame(lossless)
    assert m.info["xsize"] == 200
    m.close()
    for o in (a, b, c):
        o.close()


def test_frame_plan_matches_oracle(built):
    import jxlo
    J = built
    for kw in [dict(), dict(strategy_mode=0, distance=2.0), dict(strategy_mode=2, random_cmap=1),
               dict(color_transform=2, chroma_subsampling=4, strategy_mode=0, custom_bctx=1),   # 4:2:0: whole MCUs, subsampled DC streams
               dict(color_transform=2, chroma_subsampling=0b011011, strategy_mode=0)]:
        data = J.encode_rgb8(J.synth_image(600, 410, seed=9), **kw)
        f = J.Frame(data, threads=2)
        o = jxlo.Decoded(data, dumps=False)
        for a, b in [("xsize", "xsize"), ("ysize", "ysize"), ("num_groups", "num_groups"), ("num_dc_groups", "num_dc_groups"),
                     ("used_acs", "used_acs"), ("epf_iters", "epf_iters"), ("gab", "gab"), ("num_passes", "num_passes")]:
            assert f.info[a] == o.info[b], (a, f.info[a], o.info[b])
        assert f.info["coef_bits"] == 16
        assert 0 < f.info["ac_bytes"] < len(data)
        f.close()


def test_host_rejects_bad_input(built):
    J = built
    with pytest.raises(J.JxlAmdError):
        J.Frame(b"\x00\x01\x02")
    data = J.encode_rgb8(J.synth_image(300, 200))
    with pytest.raises(J.JxlAmdError, match="truncated"):
        J.Frame(data[: len(data) // 2])
    # a Modular (lossless) stream is valid JPEG XL but outside the GPU hot path: must be refused, not mis-decoded
    golden = os.path.join(ROOT, "tests", "golden", "fjxl_37x29_rgba_e2.jxl")
    with pytest.raises(J.JxlAmdError, match="unsupported"):
        J.Frame(open(golden, "rb").read())
    # container boxes whose 64-bit size would wrap an offset computation: refused, nothing read past the buffer
    sig = b"\0\0\0\x0cJXL \r\n\x87\n"
    for size64 in (0xFFFFFFFFFFFFFFF0, 0xFFFFFFFFFFFFFFFF, 1 << 63, len(data) + 1000):
        evil = sig + b"\0\0\0\x01jxlc" + size64.to_bytes(8, "big") + data
        with pytest.raises(J.JxlAmdError, match="box"):
            J.Frame(evil)


def test_no_gpu_means_loud_failure(built):
    J = built
    if J.lib().jxlhip_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(J.JxlAmdError, match="no HIP device"):
        J.HipContext()
    with pytest.raises(J.JxlAmdError):
        J.decode_rgb8(J.encode_rgb8(J.synth_image(64, 64)))


def test_jxl_decoder_api_events_without_pixels(built):
    """The JxlDecoder state machine (basic info / colour / frame header events) runs on the host alone."""
    J = built
    L = J.lib()
    L.JxlDecoderCreate.restype = ctypes.c_void_p
    L.JxlDecoderCreate.argtypes = [ctypes.c_void_p]
    for n in ("JxlDecoderDestroy", "JxlDecoderProcessInput", "JxlDecoderCloseInput"):
        getattr(L, n).argtypes = [ctypes.c_void_p]
    L.JxlDecoderSubscribeEvents.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.JxlDecoderSetInput.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.JxlDecoderGetBasicInfo.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.JxlSignatureCheck.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    data = J.encode_rgb8(J.synth_image(321, 123))
    assert L.JxlSignatureCheck(data, len(data)) == 2  # JXL_SIG_CODESTREAM
    assert L.JxlSignatureCheck(b"\x89PNG", 4) == 1
    dec = L.JxlDecoderCreate(None)
    assert dec
    assert L.JxlDecoderSubscribeEvents(dec, 0x40 | 0x100 | 0x400) == 0
    assert L.JxlDecoderSetInput(dec, data, len(data)) == 0
    L.JxlDecoderCloseInput(dec)
    assert L.JxlDecoderProcessInput(dec) == 0x40  # JXL_DEC_BASIC_INFO
    info = (ctypes.c_uint32 * 64)()
    assert L.JxlDecoderGetBasicInfo(dec, info) == 0
    assert (info[1], info[2], info[3]) == (321, 123, 8)  # xsize, ysize, bits_per_sample
    assert L.JxlDecoderProcessInput(dec) == 0x100  # JXL_DEC_COLOR_ENCODING
    assert L.JxlDecoderProcessInput(dec) == 0x400  # JXL_DEC_FRAME
    assert L.JxlDecoderProcessInput(dec) == 0  # JXL_DEC_SUCCESS (no image requested)
    L.JxlDecoderDestroy(dec)
    # events must be subscribed before decoding starts; garbage is an error, not a crash
    dec = L.JxlDecoderCreate(None)
    L.JxlDecoderSubscribeEvents(dec, 0x40)
    L.JxlDecoderSetInput(dec, b"garbage!", 8)
    assert L.JxlDecoderProcessInput(dec) == 1  # JXL_DEC_ERROR
    assert L.JxlDecoderProcessInput(dec) == 1  # sticky
    L.JxlDecoderDestroy(dec)


def test_reference_dc_not_gettable_sequence(built):
    """DecodeTest.DCNotGettableTest (lib/jxl/decode_test.cc:2509-2536) on the reference's own 68-byte stream: subscribed to
    BASIC_INFO only, JxlDecoderProcessInput returns JXL_DEC_BASIC_INFO and then JXL_DEC_SUCCESS."""
    J = built
    L = J.lib()
    L.JxlDecoderCreate.restype = ctypes.c_void_p
    L.JxlDecoderCreate.argtypes = [ctypes.c_void_p]
    for n in ("JxlDecoderDestroy", "JxlDecoderProcessInput"):
        getattr(L, n).argtypes = [ctypes.c_void_p]
    L.JxlDecoderSubscribeEvents.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.JxlDecoderSetInput.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.JxlDecoderGetBasicInfo.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    data = open(os.path.join(ROOT, "tests", "golden", "ref_decode_test_1x1.jxl"), "rb").read()
    dec = L.JxlDecoderCreate(None)
    assert L.JxlDecoderSubscribeEvents(dec, 0x40) == 0
    assert L.JxlDecoderSetInput(dec, data, len(data)) == 0
    assert L.JxlDecoderProcessInput(dec) == 0x40  # JXL_DEC_BASIC_INFO
    info = (ctypes.c_uint32 * 64)()
    assert L.JxlDecoderGetBasicInfo(dec, info) == 0
    assert (info[1], info[2], info[3]) == (1, 1, 8)
    assert L.JxlDecoderProcessInput(dec) == 0    # JXL_DEC_SUCCESS
    L.JxlDecoderDestroy(dec)


def test_reference_jni_wrapper_streams(built):
    """The two streams the reference's Java wrapper test holds (tools/jni/org/jpeg/jpegxl/wrapper/DecoderTest.java:12-20: a
    36-byte 1024x1024 Modular image and a 19-byte 1x1 image with alpha) and what it asserts of them without pixels
    (:69-100): decodeInfo reports the dimension and the alpha bits (0 / 8), and the first 0..5 bytes of the first stream
    are 'not enough input'. (Its ICC-size assertion needs the CMS's profile synthesis, out of scope: SURVEY.md 2.) The
    oracle decodes both; the GPU side is tests/test_gpu_modular.py."""
    import jxlo
    J = built
    L = J.lib()
    L.JxlDecoderCreate.restype = ctypes.c_void_p
    L.JxlDecoderCreate.argtypes = [ctypes.c_void_p]
    for n in ("JxlDecoderDestroy", "JxlDecoderProcessInput"):
        getattr(L, n).argtypes = [ctypes.c_void_p]
    L.JxlDecoderSubscribeEvents.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.JxlDecoderSetInput.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.JxlDecoderGetBasicInfo.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    simple = open(os.path.join(ROOT, "tests", "golden", "ref_jni_simple_1024.jxl"), "rb").read()
    pixel = open(os.path.join(ROOT, "tests", "golden", "ref_jni_pixel_alpha_1x1.jxl"), "rb").read()
    assert (len(simple), len(pixel)) == (36, 19)
    for data, dim, alpha_bits in ((simple, 1024, 0), (pixel, 1, 8)):
        dec = L.JxlDecoderCreate(None)
        assert L.JxlDecoderSubscribeEvents(dec, 0x40) == 0
        assert L.JxlDecoderSetInput(dec, data, len(data)) == 0
        assert L.JxlDecoderProcessInput(dec) == 0x40  # JXL_DEC_BASIC_INFO
        info = (ctypes.c_uint32 * 64)()
        assert L.JxlDecoderGetBasicInfo(dec, info) == 0
        assert (info[1], info[2]) == (dim, dim)
        assert info[15] == alpha_bits  # JxlBasicInfo::alpha_bits (include/jxl/codestream_header.h)
        L.JxlDecoderDestroy(dec)
        o = jxlo.Decoded(data, dumps=False)
        assert o.rgb8.shape == (dim, dim, 4 if alpha_bits else 3)
        o.close()
    for n in range(6):
        dec = L.JxlDecoderCreate(None)
        assert L.JxlDecoderSubscribeEvents(dec, 0x40) == 0
        if n:
            assert L.JxlDecoderSetInput(dec, simple[:n], n) == 0
        assert L.JxlDecoderProcessInput(dec) == 2, n  # JXL_DEC_NEED_MORE_INPUT
        L.JxlDecoderDestroy(dec)


def test_thread_parallel_runner(built):
    L = built.lib()
    L.JxlThreadParallelRunnerCreate.restype = ctypes.c_void_p
    INIT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t)
    FUNC = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t)
    L.JxlThreadParallelRunner.argtypes = [ctypes.c_void_p, ctypes.c_void_p, INIT, FUNC, ctypes.c_uint32, ctypes.c_uint32]
    hits = np.zeros(1000, np.int32)
    seen_threads = set()
    nthreads = []

    def init(_, n):
        nthreads.append(n)
        return 0

    def func(_, i, tid):
        hits[i] += 1
        seen_threads.add(tid)

    pool = L.JxlThreadParallelRunnerCreate(None, 4)
    assert L.JxlThreadParallelRunner(pool, None, INIT(init), FUNC(func), 10, 1000) == 0
    L.JxlThreadParallelRunnerDestroy(pool)
    assert nthreads == [4]
    assert (hits[10:] == 1).all() and (hits[:10] == 0).all()
    assert max(seen_threads) < 4


_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
from libjxl_amd import sharding
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
rank = dist.get_rank()
units = sharding.shard_units(10, rank, 2)
# pretend each rank took (rank + 1) seconds to decode its share
total, t = sharding.aggregate(len(units), float(rank + 1), dist)
if rank == 0:
    print("RESULT", units, total, t)
dist.destroy_process_group()
"""


def test_sharding_two_ranks_gloo(built, tmp_path):
    pytest.importorskip("torch")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "w.py"
    script.write_text(_WORKER % {"root": ROOT, "port": port})
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs)
    line = [l for l in outs[0].splitlines() if l.startswith("RESULT")][0]
    assert line == "RESULT [0, 2, 4, 6, 8] 10.0 2.0"


def test_bench_gpus_flag_starts_that_many_ranks():
    """`python bench.py --gpus N` with no launcher around it must start N ranks itself (child torch.distributed.run,
    before any GPU call) and report n_gpus = N; started by a launcher with a different world size it must refuse."""
    pytest.importorskip("torch")
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out == {"launch_check": True, "n_gpus": 2, "ranks": [0, 1], "distinct_processes": 2}
    env["WORLD_SIZE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "refusing" in (r.stdout + r.stderr)


def test_band_partition_of_group_rows():
    """sharding.band_of: contiguous, disjoint, complete; sizes within one row; 16K = 64 rows -> 8 bands of 8."""
    from libjxl_amd import sharding
    assert [sharding.band_of(64, r, 8) for r in range(8)] == [(8 * r, 8 * r + 8) for r in range(8)]
    for rows in (1, 5, 9, 64, 67):
        for world in (1, 2, 3, 8):
            bands = [sharding.band_of(rows, r, world) for r in range(world)]
            assert bands[0][0] == 0 and bands[-1][1] == rows
            assert all(bands[i][1] == bands[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in bands]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        sharding.band_of(4, 2, 2)


def test_c_program_replays_reference_call_sequence(built, tmp_path):
    """tests/c/replay_decode.c makes the calls of lib/extras/dec/jxl.cc:140-669 (incl. SetCms, box buffers, JPEG buffer
    calls, the caller's memory manager) from plain C: it must LINK against the .so and see the reference's event order.
    Without a GPU the decode stops at the pixels (exit code 3: by design there is no CPU pixel path)."""
    import replay_util as R
    J = built
    have_gpu = J.lib().jxlhip_device_count() > 0
    data = J.encode_rgb8(J.synth_image(300, 200))
    want_rc = 0 if have_gpu else 3
    head = ["BASIC_INFO", "COLOR_ENCODING", "FRAME", "NEED_IMAGE_OUT_BUFFER"]
    tail = ["FULL_IMAGE", "SUCCESS"] if have_gpu else ["ERROR"]
    rc, events, out, _ = R.run(data, tmp_path, "f32", 3)
    assert rc == want_rc, out
    assert events == head + tail, out
    assert "memory manager: allocs=" in out and "allocs=0" not in out
    # container with the codestream split over two jxlp boxes, fed in 777-byte pieces: box events for every box in file
    # order, NEED_MORE_INPUT until the frame is complete, then the same events
    rc, events, out, _ = R.run(R.container(data), tmp_path, "u8", 4, "chunk=777")
    assert rc == want_rc, out
    boxes = [l.split(" ", 2)[2] for l in out.splitlines() if l.startswith("event BOX")]
    assert boxes == ["JXL ", "ftyp", "Exif", "jxlp", "xml ", "jxlp"], out
    core = [e for e in events if e not in ("BOX", "NEED_MORE_INPUT")]
    assert core == head + tail, out
    assert events.count("NEED_MORE_INPUT") > 10
    assert events.index("BASIC_INFO") < events.index("NEED_MORE_INPUT") < events.index("FRAME")
    # truncated file: NEED_MORE_INPUT at the end, like decode.cc:1505-1517
    rc, events, out, _ = R.run(data[: len(data) // 2], tmp_path, "u8", 3, "chunk=4096")
    assert rc == 1 and events[-1] in ("NEED_MORE_INPUT", "ERROR"), out
    # the reference's own VarDCT + alpha stream: one extra channel of type alpha reported
    ref = open(os.path.join(ROOT, "tests", "golden", "ref_decode_test_1x1.jxl"), "rb").read()
    rc, events, out, _ = R.run(ref, tmp_path, "u8", 4)
    assert rc == want_rc, out
    assert "BASIC_INFO 1x1 bits=8 extra=1 alpha_bits=8" in out and "extra channel 0 type=0 bits=8" in out
    assert events[:4] == head


def test_decoder_output_color_profile_reaches_the_frame(built):
    """JxlDecoderSetOutputColorProfile(linear) must change what the decode produces AND what GetColorAsEncodedProfile
    reports for the data target (decode.cc:2810); other profiles are refused."""
    J = built
    L = J.lib()
    vp = ctypes.c_void_p
    L.JxlDecoderCreate.restype = vp
    L.JxlDecoderCreate.argtypes = [vp]
    for n in ("JxlDecoderDestroy", "JxlDecoderProcessInput", "JxlDecoderCloseInput"):
        getattr(L, n).argtypes = [vp]
    L.JxlDecoderSubscribeEvents.argtypes = [vp, ctypes.c_int]
    L.JxlDecoderSetInput.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]

    class CE(ctypes.Structure):
        _fields_ = [("color_space", ctypes.c_int), ("white_point", ctypes.c_int), ("white_point_xy", ctypes.c_double * 2),
                    ("primaries", ctypes.c_int), ("red", ctypes.c_double * 2), ("green", ctypes.c_double * 2),
                    ("blue", ctypes.c_double * 2), ("transfer_function", ctypes.c_int), ("gamma", ctypes.c_double),
                    ("rendering_intent", ctypes.c_int)]

    L.JxlDecoderGetColorAsEncodedProfile.argtypes = [vp, ctypes.c_int, ctypes.POINTER(CE)]
    L.JxlDecoderSetOutputColorProfile.argtypes = [vp, ctypes.POINTER(CE), vp, ctypes.c_size_t]
    data = J.encode_rgb8(J.synth_image(64, 64))
    dec = L.JxlDecoderCreate(None)
    assert L.JxlDecoderSubscribeEvents(dec, 0x100 | 0x400) == 0
    L.JxlDecoderSetInput(dec, data, len(data))
    L.JxlDecoderCloseInput(dec)
    assert L.JxlDecoderProcessInput(dec) == 0x100
    ce = CE()
    assert L.JxlDecoderGetColorAsEncodedProfile(dec, 1, ctypes.byref(ce)) == 0 and ce.transfer_function == 13
    ce.transfer_function = 16  # PQ: not available on this path
    assert L.JxlDecoderSetOutputColorProfile(dec, ctypes.byref(ce), None, 0) == 1
    ce.transfer_function = 8  # linear
    assert L.JxlDecoderSetOutputColorProfile(dec, ctypes.byref(ce), None, 0) == 0
    out = CE()
    assert L.JxlDecoderGetColorAsEncodedProfile(dec, 1, ctypes.byref(out)) == 0 and out.transfer_function == 8
    assert L.JxlDecoderGetColorAsEncodedProfile(dec, 0, ctypes.byref(out)) == 0 and out.transfer_function == 13  # original
    assert L.JxlDecoderProcessInput(dec) == 0x400
    L.JxlDecoderDestroy(dec)


def test_reference_wasm_demo_streams(built, tmp_path):
    """The two codestreams of the reference's tools/wasm_demo/jxl_decoder_test.js:25-40 (made by libjxl's jxl_from_tree).
    splinesJxl: the reference asserts 320x320 (:63-64); a Modular frame whose content is one spline: the front-end plans it
    with its draw cache (pixels: tests/test_splines.py). crossJxl: a 20x20 Modular frame (:117-131: 'px = 20 * 20')
    with a palette and an MA tree: the product's Modular front-end plans it."""
    import replay_util as R
    J = built
    splines = open(os.path.join(ROOT, "tests", "golden", "ref_wasm_splines.jxl"), "rb").read()
    rc, events, out, _ = R.run(splines, tmp_path, "u8", 3)
    assert "BASIC_INFO 320x320" in out and events[:4] == ["BASIC_INFO", "COLOR_ENCODING", "FRAME", "NEED_IMAGE_OUT_BUFFER"], out
    f = J.ModFrame(splines)
    assert (f.info["xsize"], f.info["ysize"], f.info["num_color"]) == (320, 320, 3)
    f.close()
    cross = open(os.path.join(ROOT, "tests", "golden", "ref_wasm_cross.jxl"), "rb").read()
    f = J.ModFrame(cross)
    assert (f.info["xsize"], f.info["ysize"], f.info["num_color"], f.info["bits"]) == (20, 20, 3, 8)
    assert f.info["num_streams"] == 1 and f.info["num_ops"] >= 1
    f.close()
    rc, events, out, _ = R.run(cross, tmp_path, "u16", 3)
    assert "BASIC_INFO 20x20" in out and events[:4] == ["BASIC_INFO", "COLOR_ENCODING", "FRAME", "NEED_IMAGE_OUT_BUFFER"], out


def _c_array(path, name):
    """The integer initialiser list of the C array (or one-array aggregate) `name` in `path`."""
    import re
    text = open(os.path.join(ROOT, path)).read()
    m = re.search(r"\b%s(?:\[[^\]]*\])?\s*=\s*\{(.*?)\};" % re.escape(name), text, re.S)
    assert m, (path, name)
    return [int(t, 0) for t in re.findall(r"0x[0-9a-fA-F]+|\d+", re.sub(r"//.*", "", m.group(1)))]


def test_icc_stream_delivered_in_small_pieces(built, tmp_path):
    """An image whose headers are followed by a 389-byte coded ICC profile, fed 100 bytes at a time inside a container:
    the decoder asks for more input until the profile is complete (it cannot know where the profile ends before
    decoding it), then reports BASIC_INFO / COLOR_ENCODING with the profile available as the ORIGINAL one."""
    import replay_util as R
    J = built
    g = os.path.join(ROOT, "tests", "golden")
    coded = open(os.path.join(g, "ref_icc_test_profile.enc"), "rb").read()
    want = open(os.path.join(g, "ref_icc_test_profile.icc"), "rb").read()
    J.set_embedded_icc(coded)
    try:
        data = J.encode_rgb8(J.synth_image(200, 120, seed=8))
    finally:
        J.set_embedded_icc(None)
    rc, events, out, _ = R.run(R.container(data), tmp_path, "u8", 3, "chunk=100")
    assert rc == (0 if J.lib().jxlhip_device_count() > 0 else 3), out
    assert "original icc size=%d" % len(want) in out, out
    core = [e for e in events if e not in ("BOX", "NEED_MORE_INPUT")]
    assert core[:4] == ["BASIC_INFO", "COLOR_ENCODING", "FRAME", "NEED_IMAGE_OUT_BUFFER"], out
    first_info = events.index("BASIC_INFO")
    assert events[:first_info].count("NEED_MORE_INPUT") >= 3  # the ~400 bytes of profile arrive in 100-byte pieces


def test_context_model_tables_match_the_reference_source():
    """The AC context model's constant tables as the reference's source has them (tests/golden/ref_constant_tables.json,
    extracted by tests/golden/make_tables_golden.py from lib/jxl/ac_context.h:29-42,91-96 and coeff_order.h:44-46) against
    every copy in this repository: the product's host tables, the HIP layer's one statement of the per-strategy tables
    (csrc/hip/jxl_hip_block_ctx.h: host and device code read the same objects) with the packed word and the log2 built
    from them, the arithmetic forms the kernels use, the oracle's and the test encoder's. A shared transcription
    error would pass every encoder -> decoder test."""
    hip = "libjxl_amd/csrc/hip/jxl_hip_block_ctx.h"
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_constant_tables.json")))
    freq, nnz = ref["kCoeffFreqContext"], ref["kCoeffNumNonzeroContext"]
    assert _c_array("libjxl_amd/csrc/host/jxh_vardct.h", "kCoeffFreqContext") == freq
    assert _c_array("libjxl_amd/csrc/host/jxh_vardct.h", "kCoeffNumNonzeroContext") == nnz
    assert _c_array("oracle/jxlo_vardct.h", "kCoeffFreqContext") == freq
    assert _c_array("oracle/jxlo_vardct.h", "kCoeffNumNonzeroContext") == nnz
    assert _c_array("libjxl_amd/csrc/hip/jxl_hip_kernels.h", "c_coeff_nnz_ctx")[1:] == nnz[1:]
    assert _c_array("libjxl_amd/csrc/hip/jxl_hip_kernels.h", "c_coeff_freq_ctx")[1:] == freq[1:]
    # the lane kernel's arithmetic form of kCoeffFreqContext (jxl_hip_entropy_lanes.h): min(b - 1, 7 + b / 2, 15 + b / 4)
    assert [min(b - 1, 7 + b // 2, 15 + b // 4) for b in range(1, 64)] == freq[1:]
    for path, name in (("libjxl_amd/csrc/host/jxh_vardct.h", "kStrategyOrder"), (hip, "kStrategyOrder"),
                       ("oracle/jxlo_vardct.h", "kStrategyOrder")):
        assert _c_array(path, name) == ref["kStrategyOrder"], path
    for path in ("libjxl_amd/csrc/host/jxh_vardct.h", "oracle/jxlo_vardct.h"):
        assert _c_array(path, "kDefault") == ref["kDefaultCtxMap"], path
        assert _c_array(path, "kCoveredX") == ref["covered_blocks_x"] and _c_array(path, "kCoveredY") == ref["covered_blocks_y"], path
        assert _c_array(path, "kStrategyQuantTable") == ref["strategy_to_quant_table"], path
    assert _c_array(hip, "kStrategyQuantTable") == ref["strategy_to_quant_table"]
    assert _c_array(hip, "kCoveredX") == ref["covered_blocks_x"] and _c_array(hip, "kCoveredY") == ref["covered_blocks_y"]
    # no table of these is typed a second time in the HIP layer: the device's copies are initialised from the objects above
    hip_text = "".join(open(os.path.join(ROOT, "libjxl_amd/csrc/hip", n)).read() for n in sorted(os.listdir(os.path.join(ROOT, "libjxl_amd/csrc/hip"))))
    for name in ("kCoveredX", "kCoveredY", "kStrategyOrder", "kStrategyQuantTable"):
        assert hip_text.count(", ".join(map(str, _c_array(hip, name)))) == 1, name
    for dev, host in (("c_covered_x", "kCoveredX"), ("c_covered_y", "kCoveredY"), ("c_strategy_order", "kStrategyOrder"),
                      ("c_strategy_qtable", "kStrategyQuantTable"), ("c_log2_covered", "kLog2Covered"), ("c_strategy_info", "kStrategyInfo")):
        assert "%s = %s;" % (dev, host) in hip_text, dev
    # the packed word of k_entropy_uni and log2 covered are built from those objects by the constant expressions of
    # MakeStrategyInfo / MakeLog2Covered, read here as written: every field of every strategy against the fixture
    text = open(os.path.join(ROOT, hip)).read()
    assert "r.v[s] = uint32_t(kCoveredX[s]) | uint32_t(kCoveredY[s]) << 8 | uint32_t(kLog2Covered[s]) << 16 | uint32_t(kStrategyOrder[s]) << 24;" in text
    assert "r.v[s] = uint8_t(Log2CoveredX(s) + Log2CoveredY(s));" in text
    import re
    pinned = {int(s_): int(w, 16) for s_, w in re.findall(r"kStrategyInfo\[(\d+)\] == (0x[0-9A-Fa-f]+)", text)}  # (the header's static_asserts)
    assert len(pinned) >= 3
    for s_, w in pinned.items():
        cx, cy = ref["covered_blocks_x"][s_], ref["covered_blocks_y"][s_]
        assert (w & 0xFF, (w >> 8) & 0xFF, w >> 24) == (cx, cy, ref["kStrategyOrder"][s_]) and 1 << ((w >> 16) & 0xFF) == cx * cy, s_
    for s_ in range(27):  # log2 covered = log2(cx * cy) is a whole number for every strategy: the sum of the two log2 is exact
        cx, cy = ref["covered_blocks_x"][s_], ref["covered_blocks_y"][s_]
        assert cx & (cx - 1) == 0 and cy & (cy - 1) == 0, s_


def test_enum_colour_encodings_of_lossless_images_are_reported(built):
    """A non-XYB image's colour encoding is metadata: the samples pass through, JxlDecoderGetColorAsEncodedProfile hands the
    coded fields out (color_encoding_internal.cc:144-200: Rec.2100 PQ; custom chromaticities with a gamma)."""
    import ctypes

    class CE(ctypes.Structure):
        _fields_ = [("color_space", ctypes.c_int), ("white_point", ctypes.c_int), ("white_point_xy", ctypes.c_double * 2),
                    ("primaries", ctypes.c_int), ("red", ctypes.c_double * 2), ("green", ctypes.c_double * 2), ("blue", ctypes.c_double * 2),
                    ("transfer_function", ctypes.c_int), ("gamma", ctypes.c_double), ("rendering_intent", ctypes.c_int)]

    J = built
    L = J.lib()
    vp = ctypes.c_void_p
    L.JxlDecoderCreate.restype = vp
    L.JxlDecoderCreate.argtypes = [vp]
    for n in ("JxlDecoderDestroy", "JxlDecoderProcessInput", "JxlDecoderCloseInput"):
        getattr(L, n).argtypes = [vp]
    L.JxlDecoderSubscribeEvents.argtypes = [vp, ctypes.c_int]
    L.JxlDecoderSetInput.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    L.JxlDecoderGetColorAsEncodedProfile.argtypes = [vp, ctypes.c_int, ctypes.POINTER(CE)]
    img = J.synth_image(64, 48, seed=2)

    def encoded_profile(**kw):
        J.set_color_encoding(**kw)
        try:
            data = J.encode_lossless(img)
        finally:
            J.set_color_encoding(None)
        J.ModFrame(data).close()  # the front-end plans it like any lossless frame
        dec = L.JxlDecoderCreate(None)
        L.JxlDecoderSubscribeEvents(dec, 0x100)
        L.JxlDecoderSetInput(dec, data, len(data))
        L.JxlDecoderCloseInput(dec)
        assert L.JxlDecoderProcessInput(dec) == 0x100
        ce = CE()
        assert L.JxlDecoderGetColorAsEncodedProfile(dec, 0, ctypes.byref(ce)) == 0
        L.JxlDecoderDestroy(dec)
        return ce

    ce = encoded_profile(white_point=1, primaries=9, transfer_function=16, intent=0)
    assert (ce.color_space, ce.white_point, ce.primaries, ce.transfer_function, ce.rendering_intent) == (0, 1, 9, 16, 0)
    assert tuple(ce.red) == (0.708, 0.292) and tuple(ce.blue) == (0.131, 0.046)
    xy = [0.31, 0.33, 0.64, 0.33, 0.3, 0.6, 0.15, 0.06]
    ce = encoded_profile(white_point=2, primaries=2, gamma=0.45455, xy=xy)
    assert (ce.white_point, ce.primaries, ce.transfer_function) == (2, 2, 65535) and abs(ce.gamma - 0.45455) < 1e-7
    got = list(ce.white_point_xy) + list(ce.red) + list(ce.green) + list(ce.blue)
    assert max(abs(a - b) for a, b in zip(got, xy)) < 1e-6
    ce = encoded_profile(white_point=11, primaries=11, transfer_function=17)  # DCI white, P3, DCI transfer function
    assert abs(ce.white_point_xy[0] - 0.314) < 1e-9 and tuple(ce.green) == (0.265, 0.690) and ce.transfer_function == 17


_HALO_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
from libjxl_amd import sharding
world = %(world)d
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=world)
rank = dist.get_rank()
# a frame of `world` bands of 4 rows x 6 columns; row y holds the value y everywhere; each rank owns rows [4r, 4r + 4)
# and has room for 2 halo rows either side
H, W, HALO = 4, 6, 2
plane = torch.full((H * world, W), -1.0)
plane[H * rank:H * (rank + 1)] = torch.arange(H * rank, H * (rank + 1), dtype=torch.float32)[:, None]
def pack(side):
    y0 = H * rank if side == 0 else H * (rank + 1) - HALO
    return plane[y0:y0 + HALO].clone()
def unpack(side, block):
    y0 = H * rank - HALO if side == 0 else H * (rank + 1)
    plane[y0:y0 + HALO] = block
def send(block, peer):
    dist.send(block, peer)
def recv(peer):
    t = torch.empty((HALO, W))
    dist.recv(t, peer)
    return t
sharding.exchange_halos(rank, world, pack, unpack, send, recv)
lo, hi = max(0, H * rank - HALO), min(H * world, H * (rank + 1) + HALO)
want = torch.arange(lo, hi, dtype=torch.float32)[:, None].expand(hi - lo, W)
ok = bool(torch.equal(plane[lo:hi], want)) and bool((plane[:lo] == -1).all()) and bool((plane[hi:] == -1).all())
print("HALO", rank, ok)
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world", [2, 3])
def test_halo_exchange_schedule_gloo(built, tmp_path, world):
    """sharding.exchange_halos over blocking point-to-point sends (gloo here, RCCL between GPUs): every rank ends up with
    exactly its neighbours' boundary rows beside its band, nothing else moves, and the even / odd ordering does not
    deadlock (2 and 3 ranks: an end rank, a middle rank)."""
    pytest.importorskip("torch")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "h.py"
    script.write_text(_HALO_WORKER % {"root": ROOT, "port": port, "world": world})
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    for r in range(world):
        assert "HALO %d True" % r in outs[r], outs[r]


def test_oracle_and_host_read_a_preview_frame(built):
    """The image header's PreviewHeader (headers.cc:155-183) and the preview as the codestream's first frame, sized by it
    (frame_header.h:450-463, decode.cc:1266-1268): oracle and host front-end, no GPU."""
    import jxlo
    J = built
    img, pv = J.synth_image(600, 400, seed=3), J.synth_image(75, 50, seed=4)
    for preview in (pv, J.synth_image(80, 48, seed=5)):  # (sizes coded directly, and as multiples of 8)
        data = J.encode_with_preview(img, preview)
        o = jxlo.Decoded(data, dumps=False, preview=True)
        assert o.rgb8.shape == preview.shape and np.abs(o.rgb8.astype(int) - preview).mean() < 6
        o.close()
        o = jxlo.Decoded(data, dumps=False)
        assert o.rgb8.shape == img.shape and np.abs(o.rgb8.astype(int) - img).mean() < 4
        o.close()
        f = J.Frame(data)  # the first frame of the codestream: the preview
        assert (f.info["xsize"], f.info["ysize"]) == (preview.shape[1], preview.shape[0])
        f.close()


def test_partial_frame_plan_counts_the_passes_that_have_arrived(built):
    """jxlamd_frame_parse_partial_at + jxlamd_frame_complete_passes (dec_frame.cc:620-680, dec_frame.h:186-200): from a prefix
    of a two-pass frame every group is planned with its leading passes whose sections are whole; the count every group has
    grows with the bytes and reaches the frame's number of passes exactly at its end; groups_present counts the groups with
    at least one pass."""
    import ctypes
    J = built
    L = J.lib()
    data = J.encode_rgb8(J.synth_image(1100, 800, seed=9), num_passes=2)
    L.jxlamd_frame_parse_partial_at.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32)]
    L.jxlamd_frame_complete_passes.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.jxlamd_frame_complete_passes.restype = ctypes.c_uint32
    L.jxlamd_frame_free.argtypes = [ctypes.c_void_p]
    info = (ctypes.c_uint32 * 10)()
    seen, present_seen, first_ok = [], [], None
    for have in list(range(2000, len(data), 4000)) + [len(data) - 1]:
        f, present = ctypes.c_void_p(), ctypes.c_uint32()
        r = L.jxlamd_frame_parse_partial_at(data[:have], have, 0, 0, None, None, ctypes.byref(f), ctypes.byref(present))
        if r:  # (the DC image is not whole yet)
            assert first_ok is None, have
            continue
        first_ok = first_ok or have
        complete = L.jxlamd_frame_complete_passes(f, have, info)
        assert list(info)[:2] == [2, 0]
        # the same plan asked about more bytes than it was parsed from: the table of contents answers
        assert L.jxlamd_frame_complete_passes(f, len(data), info) == 2
        assert L.jxlamd_frame_complete_passes(f, 0, info) == 0
        seen.append(complete)
        present_seen.append(present.value)
        L.jxlamd_frame_free(f)
    assert seen == sorted(seen) and seen[0] == 0 and 1 in seen and seen[-1] < 2, seen  # (one byte short of the end: the last section is cut)
    assert present_seen == sorted(present_seen) and present_seen[0] < 20 and present_seen[-1] == 20, present_seen  # 5 x 4 groups
    f = J.Frame(data)
    assert L.jxlamd_frame_complete_passes(f._h, 1, info) == 2  # a whole frame: all of its passes
    f.close()


def test_float_and_deep_integer_modular_streams_on_the_host(built):
    """CPU half of tests/test_gpu_modular.py::test_float_and_deep_integer_samples: the stream writer's float / deep-integer
    Modular streams decode (oracle) to the integers they were made from, the product's host front-end plans them (it refused
    them before round 4), and the NumPy reading of dec_modular.cc:128-185 agrees with NumPy's own binary16 widening on all
    65 536 patterns."""
    import importlib.util
    import jxlo
    J = built
    spec = importlib.util.spec_from_file_location("tgm", os.path.join(ROOT, "tests", "test_gpu_modular.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    every = np.arange(65536, dtype=np.int32)
    assert np.array_equal(m.np_sample_to_float(every, 16, 5).view(np.uint32),
                          every.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32))
    assert m.np_sample_to_float(np.array([0x3F800000, -(1 << 31)]), 32, 8).view(np.uint32).tolist() == [0x3F800000, 0x80000000]
    for kind, flags, (w, h), nc in (("f32", 4, (300, 70), 3), ("f16", 16, (280, 300), 1), ("f24", 0, (260, 40), 3), ("u24", 8, (300, 260), 3)):
        v, bits, exp_bits = m._deep_samples(kind, h, w, nc, seed=3)
        data = J.encode_lossless_samples(v, bits, exp_bits, flags=flags)
        o = jxlo.Decoded(data, dumps=True)
        assert o.info["bits"] == bits
        assert np.array_equal(o.buffer("modular").reshape(nc, h, w), np.moveaxis(v, -1, 0))
        o.close()
        J.ModFrame(data).close()
