"""The device's AC coefficient walk, both ways, against tests/ac_walk_np.py, the plain reading of the reference's text
(tests/test_ac_walk.py holds the oracle, the stream writer and the reading's own misreadings to it on the CPU):
  decode    the coefficients over the used slots of every group, kend where the frame is kept in scan order, the end bit of
            every section, no error flag; the oracle only parses the tables the reading is given. The list runs in this
            process, where every frame takes the kernel the library chooses for it, and once more in one child process under
            JXLHIP_ENTROPY=1, where none takes the lane kernel (the setting is latched per process). DEVICE_CASES says which
            kernel each case must take in either process, and that is asserted: k_entropy_lanes (with the host-built block
            records), k_entropy_uni, k_entropy_ans and k_entropy_generic each decode a horizontally subsampled frame with
            quant-field thresholds, where the quant field's column matters;
  tokenise  k_enc_tok_count / k_enc_tok_emit on the device's own forward output, under the descriptor variants of the CPU
            test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_ac_walk as C

pytestmark = pytest.mark.gpu

LANES, UNI, ANS, GENERIC = 0, 1, 2, 3  # HipContext.entropy_route
# case: (kernel in this process, kernel under JXLHIP_ENTROPY=1). A one-pass frame of the lane kernel is kept in scan order
# and has extents (kend); every other frame is kept in the natural layout.
DEVICE_CASES = {
    "rgb8": (LANES, UNI),
    "random_bctx_orders_hist3": (LANES, UNI),
    "mixed_520": (LANES, UNI),
    "passes2": (LANES, UNI),
    "subsampled0_bctx1": (LANES, UNI),  # 4:2:0
    "subsampled3_bctx1": (LANES, UNI),  # 0b011011: luma subsampled too
    "subsampled0_bctx1_prefix_lz77": (GENERIC, GENERIC),
    "subsampled0_bctx1_clusters": (LANES, ANS),  # (the lane kernel reads alias tables of any size in place)
    "prefix_lz77": (GENERIC, GENERIC),
    "passes2_hist2_prefix_lz77": (GENERIC, GENERIC),  # the section-per-workgroup kernels' passes and selector
    "passes2_hist2_clusters": (LANES, ANS),
    "hist2_clusters": (LANES, ANS),
    "rgba": (LANES, UNI),
    "int32": (LANES, UNI),
}


def expected(J, name):
    """What the reading says the device must hold, as plain arrays (the child process loads them from a file)."""
    c = C.case(J, name)
    T = c["tables"]
    ng, npass = T["num_groups"], T["num_passes"]
    coeffs = np.stack([r["coeffs"] for r in c["groups"]])
    used = np.array([r["used"] for r in c["groups"]], np.int64)
    last0 = np.concatenate([r["last"][0] for r in c["groups"]])
    end_rel = np.array([[c["groups"][g]["end_bits"][p] - 8 * T["sections"][p][g][1] for g in range(ng)] for p in range(npass)], np.int64)
    return dict(data=np.frombuffer(c["data"], np.uint8), coeffs=coeffs, used=used, last0=last0, end_rel=end_rel,
                int32=np.int64(name == "int32"))  # (the case that must be in int32 storage; the others as the host decides)


def device_check(J, name, e, route):
    f = J.Frame(e["data"].tobytes(), threads=2)
    c = J.HipContext()
    try:
        assert f.info["coef_bits"] == 32 or not int(e["int32"]), name
        c.upload(f)
        assert c.entropy_route() == route, (name, c.entropy_route())
        c.run_entropy()
        c.sync()
        r, flags = c.errors()
        assert r == 0 and not any(flags), (name, flags)
        co = c.download("coeffs")
        assert co.dtype == (np.int32 if f.info["coef_bits"] == 32 else np.int16)
        co = co.astype(np.int32)
        for g, n in enumerate(e["used"]):
            bad = np.argwhere(co[g][:, :n] != e["coeffs"][g][:, :n])
            assert bad.size == 0, "%s group %d: %d coefficients differ from the reading's, first at channel %d slot %d" % (
                name, g, len(bad), bad[0][0], bad[0][1])
        assert np.array_equal(c.section_end_bits(), e["end_rel"]), name
        if route == LANES and e["end_rel"].shape[0] == 1:
            assert np.array_equal(c.download("kend").astype(np.int64), e["last0"]), name
        else:  # the natural layout: there are no extents
            with pytest.raises(J.JxlAmdError):
                c.download("kend")
    finally:
        c.close()
        f.close()


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_device_coefficients_extents_and_end_bits_are_the_readings(built, name):
    device_check(built, name, expected(built, name), DEVICE_CASES[name][0])


def test_the_same_list_on_the_section_per_wave_kernels(built, tmp_path):
    J = built
    path = os.path.join(str(tmp_path), "expected.npz")
    flat = {}
    for name in DEVICE_CASES:
        for k, v in expected(J, name).items():
            flat[name + "/" + k] = v
    np.savez(path, **flat)
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import numpy as np, libjxl_amd as J, test_gpu_ac_walk as G\n"
            "z = np.load(%r)\n"
            "for name in G.DEVICE_CASES:\n"
            "    G.device_check(J, name, {k: z[name + '/' + k] for k in ('data', 'coeffs', 'used', 'last0', 'end_rel', 'int32')},\n"
            "                   G.DEVICE_CASES[name][1])\n"
            "print('ok')\n") % (root, os.path.join(root, "oracle"), here, path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, JXLHIP_ENTROPY="1"))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.parametrize("size,distance,mode", C.TOKEN_MODELS)
def test_the_device_tokeniser_gives_the_readings_tokens(built, size, distance, mode):
    J = built
    ctx = J.HipContext()
    try:
        model = J.enc_forward_model(J.synth_image(*size), ctx, distance=distance, strategy_mode=mode)
        C.check_tokens(J, ctx, model)
    finally:
        ctx.close()


def test_upload_rejects_a_subsampled_frame_whose_varblocks_are_not_in_raster_order(built):
    """The entropy stage finds the block at a subsampled channel's own column a few entries back in the row, so
    jxlhip_frame_upload must refuse a descriptor where that is not so (JXLHIP_ERR_INVALID_ARGUMENT = 1). The same exchange
    in a 4:4:4 frame, where nothing depends on the order, is taken: it is this validation that refuses."""
    import ctypes
    J = built
    L = J.lib()
    L.jxlamd_frame_debug_swap_blocks.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    for kw, refused in ((dict(color_transform=2, chroma_subsampling=4), True), (dict(), False)):
        f = J.Frame(J.encode_rgb8(J.synth_image(64, 32, seed=3), strategy_mode=0, **kw))
        c = J.HipContext()
        try:
            c.upload(f)  # as parsed: accepted
            assert L.jxlamd_frame_debug_swap_blocks(f._h, 0, f.info["xsize_blocks"] - 1) == 0  # block 0 now claims column 7
            if refused:
                with pytest.raises(J.JxlAmdError, match="code 1"):
                    c.upload(f)
            else:
                c.upload(f)
        finally:
            c.close()
            f.close()
