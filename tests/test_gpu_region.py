"""GPU tests (-m gpu) of the region decode: only the 256 x 256 groups a box reads are uploaded, as a frame of their own
(Frame.plan_window, HipContext.upload_window, k_dc_window, torch_io.decode_*(region=True)).

Everything here is exact. The window runs the kernels of a whole decode on the same inputs, so every stage of the window
equals the same stage of the whole frame bit for bit: the DC planes everywhere, the coefficients group by group, the
filtered planes and the f32 pixels at every pixel at least H (the reach of the frame's loop filters, 0 to 7) away from a
window edge that is not a frame edge. A difference is a placement bug (halo, apron, origin), never a tolerance to widen.
The whole frame is decoded once per stream and shared."""
import ctypes

import numpy as np
import pytest
import torch

from libjxl_amd import torch_io

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_INT = {torch.float16: (torch.int16, np.int16, 0x7B5A), torch.bfloat16: (torch.int16, np.int16, 0x7B5A),
        torch.float32: (torch.int32, np.int32, 0x7B5A7B5A), torch.uint8: (torch.uint8, np.uint8, 0x5A)}
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Canvas:
    """A tensor of the output inside a larger sentinel-filled allocation (the helper of tests/test_gpu_resample.py, copied)."""

    def __init__(self, dtype, layout, nc, h, w, padded, device="cuda"):
        self.dtype, self.layout = dtype, layout
        it, self.np_int, self.sentinel = _INT[dtype]
        ph, pw = (h + 5, w + 3) if padded else (h, w)
        self.offset = 1 if padded else 0
        self.shape = (nc, ph, pw) if layout == "CHW" else (ph, pw, nc)
        n = self.offset + nc * ph * pw + (2 if padded else 0)
        self.flat = torch.empty(n, dtype=dtype, device=device)
        self.flat.view(it).fill_(self.sentinel if dtype != torch.uint8 else 0x5A)
        self.cut = (slice(None), slice(0, h), slice(0, w)) if layout == "CHW" else (slice(0, h), slice(0, w), slice(None))
        self.tensor = self.flat[self.offset:self.offset + nc * ph * pw].view(self.shape)[self.cut]
        self.it = it

    def got(self):
        torch.cuda.synchronize()
        return self.flat.view(self.it).cpu().numpy()

    def image(self):
        """([H, W, C] integer view of the output, whether everything around it kept the sentinel)."""
        full = self.got().copy()
        n = int(np.prod(self.shape))
        view = full[self.offset:self.offset + n].reshape(self.shape)
        img = view[self.cut].copy()
        view[self.cut] = self.sentinel
        return (img.transpose(1, 2, 0) if self.layout == "CHW" else img), bool((full == self.np_int(self.sentinel)).all())


def _halo(gab, epf):
    return (1 if gab else 0) + (3 if epf >= 3 else 0) + (2 if epf >= 1 else 0) + (1 if epf >= 2 else 0)


def _bits(t):
    """A tensor's bit patterns on the host (NaN-proof equality)."""
    torch.cuda.synchronize()
    return t.contiguous().view(_INT[t.dtype][0]).cpu().numpy()


# ------------------------------------------------------------------------------------------------ stage by stage
STAGE_CASES = {
    "epf1": dict(epf_iters=1),
    "epf3_gab": dict(epf_iters=3, gab=1),
    "h0": dict(epf_iters=0, gab=0),
    "skip_dc_smoothing": dict(skip_dc_smoothing=1),
    "passes2": dict(num_passes=2),
    "prefix": dict(ac_code_mode=1),
}


def _stage_boxes(H):
    """The windows of the host list (tests/test_region_host.py) on the 1000 x 700 frame."""
    boxes = [(300, 300, 100, 100),               # interior of one group
             (256 + H, 300, 100, 100),           # H behind a boundary: one group
             (300, 300, 512 - H - 300 + 1, 50),  # one pixel past the far side: two columns
             (200, 200, 400, 400),               # across a four-group corner and more: 3 x 3 groups
             (600, 400, 1, 1),                   # one pixel
             (990, 690, 10, 10),                 # the ragged corner
             (0, 0, 40, 40)]                     # the frame's own corner
    if H:
        boxes.append((256 + H - 1, 300, 100, 100))  # H - 1 behind it: two columns
    return boxes


def _run_stages(J, c, upload):
    c.set_option("keep_dc", 1)
    c.set_option("keep_filtered", 1)
    c.set_output_format(0, 3)
    upload()
    c.run_all()
    r, flags = c.errors()
    assert r == 0 and not any(flags)
    fi = c.frame_info
    return dict(dc=c.download("dc").reshape(3, fi["ysize_blocks"], fi["xsize_blocks"]).copy(), coeffs=c.download("coeffs").copy(), filtered=c.download("xyb_filtered").copy(), pixels=c.pixels().copy())


def _whole(J, name):
    def make():
        data = J.encode_rgb8(J.synth_image(1000, 700, seed=41), **STAGE_CASES[name])
        f = J.Frame(data)
        c = J.HipContext()
        try:
            out = _run_stages(J, c, lambda: c.upload(f))
            out["data"], out["info"] = data, dict(f.info)
        finally:
            c.close()
            f.close()
        return out
    return _cached(("whole", name), make)


@pytest.mark.parametrize("name", sorted(STAGE_CASES))
def test_every_stage_of_a_window_is_the_frames(built, name):
    J = built
    whole = _whole(J, name)
    info = whole["info"]
    H = _halo(info["gab"], info["epf_iters"])
    if name == "epf3_gab":
        assert H == 7
    if name == "h0":
        assert H == 0
    if name == "passes2":
        assert info["num_passes"] == 2
    xb, yb = info["xsize_blocks"], info["ysize_blocks"]
    f = J.Frame(whole["data"])
    c = J.HipContext()
    try:
        for box in _stage_boxes(H):
            w = f.plan_window(box)
            assert w["reason"] == 0, (box, w)
            got = _run_stages(J, c, lambda: c.upload_window(f, w))
            fi = c.frame_info
            assert fi["num_groups"] == w["groups_taken"] == len(c.errors()[1]) and (fi["xsize"], fi["ysize"]) == (w["xsize"], w["ysize"])
            x0, y0, xs, ys = w["x0"], w["y0"], w["xsize"], w["ysize"]
            bx0, by0, bxs, bys = x0 // 8, y0 // 8, (xs + 7) // 8, (ys + 7) // 8
            # the DC planes: the crop of the frame's, bit for bit
            assert got["dc"].shape == (3, bys, bxs) and whole["dc"].shape == (3, yb, xb)
            assert np.array_equal(got["dc"].view(np.int32), whole["dc"][:, by0:by0 + bys, bx0:bx0 + bxs].view(np.int32)), (name, box)
            # the coefficients: window group i is the frame's group
            assert got["coeffs"].shape[0] == len(w["groups"])
            # (a group's blocks fill the head of its 65536 slots per channel; behind them a ragged group's slots are never
            # written and hold what the buffer held before)
            for i, g in enumerate(w["groups"]):
                used = 64 * min(32, xb - 32 * (g % 4)) * min(32, yb - 32 * (g // 4))
                assert np.array_equal(got["coeffs"][i][:, :used], whole["coeffs"][g][:, :used]), (name, box, i, g)
                assert np.any(got["coeffs"][i][:, :used])
            # filtered planes and f32 pixels, H away from the window's edges that are not the frame's
            l, t = (H if x0 else 0), (H if y0 else 0)
            r, b = (xs - H if x0 + xs < 1000 else xs), (ys - H if y0 + ys < 700 else ys)
            assert np.array_equal(got["filtered"][:, t:b, l:r].view(np.int32), whole["filtered"][:, y0 + t:y0 + b, x0 + l:x0 + r].view(np.int32)), (name, box)
            assert got["pixels"].shape == (ys, xs, 3)
            assert np.array_equal(got["pixels"][t:b, l:r].view(np.int32), whole["pixels"][y0 + t:y0 + b, x0 + l:x0 + r].view(np.int32)), (name, box)
            # the caller's box lies inside that region, and is the frame's box
            u0, v0, bw, bh = w["box"]
            assert l <= u0 and u0 + bw <= r and t <= v0 and v0 + bh <= b
            assert np.array_equal(got["pixels"][v0:v0 + bh, u0:u0 + bw].view(np.int32),
                                  whole["pixels"][box[1]:box[1] + bh, box[0]:box[0] + bw].view(np.int32))
    finally:
        c.close()
        f.close()


# ------------------------------------------------------------------------------------------------ k_dc_window alone
DCW_FRAME = (260, 12)  # blocks: two DC groups across
DCW_STEP = (np.float32(1 / 4096), np.float32(1 / 512), np.float32(1 / 256))
DCW_CFL = (np.float32(0.0234375), np.float32(0.935669))
DCW_WINDOWS = [(0, 0, 1, 1), (259, 0, 1, 1), (0, 11, 1, 1), (259, 11, 1, 1),  # 1 x 1 at each frame corner
               (100, 4, 3, 3),      # interior
               (10, 1, 65, 9),      # one tile plus a ragged column and row
               (250, 2, 10, 8),     # across block column 256
               (0, 0, 260, 12)]     # the whole plane


def _dcw_planes():
    """Hand-made coded integers: slow ramps on the left (their smoothing residual is a fraction of a step, so the samples are
    smoothed), the same with noise of three units on the right (most of those keep their value: the gap passes 3 / 4 step).
    A float64 run of the rule on the CPU put 51 % and 77 % of the interior on the smoothed side for the two shift pairs."""
    rng = np.random.default_rng(12)
    xs, ys = DCW_FRAME
    y, x = np.mgrid[0:ys, 0:xs]
    q = np.stack([np.rint(0.3 * x + 0.2 * y), np.rint(900 * np.cos(x / 97.0 + y / 45.0)), np.rint(0.25 * y - 0.15 * x)])
    return (q + rng.integers(-3, 4, q.shape) * (x >= 130)[None]).astype(np.int32)


def _dequant_f32(q, ep):
    """DequantDC in float32 NumPy, products unfused as in DcDequantSample: the step of a DC group is step / 2^shift."""
    xs = q.shape[2]
    shift = np.asarray(ep, np.uint8)[np.arange(xs) >> 8]
    mul = (np.float32(1) / (np.uint32(1) << shift).astype(np.float32)).astype(np.float32)[None, :]
    inq = [q[c].astype(np.float32) * (DCW_STEP[c] * mul).astype(np.float32) for c in range(3)]
    out = np.empty(q.shape, np.float32)
    out[1] = inq[1]
    out[0] = (inq[1] * DCW_CFL[0]).astype(np.float32) + inq[0]
    out[2] = (inq[1] * DCW_CFL[1]).astype(np.float32) + inq[2]
    return out


@pytest.mark.parametrize("ep", [(0, 3), (2, 1)], ids=["shifts03", "shifts21"])
def test_dc_window_kernel_alone(built, ep):
    """jxlhip_debug_dc_window on hand-made planes of 260 x 12 blocks (the test encoders write precision shift 0). Smoothing
    off: the float32 NumPy statement of DequantDC, exactly. Smoothing on: every window is the crop of the whole-plane
    result, and the frame's border samples are the unsmoothed values. The entry's sentinel behind the planes stays (a write
    there is JXLHIP_ERR_GUARD = 5, which _check raises)."""
    J = built
    q = _dcw_planes()
    want = _dequant_f32(q, ep)
    c = J.HipContext()
    try:
        def run(win, smoothing):
            return c.debug_dc_window(q, win, ep, DCW_STEP, float(DCW_CFL[0]), float(DCW_CFL[1]), smoothing)
        whole = run((0, 0, 260, 12), True)
        assert whole.shape == (3, 12, 260)
        border = np.zeros((12, 260), bool)
        border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
        assert np.array_equal(whole[:, border].view(np.int32), want[:, border].view(np.int32))
        changed = (whole.view(np.int32) != want.view(np.int32)).any(axis=0)
        assert changed[~border].mean() > 0.2 and (~changed[~border]).mean() > 0.02  # both branches of the smoothing are met
        for win in DCW_WINDOWS:
            x0, y0, xs, ys = win
            plain = run(win, False)
            assert np.array_equal(plain.view(np.int32), want[:, y0:y0 + ys, x0:x0 + xs].view(np.int32)), win
            smooth = run(win, True)
            assert np.array_equal(smooth.view(np.int32), whole[:, y0:y0 + ys, x0:x0 + xs].view(np.int32)), win
        # refused on the host: a wrong apron, a missing precision byte
        for kw in (dict(apron=(99, 3, 4, 5)), dict(apron=(99, 3, 5, 6))):
            with pytest.raises(J.JxlAmdError):
                c.debug_dc_window(q, (100, 4, 3, 3), ep, DCW_STEP, 0.0, 1.0, True, **kw)
        with pytest.raises(J.JxlAmdError):
            c.debug_dc_window(q, (250, 2, 10, 8), ep[:1], DCW_STEP, 0.0, 1.0, True)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_stream(J):
    return _cached("e2e", lambda: J.encode_rgb8(J.synth_image(1000, 700, seed=41), epf_iters=3, gab=1))


E2E_BOXES = {
    "interior": (300, 300, 100, 100),
    "four_group_corner": (200, 200, 120, 110),
    "near_left": (256 + 6, 300, 100, 100),
    "at_left": (256 + 7, 300, 100, 100),
    "near_right": (300, 300, 512 - 6 - 300, 60),
    "at_right": (300, 300, 512 - 7 - 300, 60),
    "near_top": (300, 256 + 6, 100, 100),
    "near_bottom": (300, 300, 60, 512 - 6 - 300),
    "ragged_corner": (900, 640, 100, 60),
    "one_pixel": (600, 400, 1, 1),
    "whole": (0, 0, 1000, 700),
}


@pytest.mark.parametrize("name", sorted(E2E_BOXES))
def test_region_equals_the_whole_decode(built, name):
    """decode_to_tensor(size=(64, 48), box=b, float32): region=True and region=False give the same bits; nothing outside the
    tensor is written."""
    J = built
    data = _e2e_stream(J)
    box = E2E_BOXES[name]
    ref = torch_io.decode_to_tensor(data, size=(64, 48), box=box, dtype=torch.float32, region=False)
    cv = Canvas(torch.float32, "CHW", 3, 64, 48, True)
    torch_io.decode_to_tensor(data, size=(64, 48), box=box, dtype=torch.float32, region=True, out=cv.tensor)
    img, clean = cv.image()
    assert clean
    assert np.array_equal(img.transpose(2, 0, 1), _bits(ref)), name
    assert not np.isnan(ref.cpu().numpy()).any() and float(ref.abs().max()) > 0


@pytest.mark.parametrize("dtype,affine,layout", [(torch.float16, True, "CHW"), (torch.uint8, False, "HWC"), (torch.bfloat16, True, "HWC")],
                         ids=["f16_mean_std", "u8", "bf16_mean_std"])
def test_region_equals_the_whole_decode_in_other_types(built, dtype, affine, layout):
    J = built
    data = _e2e_stream(J)
    kw = dict(mean=MEAN, std=STD, clamp=True) if affine else {}
    for box in (E2E_BOXES["near_left"], E2E_BOXES["four_group_corner"]):
        ref = torch_io.decode_to_tensor(data, size=(64, 48), box=box, dtype=dtype, layout=layout, region=False, **kw)
        cv = Canvas(dtype, layout, 3, 64, 48, True)
        torch_io.decode_to_tensor(data, size=(64, 48), box=box, dtype=dtype, layout=layout, region=True, out=cv.tensor, **kw)
        img, clean = cv.image()
        assert clean
        want = _bits(ref)
        assert np.array_equal(img, want.transpose(1, 2, 0) if layout == "CHW" else want), box


def test_orientation(built):
    """A 600 x 300 stream whose output undoes orientation 6 (rows of the output are columns of the image, 300 wide and 600
    high): the window is the one the box maps to, and the tensors are equal. Through torch_io (which undoes no orientation)
    a stream tagged with orientation 6 decodes equally too."""
    J = built
    J.set_orientation(6)
    try:
        data = J.encode_rgb8(J.synth_image(600, 300, seed=116), epf_iters=1, gab=1)
    finally:
        J.set_orientation(1)
    box = (20, 30, 100, 90)  # columns 20..120 of the output are rows 300 - 120 .. 300 - 20 of the frame, rows 30..120 its columns
    f = J.Frame(data)
    try:
        w = f.plan_window(box, orientation=6)
        assert w["reason"] == 0 and w["groups"] == [0, 3] and (w["x0"], w["y0"], w["xsize"], w["ysize"]) == (0, 0, 256, 300)
        assert w["box"] == (20, 30, 100, 90)  # (the window keeps the frame's rows, and its columns start at the frame's)
        w2 = f.plan_window((20, 300, 100, 90), orientation=6)  # rows 300..390 of the output: columns 300..390 of the frame
        assert w2["groups"] == [1, 4] and w2["box"] == (20, 300 - 256, 100, 90)
        outs = []
        for plan in (None, w, w2):
            for b in ((box,) if plan is not w2 else ((20, 300, 100, 90),)):
                c = J.HipContext()
                try:
                    c.set_output_orientation(6)
                    t = torch.zeros((3, 40, 24), dtype=torch.float32, device="cuda")
                    if plan is None:
                        torch_io.bind_resized(c, t, "CHW", b)
                        c.upload(f)
                    else:
                        torch_io.bind_resized(c, t, "CHW", plan["box"])
                        c.upload_window(f, plan)
                    c.run_all()
                    assert c.errors()[0] == 0
                    outs.append(_bits(t))
                finally:
                    c.close()
        assert np.array_equal(outs[0], outs[1]) and outs[0].any()
        c = J.HipContext()
        try:
            c.set_output_orientation(6)
            t = torch.zeros((3, 40, 24), dtype=torch.float32, device="cuda")
            torch_io.bind_resized(c, t, "CHW", (20, 300, 100, 90))
            c.upload(f)
            c.run_all()
            assert np.array_equal(_bits(t), outs[2])
        finally:
            c.close()
    finally:
        f.close()
    a = torch_io.decode_to_tensor(data, size=(40, 24), box=(300, 20, 100, 90), dtype=torch.float32, region=True)
    b = torch_io.decode_to_tensor(data, size=(40, 24), box=(300, 20, 100, 90), dtype=torch.float32, region=False)
    assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ work
def test_only_the_windows_groups_are_uploaded(built):
    """After upload_window the context is a frame of the window's groups: 1 of 12 for an interior 100 x 100 box of the
    1000 x 700 frame, 2 when the box comes within H of a boundary. (That any 224 x 224 box of a 3840 x 2160 frame takes at
    most 4 of 135 is held on the host: tests/test_region_host.py, tests/c/window_kats.cc.)"""
    J = built
    f = J.Frame(_e2e_stream(J))
    c = J.HipContext()
    try:
        for box, count in (((300, 300, 100, 100), 1), ((256 + 6, 300, 100, 100), 2), ((200, 200, 120, 110), 4)):
            w = f.plan_window(box)
            assert (w["groups_taken"], w["groups_in_frame"]) == (count, 12)
            c.upload_window(f, w)
            assert c.frame_info["num_groups"] == count
            c.run_all()
            r, flags = c.errors()
            assert r == 0 and len(flags) == count
            assert c.download("coeffs").shape[0] == count
        w = f.plan_window(None)
        c.upload_window(f, w)  # a reason: the whole frame, by the route it had
        assert c.frame_info["num_groups"] == 12
        bad = dict(w, reason=0)
        with pytest.raises(J.JxlAmdError):
            c.upload_window(f, bad)  # not a window of this frame: every group is no window
        w = dict(f.plan_window((300, 300, 100, 100)), xsize=255)
        with pytest.raises(J.JxlAmdError):
            c.upload_window(f, w)
    finally:
        c.close()
        f.close()


# ------------------------------------------------------------------------------------------------ whole-frame reasons
def _reason_streams(J):
    img = J.synth_image(600, 300, seed=77)

    def splined():
        J.set_splines([dict(points=[(20, 20), (200, 100), (500, 250)], color=[[30] + [0] * 31, [40] + [0] * 31, [10] + [0] * 31],
                            sigma=[20] + [0] * 31)])
        try:
            return J.encode_rgb8(img)
        finally:
            J.set_splines(None)

    rgba = np.dstack([img, np.full(img.shape[:2], 200, np.uint8)])
    return {
        # name: (stream, channels, the reason or None for a Modular frame)
        "noisy": (lambda: J.encode_rgb8(img, noise=60), 3, "noise"),
        "upsampled": (lambda: J.encode_rgb8(img, upsampling=2), 3, "upsampling"),
        "splined": (splined, 3, "splines"),
        "subsampled": (lambda: J.encode_rgb8(img, color_transform=2, chroma_subsampling=4, strategy_mode=0), 3, "subsampling"),
        "modular": (lambda: J.encode_lossless(img), 3, None),
        "four_channels": (lambda: J.encode_rgba8(rgba, epf_iters=1), 4, "alpha"),
    }


@pytest.mark.parametrize("name", ["noisy", "upsampled", "splined", "subsampled", "modular", "four_channels"])
def test_whole_frame_reasons_keep_the_former_route(built, name):
    J = built
    make, nc, reason = _reason_streams(J)[name]
    data = make()
    box = (300, 40, 64, 64)
    if reason is not None:
        f = J.Frame(data)
        w = f.plan_window(box, nc)
        assert J.WINDOW_REASONS[w["reason"]] == reason and w["box"] == box and w["groups_taken"] == w["groups_in_frame"]
        f.close()
    a = torch_io.decode_to_tensor(data, size=(32, 32), box=box, dtype=torch.float32, channels=nc, region=True)
    b = torch_io.decode_to_tensor(data, size=(32, 32), box=box, dtype=torch.float32, channels=nc, region=False)
    assert np.array_equal(_bits(a), _bits(b)) and _bits(a).any()


def test_a_patched_frame_reports_patches(built):
    """The patched frame is the stream's second (torch_io decodes a stream's first frame): the plan reports the reason."""
    J = built
    img = J.synth_image(600, 300, seed=77)
    data = J.encode_patched(img, J.synth_image(64, 48, seed=3), [dict(x0=4, y0=6, xsize=20, ysize=16, positions=[(250, 170, 2, 0)])],
                            atlas_vardct=True)
    first = J.Frame(data)
    second = J.Frame(data, frame_pos=first.end, frame_index=1)
    try:
        assert J.WINDOW_REASONS[second.plan_window((300, 40, 64, 64))["reason"]] == "patches"
        a = torch_io.decode_to_tensor(data, size=(16, 16), box=(3, 3, 40, 30), dtype=torch.float32, region=True)
        b = torch_io.decode_to_tensor(data, size=(16, 16), box=(3, 3, 40, 30), dtype=torch.float32, region=False)
        assert np.array_equal(_bits(a), _bits(b))
    finally:
        first.close()
        second.close()


# ------------------------------------------------------------------------------------------------ batch
def test_a_batch_of_crops(built):
    """Five frames of different sizes, one of them Modular, one without a box: each out[i] is the single-frame call."""
    J = built
    datas = [_e2e_stream(J),
             J.encode_rgb8(J.synth_image(520, 300, seed=820), epf_iters=1),
             J.encode_lossless(J.synth_image(264, 40, seed=11)),
             J.encode_rgb8(J.synth_image(700, 600, seed=5), epf_iters=2, num_passes=2),
             J.encode_rgb8(J.synth_image(300, 260, seed=6), epf_iters=0, gab=0)]
    boxes = [(600, 300, 224, 224), (260, 10, 200, 200), (10, 5, 100, 30), None, (256, 0, 44, 256)]
    out = torch_io.decode_batch_to_tensor(datas, size=(32, 32), boxes=boxes, dtype=torch.float32)
    old = torch_io.decode_batch_to_tensor(datas, size=(32, 32), boxes=boxes, dtype=torch.float32, region=False)
    assert np.array_equal(_bits(out), _bits(old))
    for i, (d, b) in enumerate(zip(datas, boxes)):
        one = torch_io.decode_to_tensor(d, size=(32, 32), box=b, dtype=torch.float32)
        assert np.array_equal(_bits(out[i]), _bits(one)), i


# ------------------------------------------------------------------------------------------------ damage
def _section_ranges(J, f):
    """(begin, end) in the file of every AC group section, [pass * num_groups + group]: they are the frame's last sections."""
    L = J.lib()
    L.jxlamd_frame_section_sizes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    L.jxlamd_frame_section_sizes.restype = ctypes.c_size_t
    n = f.info["num_groups"] * f.info["num_passes"]
    sizes = (ctypes.c_uint32 * n)()
    assert L.jxlamd_frame_section_sizes(f._h, sizes, n) == n
    ends = f.end - (sum(sizes) - np.cumsum(list(sizes)))
    return [(int(e) - int(s), int(e)) for s, e in zip(sizes, ends)]


def _flip(data, begin, end, seed):
    rng = np.random.default_rng(seed)
    b = bytearray(data)
    for at in rng.integers(begin + (end - begin) // 4, end - (end - begin) // 4, 12):
        b[int(at)] ^= int(rng.integers(1, 256))
    return bytes(b)


def test_damage_outside_the_window_is_not_seen_and_inside_it_is_named(built):
    """Fixed, seeded damage, each stream run once. Bytes flipped in the section of group 0: the region decode of a box in
    group 5 succeeds and equals the undamaged one (the documented deviation: the whole decode raises). Bytes flipped in
    group 5's section: JxlAmdError names group 5 of the FRAME, though it is group 0 of the window."""
    J = built
    data = _cached("damage", lambda: J.encode_rgb8(J.synth_image(1000, 700, seed=41), epf_iters=1))
    f = J.Frame(data)
    ranges = _section_ranges(J, f)
    assert f.plan_window((300, 300, 100, 100))["groups"] == [5]
    f.close()
    kw = dict(size=(64, 48), box=(300, 300, 100, 100), dtype=torch.float32)
    good = torch_io.decode_to_tensor(data, **kw)
    outside = _flip(data, ranges[0][0], ranges[0][1], 1)
    assert outside != data
    assert np.array_equal(_bits(torch_io.decode_to_tensor(outside, **kw)), _bits(good))
    with pytest.raises(J.JxlAmdError, match=r"corrupt AC sections: \[\(0, "):
        torch_io.decode_to_tensor(outside, region=False, **kw)
    inside = _flip(data, ranges[5][0], ranges[5][1], 2)
    with pytest.raises(J.JxlAmdError, match=r"corrupt AC sections: \[\(5, "):
        torch_io.decode_to_tensor(inside, **kw)
    with pytest.raises(J.JxlAmdError, match=r"frame 1: corrupt AC sections: \[\(5, "):
        torch_io.decode_batch_to_tensor([data, inside], size=(64, 48), boxes=[kw["box"]] * 2, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("byte", ["0xA5", "0xFF"])
def test_guard_bands_stay_clean(built, monkeypatch, byte):
    """JXLHIP_GUARD=1 under both fills: no kernel of a window decode (k_dc_window among them) writes next to a buffer, and
    none reads what nothing wrote (the pixels are those of the unguarded run)."""
    J = built
    data = _e2e_stream(J)
    want = _cached("guard_ref", lambda: _bits(torch_io.decode_to_tensor(data, size=(64, 48), box=E2E_BOXES["near_left"], dtype=torch.float32)))
    monkeypatch.setenv("JXLHIP_GUARD", "1")
    monkeypatch.setenv("JXLHIP_GUARD_BYTE", byte)
    f = J.Frame(data)
    c = J.HipContext()
    try:
        for box in (E2E_BOXES["near_left"], E2E_BOXES["ragged_corner"]):
            w = f.plan_window(box)
            t = torch.zeros((3, 64, 48), dtype=torch.float32, device="cuda")
            torch_io.bind_resized(c, t, "CHW", w["box"])
            c.upload_window(f, w)
            c.run_all()
            assert c.errors()[0] == 0
            c.sync()
            assert c.check_guards() == 0
            if box == E2E_BOXES["near_left"]:
                assert np.array_equal(_bits(t), want)
    finally:
        c.close()
        f.close()
