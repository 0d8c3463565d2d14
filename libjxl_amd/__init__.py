"""libjxl_amd — MI355X-native JPEG XL VarDCT decode path (Python plumbing over the C ABI).

The product is the shared library ``libjxl_amd/_build/libjxl_amd.so`` (HIP kernels + ``extern "C"`` layer declared in
``include/jxl_amd_hip.h``, ``include/jxl_amd.h`` and ``include/jxl/decode.h``).  This module only binds it with
ctypes for tests and ``bench.py``; it contains no decode logic and there is no CPU fallback: if the library or a HIP
device is missing, calls raise.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libjxl_amd.so")
ENC_PATH = os.path.join(_HERE, "_build", "libjxlenc.so")

_lib = None
_enc = None


class JxlAmdError(RuntimeError):
    pass


def build(verbose=False):
    """Compiles the in-tree shared libraries (hipcc --offload-arch=gfx950)."""
    r = subprocess.run(["make", "-C", _HERE], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise JxlAmdError("building libjxl_amd failed")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JxlAmdError("%s is missing: run libjxl_amd.build() (hipcc) first; there is no fallback path" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        vp, cp, u32p = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)
        L.jxlhip_version.restype = cp
        L.jxlhip_device_count.restype = ctypes.c_int
        L.jxlhip_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.jxlhip_ctx_destroy.argtypes = [vp]
        for name in ("jxlhip_run_entropy", "jxlhip_run_transform", "jxlhip_run_filter_color", "jxlhip_run_all", "jxlhip_sync"):
            getattr(L, name).argtypes = [vp]
        for name in ("jxlhip_run_entropy_batch", "jxlhip_run_transform_batch", "jxlhip_run_filter_color_batch"):
            getattr(L, name).argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        L.jxlhip_download_rgb8.argtypes = [vp, vp, ctypes.c_size_t]
        L.jxlhip_set_option.argtypes = [vp, cp, ctypes.c_int]
        L.jxlhip_share_planes.argtypes = [vp, vp]
        L.jxlhip_download_rgb8_rows.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]
        L.jxlamd_frame_upload_band.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32]
        L.jxlhip_rgb8_device_ptr.argtypes = [vp]
        L.jxlhip_rgb8_device_ptr.restype = vp
        L.jxlhip_get_errors.argtypes = [vp, u32p, ctypes.c_size_t]
        L.jxlhip_download.argtypes = [vp, cp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        L.jxlhip_last_stage_ms.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        L.jxlamd_frame_parse.argtypes = [cp, ctypes.c_size_t, vp, vp, ctypes.POINTER(vp)]
        L.jxlamd_frame_free.argtypes = [vp]
        L.jxlamd_frame_info.argtypes = [vp, u32p]
        L.jxlamd_frame_out_size.argtypes = [vp, u32p]
        L.jxlamd_frame_upload.argtypes = [vp, vp]
        L.jxlamd_modframe_parse.argtypes = [cp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.jxlamd_modframe_free.argtypes = [vp]
        L.jxlamd_modframe_info.argtypes = [vp, u32p]
        L.jxlamd_modframe_upload.argtypes = [vp, vp]
        L.jxlamd_modframe_extra_buffer.argtypes = [vp, ctypes.c_uint32]
        L.jxlamd_modframe_extra_buffer.restype = ctypes.c_uint32
        L.jxlhip_modular_run.argtypes = [vp]
        L.jxlhip_modular_run_batch.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        L.jxlhip_modular_status.argtypes = [vp, u32p, u32p, ctypes.c_size_t]
        L.jxlhip_modular_download_buffer.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_size_t]
        L.jxlhip_set_output_format.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
        L.jxlhip_download_pixels.argtypes = [vp, vp, ctypes.c_size_t]
        L.jxlamd_last_error.restype = cp
        L.JxlThreadParallelRunnerCreate.restype = vp
        L.JxlThreadParallelRunnerCreate.argtypes = [vp, ctypes.c_size_t]
        L.JxlThreadParallelRunnerDestroy.argtypes = [vp]
        _lib = L
    return _lib


def _check(r, what):
    if r != 0:
        err = lib().jxlamd_last_error()
        raise JxlAmdError("%s failed: code %d %s" % (what, r, err.decode() if err else ""))


def _frame_splines(fn, handle):
    """What jxlamd_frame_splines / jxlamd_modframe_splines hand out, or None for a frame without splines."""
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    fn.restype = ctypes.c_size_t

    def part(what, dtype):
        a = np.zeros(int(fn(handle, what, None, 0)) // 4, dtype)
        if a.size:
            fn(handle, what, a.ctypes.data, a.nbytes)
        return a

    words = part(0, np.int32)
    if not words.size:
        return None
    w = [int(v) for v in words]
    splines, pos = [], 2
    for _ in range(w[1]):
        n = w[pos + 2]
        deltas = [(w[pos + 3 + 2 * k], w[pos + 4 + 2 * k]) for k in range(n)]
        q = pos + 3 + 2 * n
        splines.append(dict(start=(w[pos], w[pos + 1]), deltas=deltas, color=[w[q + 32 * c:q + 32 * c + 32] for c in range(3)],
                            sigma=w[q + 96:q + 128]))
        pos = q + 128
    assert pos == len(w)
    used = part(4, np.uint32)
    return dict(dictionary=dict(adjustment=w[0], splines=splines), words=words, segments=part(1, np.float32).reshape(-1, 8),
                row_start=part(2, np.uint32), row_segments=part(3, np.uint32), xsize=int(used[0]), ysize=int(used[1]),
                y_to_x=float(used[2:3].view(np.float32)[0]), y_to_b=float(used[3:4].view(np.float32)[0]))


class Frame:
    """Host-parsed frame (headers, DC, tables); AC sections stay compressed."""

    INFO = ("xsize", "ysize", "xsize_blocks", "ysize_blocks", "num_groups", "num_dc_groups", "num_passes", "used_acs",
            "epf_iters", "gab", "coef_bits", "ac_bytes", "log_alpha", "num_clusters", "ctx_map_size")

    def __init__(self, data, threads=0, frame_pos=0, frame_index=0, reduced=False):
        """frame_pos / frame_index: a later frame of an animation (frame_pos = the `end` of the frame before it).
        reduced=True: the parse of a reduced decode (jxlamd_frame_parse_reduced): headers, TOC and the DC sections alone, from
        the whole file or any prefix of at least frame_dc_extent(data) bytes; HipContext.upload_reduced takes the frame."""
        L = lib()
        self._data = bytes(data)  # must outlive upload
        self._h = ctypes.c_void_p()
        self.reduced = bool(reduced)
        if reduced and (frame_pos or frame_index):
            raise ValueError("a reduced parse takes the first frame")
        L.jxlamd_frame_parse_at.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.jxlamd_frame_parse_reduced.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.jxlamd_frame_end.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        L.jxlamd_frame_end.restype = ctypes.c_size_t
        runner = None
        pool = None
        if threads > 0:
            pool = L.JxlThreadParallelRunnerCreate(None, threads)
            runner = ctypes.cast(L.JxlThreadParallelRunner, ctypes.c_void_p)
        try:
            if reduced:
                _check(L.jxlamd_frame_parse_reduced(self._data, len(self._data), runner, pool, ctypes.byref(self._h)), "jxlamd_frame_parse_reduced")
            else:
                _check(L.jxlamd_frame_parse_at(self._data, len(self._data), frame_pos, frame_index, runner, pool, ctypes.byref(self._h)),
                       "jxlamd_frame_parse_at")
        finally:
            if pool:
                L.JxlThreadParallelRunnerDestroy(pool)
        info = (ctypes.c_uint32 * 16)()
        L.jxlamd_frame_info(self._h, info)
        self.info = dict(zip(self.INFO, list(info)))
        wh = (ctypes.c_uint32 * 2)()
        L.jxlamd_frame_out_size(self._h, wh)
        self.info["out_xsize"], self.info["out_ysize"] = int(wh[0]), int(wh[1])  # the image (upsampled frames: > frame size)
        t = (ctypes.c_uint32 * 3)()
        self.end = int(L.jxlamd_frame_end(self._h, t))  # byte offset behind the frame (it may lie beyond a prefix given to a reduced parse)
        self.duration, self.is_last, self.timecode = int(t[0]), bool(t[1]), int(t[2])

    def reduced_size(self):
        """(width, height) of the reduced image: the frame's size in 8x8 blocks."""
        L = lib()
        L.jxlamd_frame_reduced_size.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        wh = (ctypes.c_uint32 * 2)()
        L.jxlamd_frame_reduced_size(self._h, wh)
        return int(wh[0]), int(wh[1])

    def dc_quantised(self):
        """Test access: (the coded DC integers of X, Y, B as int32 [3, ysize_blocks, xsize_blocks], the precision shift of
        every DC group as uint8). A reduced frame or a whole one."""
        L = lib()
        L.jxlamd_frame_dc_quantised.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        w, h = self.reduced_size()
        q = np.empty((3, h, w), np.int32)
        ep = np.empty(self.info["num_dc_groups"], np.uint8)
        _check(L.jxlamd_frame_dc_quantised(self._h, q.ctypes.data, q.size, ep.ctypes.data, ep.size), "jxlamd_frame_dc_quantised")
        return q, ep

    def set_linear_output(self, linear=True):
        """The sRGB transfer function (False) or none (True) on the way out; before upload."""
        L = lib()
        L.jxlamd_frame_set_linear_output.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.jxlamd_frame_set_linear_output.restype = None
        L.jxlamd_frame_set_linear_output(self._h, 1 if linear else 0)

    def set_color_output(self, target=None, desired_intensity=0.0):
        """The colour stage the JxlDecoder gives an XYB image tagged with an enum encoding (PQ, HLG, P3, grey ...): rendered
        to `target` (a ctypes JxlColorEncoding; None: the image's own encoding) for desired_intensity (0: the image's)
        (jxlamd_frame_set_color_output); before upload."""
        L = lib()
        L.jxlamd_frame_set_color_output.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
        _check(L.jxlamd_frame_set_color_output(self._h, None if target is None else ctypes.byref(target), desired_intensity),
               "jxlamd_frame_set_color_output")

    def upsampling_kernels(self, factor):
        """The factor x factor 5x5 upsampling kernels the host builds from the image's coded or default weights."""
        L = lib()
        L.jxlamd_upsampling_kernels.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        k = np.zeros((factor, factor, 5, 5), np.float32)
        _check(L.jxlamd_upsampling_kernels(self._h, factor, k.ctypes.data), "jxlamd_upsampling_kernels")
        return k

    def splines(self):
        """Test access: the spline dictionary as parsed and the draw cache built from it (None: no splines)."""
        return _frame_splines(lib().jxlamd_frame_splines, self._h)

    def plan_window(self, box, channels=3, orientation=1):
        """The window of a region decode (jxlamd_frame_plan_window; no device): the rectangle of whole 256 x 256 groups that
        box = (x0, y0, xsize, ysize) of the oriented output image needs (None: the whole image), for an output of `channels`
        channels on a context that undoes `orientation` (set_output_orientation). A dict: x0 / y0 / xsize / ysize (frame
        pixels), gx0 / gy0 / gxs / gys (groups), box (the caller's box in the window image: bind this one), groups (the
        frame's group number of every window group), groups_taken, groups_in_frame, reason (0: a true window; else
        WINDOW_REASONS[reason] says why the window is the whole frame) and orientation. HipContext.upload_window takes it."""
        L = lib()
        L.jxlamd_frame_plan_window.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(Window)]
        L.jxlamd_sizeof_window.restype = ctypes.c_size_t
        assert L.jxlamd_sizeof_window() == ctypes.sizeof(Window)
        w = Window()
        w.orientation = int(orientation)
        b = (ctypes.c_uint32 * 4)(*([0, 0, 0, 0] if box is None else [int(v) for v in box]))
        _check(L.jxlamd_frame_plan_window(self._h, b, int(channels), ctypes.byref(w)), "jxlamd_frame_plan_window")
        out = {name: int(getattr(w, name)) for name, _ in Window._fields_ if name != "box"}
        out["box"] = tuple(int(v) for v in w.box)
        per_row = (self.info["xsize"] + 255) // 256
        out["groups"] = [(w.gy0 + i // w.gxs) * per_row + w.gx0 + i % w.gxs for i in range(w.gxs * w.gys)]
        return out

    def close(self):
        if self._h:
            lib().jxlamd_frame_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModFrame:
    """Host-parsed Modular (lossless) frame: headers, trees, histograms, stream descriptors; samples stay compressed."""

    # launch_levels: levels of inverse-transform launches (the deepest chain of group-local operations + the frame's own
    # transforms; one launch per level and kind whatever the number of groups); num_local_ops / local_levels: the group part
    INFO = ("xsize", "ysize", "num_color", "has_alpha", "bits", "num_streams", "num_buffers", "num_ops", "num_extra", "section_bytes",
            "max_table_words", "lz77", "max_tree_nodes", "launch_levels", "num_local_ops", "local_levels")

    def __init__(self, data, frame_pos=0, frame_index=0):
        L = lib()
        self._data = bytes(data)  # must outlive upload
        self._h = ctypes.c_void_p()
        L.jxlamd_modframe_parse_at.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_void_p)]
        L.jxlamd_modframe_end.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        L.jxlamd_modframe_end.restype = ctypes.c_size_t
        _check(L.jxlamd_modframe_parse_at(self._data, len(self._data), frame_pos, frame_index, ctypes.byref(self._h)),
               "jxlamd_modframe_parse_at")
        info = (ctypes.c_uint32 * 16)()
        L.jxlamd_modframe_info(self._h, info)
        self.info = dict(zip(self.INFO, list(info)))
        t = (ctypes.c_uint32 * 3)()
        self.end = int(L.jxlamd_modframe_end(self._h, t))
        self.duration, self.is_last, self.timecode = int(t[0]), bool(t[1]), int(t[2])

    def section(self, index):
        """(offset, size) of TOC section `index` in the data: 0 = DC global, then the DC groups, then the AC groups."""
        L = lib()
        L.jxlamd_modframe_section.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        off, size = ctypes.c_uint64(), ctypes.c_uint32()
        if L.jxlamd_modframe_section(self._h, index, ctypes.byref(off), ctypes.byref(size)):
            raise IndexError("no section %d" % index)
        return int(off.value), int(size.value)

    def splines(self):
        """Test access: as Frame.splines()."""
        return _frame_splines(lib().jxlamd_modframe_splines, self._h)

    def close(self):
        if self._h:
            lib().jxlamd_modframe_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TENSOR_F32, TENSOR_U8, TENSOR_F16, TENSOR_BF16 = 0, 2, 5, 6  # JXLHIP_TENSOR_*


class TensorOut(ctypes.Structure):  # JxlHipTensorOut
    _fields_ = [("data", ctypes.c_void_p), ("bytes", ctypes.c_size_t), ("dtype", ctypes.c_uint32), ("num_channels", ctypes.c_uint32),
                ("stride_c", ctypes.c_int64), ("stride_y", ctypes.c_int64), ("stride_x", ctypes.c_int64),
                ("scale", ctypes.c_float * 4), ("bias", ctypes.c_float * 4), ("clamp01", ctypes.c_uint32),
                ("consumer_stream", ctypes.c_void_p)]


RESAMPLE_TRIANGLE = 0  # JXLHIP_RESAMPLE_*


class ResizedOut(ctypes.Structure):  # JxlHipResizedOut
    _fields_ = [("tensor", TensorOut), ("out_xsize", ctypes.c_uint32), ("out_ysize", ctypes.c_uint32),
                ("box_x0", ctypes.c_uint32), ("box_y0", ctypes.c_uint32), ("box_xsize", ctypes.c_uint32), ("box_ysize", ctypes.c_uint32),
                ("filter", ctypes.c_uint32)]


def _tensor_out(ptr, nbytes, dtype, num_channels, strides, scale, bias, clamp, stream):
    t = TensorOut()
    t.data, t.bytes, t.dtype, t.num_channels = int(ptr), int(nbytes), int(dtype), int(num_channels)
    t.stride_c, t.stride_y, t.stride_x = [int(s) for s in strides]
    for c in range(4):
        t.scale[c] = 1.0 if scale is None or c >= len(scale) else float(scale[c])
        t.bias[c] = 0.0 if bias is None or c >= len(bias) else float(bias[c])
    t.clamp01 = 1 if clamp else 0
    t.consumer_stream = int(stream) or None
    return t


def _resized_out(ptr, nbytes, dtype, num_channels, strides, out_size, box, scale, bias, clamp, stream, filter):
    d = ResizedOut()
    d.tensor = _tensor_out(ptr, nbytes, dtype, num_channels, strides, scale, bias, clamp, stream)
    d.out_xsize, d.out_ysize = int(out_size[0]), int(out_size[1])
    d.box_x0, d.box_y0, d.box_xsize, d.box_ysize = [int(v) for v in (box if box is not None else (0, 0, 0, 0))]
    d.filter = int(filter)
    return d


def frame_dc_extent(data):
    """The number of leading bytes of `data` (the file or a prefix of it) that a reduced parse, Frame(data, reduced=True),
    reads: up to the end of the DC sections. Raises JxlAmdError "truncated frame header" when `data` is too short to tell."""
    L = lib()
    L.jxlamd_frame_dc_extent.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    need = ctypes.c_size_t()
    data = bytes(data)
    _check(L.jxlamd_frame_dc_extent(data, len(data), ctypes.byref(need)), "jxlamd_frame_dc_extent")
    return int(need.value)


class Window(ctypes.Structure):  # JxlAmdWindow
    _fields_ = [("orientation", ctypes.c_uint32), ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("xsize", ctypes.c_uint32),
                ("ysize", ctypes.c_uint32), ("gx0", ctypes.c_uint32), ("gy0", ctypes.c_uint32), ("gxs", ctypes.c_uint32),
                ("gys", ctypes.c_uint32), ("box", ctypes.c_uint32 * 4), ("groups_taken", ctypes.c_uint32),
                ("groups_in_frame", ctypes.c_uint32), ("reason", ctypes.c_uint32)]


# enum WholeFrameReason of csrc/host/jxh_window_plan.h: why a frame's window is the whole frame (0: a true window)
WINDOW_REASONS = ("windowed", "partial", "upsampling", "subsampling", "noise", "patches", "splines", "dc_frame", "alpha",
                  "single_section", "one_group", "window_is_frame")


class DcWindow(ctypes.Structure):  # JxlHipDcWindow
    _fields_ = [("frame_xsize_blocks", ctypes.c_uint32), ("frame_ysize_blocks", ctypes.c_uint32),
                ("win_x0", ctypes.c_uint32), ("win_y0", ctypes.c_uint32), ("win_xsize", ctypes.c_uint32), ("win_ysize", ctypes.c_uint32),
                ("apron_x0", ctypes.c_uint32), ("apron_y0", ctypes.c_uint32), ("apron_xsize", ctypes.c_uint32), ("apron_ysize", ctypes.c_uint32),
                ("apron", ctypes.c_void_p), ("dc_extra_precision", ctypes.c_void_p), ("num_dc_groups", ctypes.c_uint32),
                ("dc_step", ctypes.c_float * 3), ("dc_cfl_x", ctypes.c_float), ("dc_cfl_b", ctypes.c_float), ("dc_smoothing", ctypes.c_uint32)]


def dc_apron(window, frame_size):
    """(x0, y0, xsize, ysize) in blocks: the window grown by one block on every side and clipped to the frame (PlanDcApron of
    csrc/host/jxh_window_plan.h)."""
    x0, y0, xs, ys = window
    fx, fy = frame_size
    ax0, ay0 = max(x0 - 1, 0), max(y0 - 1, 0)
    return ax0, ay0, min(x0 + xs + 1, fx) - ax0, min(y0 + ys + 1, fy) - ay0


def frame_is_modular(data):
    """Whether the codestream's first frame is Modular-coded (ModFrame, upload_modular) or VarDCT (Frame, upload)."""
    L = lib()
    L.jxlamd_frame_is_modular.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    m = ctypes.c_uint32()
    data = bytes(data)
    _check(L.jxlamd_frame_is_modular(data, len(data), ctypes.byref(m)), "jxlamd_frame_is_modular")
    return bool(m.value)


class HipContext:
    """One HIP stream + the device buffers of one frame (include/jxl_amd_hip.h)."""

    def __init__(self, device=0):
        L = lib()
        if L.jxlhip_device_count() <= 0:
            raise JxlAmdError("no HIP device visible: the decode path has no CPU implementation")
        self._h = ctypes.c_void_p()
        _check(L.jxlhip_ctx_create(device, ctypes.byref(self._h)), "jxlhip_ctx_create")
        self.frame_info = None

    def close(self):
        if self._h:
            lib().jxlhip_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_color(self, xyb, linear=False):
        """Test entry: the colour stage alone on XYB triples (array [3, n]) -> float RGB [n, 3]."""
        xyb = np.ascontiguousarray(xyb, np.float32)
        n = xyb.shape[1]
        out = np.empty((n, 3), np.float32)
        L = lib()
        L.jxlhip_debug_color.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        _check(L.jxlhip_debug_color(self._h, xyb.ctypes.data, n, 1 if linear else 0, out.ctypes.data), "jxlhip_debug_color")
        return out

    def debug_noise(self, xyb, seed0, seed1, lut, ytox, ytob, band=None, want_raw=True):
        """Test entry: the noise kernels alone on planes xyb [3, ys, xs] -> (planes with the noise, raw random planes or None);
        band = (y_begin, y_end): only those rows get noise."""
        xyb = np.ascontiguousarray(xyb, np.float32)
        _, ys, xs = xyb.shape
        y0, y1 = band if band is not None else (0, ys)
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.shape == (8,)
        out = np.empty_like(xyb)
        raw = np.empty_like(xyb) if want_raw else None
        L = lib()
        L.jxlhip_debug_noise.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.jxlhip_debug_noise(self._h, xyb.ctypes.data, xs, ys, seed0, seed1, lut.ctypes.data, ytox, ytob, y0, y1,
                                    raw.ctypes.data if want_raw else None, out.ctypes.data), "jxlhip_debug_noise")
        return out, raw

    def upsample_plane(self, plane, factor, kernels, out_xs, out_ys, as_alpha=False):
        """jxlhip_upsample_plane on plane [ys, xs] with kernels [factor, factor, 5, 5]: the result [out_ys, out_xs], or (as_alpha)
        None, the result being the context's alpha plane (download_alpha)."""
        plane = np.ascontiguousarray(plane, np.float32)
        kernels = np.ascontiguousarray(kernels, np.float32)
        assert kernels.size == factor * factor * 25
        out = None if as_alpha else np.empty((out_ys, out_xs), np.float32)
        L = lib()
        L.jxlhip_upsample_plane.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        _check(L.jxlhip_upsample_plane(self._h, plane.ctypes.data, plane.shape[1], plane.shape[0], factor, kernels.ctypes.data, out_xs, out_ys,
                                       1 if as_alpha else 0, None if as_alpha else out.ctypes.data), "jxlhip_upsample_plane")
        return out

    def download_alpha(self, out_xs, out_ys):
        L = lib()
        L.jxlhip_download_alpha.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        out = np.empty((out_ys, out_xs), np.float32)
        _check(L.jxlhip_download_alpha(self._h, out.ctypes.data), "jxlhip_download_alpha")
        return out

    def pixel_route(self):
        """Test access: 0 = the generic writer makes the pixels of the uploaded frame, 1 = the filter kernel, 2 = the filter
        kernel's one-channel 8-bit form."""
        L = lib()
        L.jxlhip_debug_pixel_route.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        r = ctypes.c_uint32()
        _check(L.jxlhip_debug_pixel_route(self._h, ctypes.byref(r)), "jxlhip_debug_pixel_route")
        return int(r.value)

    def check_guards(self):
        """JXLHIP_GUARD=1 debug aid: 0 when no kernel wrote next to one of this context's device buffers."""
        t = ctypes.c_uint32()
        _check(lib().jxlhip_check_guards(self._h, ctypes.byref(t)), "jxlhip_check_guards")
        return int(t.value)

    def set_option(self, name, value):
        _check(lib().jxlhip_set_option(self._h, name.encode(), int(value)), "jxlhip_set_option")

    def share_planes(self, lender):
        """Keep this context's XYB planes in `lender`'s buffer (None: its own again); call before upload()."""
        _check(lib().jxlhip_share_planes(self._h, lender._h if lender is not None else None), "jxlhip_share_planes")
        self._lender = lender  # keeps the lender alive

    def upload(self, frame, band=None):
        """band = (group_row_begin, group_row_end): produce only those rows of 256x256 groups (multi-GPU split)."""
        b0, b1 = band if band else (0, 0)
        _check(lib().jxlamd_frame_upload_band(frame._h, self._h, b0, b1), "jxlamd_frame_upload_band")
        self.frame_info = dict(frame.info)

    def upload_window(self, frame, window):
        """Region decode (jxlamd_frame_upload_window): uploads the window frame.plan_window made as a frame of its own. The
        context then is a frame of the window's size: frame_info has its sizes and group count, errors() is indexed by window
        group (window["groups"] maps back). A window with a reason set is upload(frame)."""
        L = lib()
        L.jxlamd_frame_upload_window.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Window)]
        w = Window()
        for name, _ in Window._fields_:
            if name != "box":
                setattr(w, name, int(window[name]))
        w.box = (ctypes.c_uint32 * 4)(*window["box"])
        _check(L.jxlamd_frame_upload_window(frame._h, self._h, ctypes.byref(w)), "jxlamd_frame_upload_window")
        self.frame_info = dict(frame.info)
        if not window["reason"]:
            fi = self.frame_info
            fi["xsize"], fi["ysize"] = window["xsize"], window["ysize"]
            fi["out_xsize"], fi["out_ysize"] = window["xsize"], window["ysize"]
            fi["xsize_blocks"], fi["ysize_blocks"] = (window["xsize"] + 7) // 8, (window["ysize"] + 7) // 8
            fi["num_groups"] = window["groups_taken"]

    def debug_dc_window(self, q, window, extra_precision, step, cfl_x, cfl_b, smoothing=True, apron=None):
        """Test entry (jxlhip_debug_dc_window): k_dc_window alone on the coded integer planes q [3, ys, xs] of a frame with
        the DC groups' precision shifts `extra_precision` (None: all 0), for window = (x0, y0, xsize, ysize) in blocks ->
        float32 [3, ysize, xsize]. apron: the rectangle handed over instead of the planned one (for the refusals)."""
        q = np.ascontiguousarray(q, np.int32)
        _, fys, fxs = q.shape
        x0, y0, xs, ys = window
        ax0, ay0, axs, ays = apron if apron is not None else dc_apron(window, (fxs, fys))
        cut = np.ascontiguousarray(q[:, ay0:ay0 + ays, ax0:ax0 + axs])
        ep = None if extra_precision is None else np.ascontiguousarray(extra_precision, np.uint8)
        d = DcWindow(fxs, fys, x0, y0, xs, ys, ax0, ay0, axs, ays, cut.ctypes.data, None if ep is None else ep.ctypes.data,
                     0 if ep is None else ep.size, (ctypes.c_float * 3)(*step), cfl_x, cfl_b, 1 if smoothing else 0)
        out = np.empty((3, ys, xs), np.float32)
        L = lib()
        L.jxlhip_debug_dc_window.argtypes = [ctypes.c_void_p, ctypes.POINTER(DcWindow), ctypes.c_void_p]
        _check(L.jxlhip_debug_dc_window(self._h, ctypes.byref(d), out.ctypes.data), "jxlhip_debug_dc_window")
        return out

    def upload_reduced(self, frame):
        """The frame's DC image as a reduced (1/8-scale) image: a Frame(data, reduced=True) or a whole Frame. Then
        run_reduced(); pixels() / rgb8() hand out the reduced image, or the bound tensor holds it."""
        L = lib()
        L.jxlamd_frame_upload_reduced.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _check(L.jxlamd_frame_upload_reduced(frame._h, self._h), "jxlamd_frame_upload_reduced")
        w, h = frame.reduced_size()
        self.frame_info = dict(frame.info)
        self.frame_info["out_xsize"], self.frame_info["out_ysize"] = w, h

    def run_reduced(self):
        L = lib()
        L.jxlhip_reduced_run.argtypes = [ctypes.c_void_p]
        _check(L.jxlhip_reduced_run(self._h), "jxlhip_reduced_run")

    def halo_rows(self):
        """Rows of the neighbouring bands the filters of this band read (after an upload)."""
        L = lib()
        L.jxlhip_halo_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        n = ctypes.c_uint32()
        _check(L.jxlhip_halo_rows(self._h, ctypes.byref(n)), "jxlhip_halo_rows")
        return int(n.value)

    def halo_floats(self):
        """Floats of one halo block ([3][rows][padded xsize])."""
        xp = ((self.frame_info["xsize"] + 7) // 8) * 8
        return 3 * self.halo_rows() * xp

    def halo_pack(self, side, device_ptr, nbytes):
        """side 0: this band's first rows (for the band above), 1: its last rows (for the band below) -> device memory."""
        L = lib()
        L.jxlhip_halo_pack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        _check(L.jxlhip_halo_pack(self._h, side, device_ptr, nbytes), "jxlhip_halo_pack")

    def halo_unpack(self, side, device_ptr, nbytes):
        """side 0: the rows just above this band, 1: just below it <- device memory (what the neighbour packed)."""
        L = lib()
        L.jxlhip_halo_unpack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        _check(L.jxlhip_halo_unpack(self._h, side, device_ptr, nbytes), "jxlhip_halo_unpack")

    def set_output_format(self, data_type=2, num_channels=3, bits=0, big_endian=False):
        """JxlDataType numbering: 0 f32, 2 u8, 3 u16, 5 f16; call before upload."""
        _check(lib().jxlhip_set_output_format(self._h, data_type, num_channels, bits, 1 if big_endian else 0), "jxlhip_set_output_format")
        self._out = (data_type, num_channels)

    def set_output_tensor(self, ptr, nbytes=0, dtype=TENSOR_F16, num_channels=3, strides=None, scale=None, bias=None, clamp=False, stream=0):
        """jxlhip_set_output_tensor: the pixels of the next uploads go to caller-owned device memory at `ptr` (`nbytes` of
        room) instead of the context's own buffer; ptr=None unbinds. dtype: TENSOR_U8 / _F16 / _BF16 / _F32; strides =
        (stride_c, stride_y, stride_x) in elements of the output image; float types store v * scale[c] + bias[c] (after a
        clamp to 0..1 if asked), each step rounded; stream: the consumer's hipStream_t as an integer (0 = the null stream),
        ordered before and behind the writes without a host wait. Call before upload. libjxl_amd.torch_io binds a tensor."""
        L = lib()
        L.jxlhip_set_output_tensor.argtypes = [ctypes.c_void_p, ctypes.POINTER(TensorOut)]
        if ptr is None:
            _check(L.jxlhip_set_output_tensor(self._h, None), "jxlhip_set_output_tensor")
            self._tensor = None
            return
        t = _tensor_out(ptr, nbytes, dtype, num_channels, strides, scale, bias, clamp, stream)
        _check(L.jxlhip_set_output_tensor(self._h, ctypes.byref(t)), "jxlhip_set_output_tensor")
        self._tensor = t

    def set_output_resized(self, ptr, nbytes=0, dtype=TENSOR_F16, num_channels=3, strides=None, out_size=None, box=None, scale=None,
                           bias=None, clamp=False, stream=0, filter=RESAMPLE_TRIANGLE):
        """jxlhip_set_output_resized: a box of the next uploads' oriented output image, box = (x0, y0, xsize, ysize) or None
        for the whole image, is resampled (antialiased triangle filter) to out_size = (out_xsize, out_ysize) and goes to the
        caller-owned device memory at `ptr`, described as for set_output_tensor at the OUTPUT size; ptr=None unbinds.
        uint8 takes the undithered 8-bit sample. Replaces a bound tensor. libjxl_amd.torch_io.bind_resized binds a tensor."""
        L = lib()
        L.jxlhip_set_output_resized.argtypes = [ctypes.c_void_p, ctypes.POINTER(ResizedOut)]
        if ptr is None:
            _check(L.jxlhip_set_output_resized(self._h, None), "jxlhip_set_output_resized")
            self._resized = None
            return
        d = _resized_out(ptr, nbytes, dtype, num_channels, strides, out_size, box, scale, bias, clamp, stream, filter)
        _check(L.jxlhip_set_output_resized(self._h, ctypes.byref(d)), "jxlhip_set_output_resized")
        self._resized = d

    def debug_resample(self, src, ptr, nbytes, dtype, strides, out_size, box=None, scale=None, bias=None, clamp=False, stream=0,
                       filter=RESAMPLE_TRIANGLE, num_channels=None):
        """Test entry: the two resample passes alone on src [ysize, xsize, nc] (host floats) into the device memory at `ptr`,
        described as for set_output_resized (num_channels: the tensor's, nc unless given); complete on return."""
        src = np.ascontiguousarray(src, np.float32)
        ys, xs, nc = src.shape
        d = _resized_out(ptr, nbytes, dtype, nc if num_channels is None else num_channels, strides, out_size, box, scale, bias, clamp, stream, filter)
        L = lib()
        L.jxlhip_debug_resample.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.POINTER(ResizedOut)]
        _check(L.jxlhip_debug_resample(self._h, src.ctypes.data, xs, ys, nc, ctypes.byref(d)), "jxlhip_debug_resample")

    def set_output_orientation(self, orientation=1):
        """Undo this image orientation (1..8, EXIF numbering) in the pixel writer; call before upload."""
        L = lib()
        L.jxlhip_set_output_orientation.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _check(L.jxlhip_set_output_orientation(self._h, int(orientation)), "jxlhip_set_output_orientation")
        self._transposed = orientation > 4

    def enc_rerun(self, times=1):
        """Measurement: the forward-path kernels of the last encode_rgb8_gpu on this context, `times` more times on the
        resident input. Returns (ms of all passes, ms of the transform kernel of the last pass)."""
        L = lib()
        L.jxlhip_enc_forward_rerun.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.jxlhip_enc_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        L.jxlhip_enc_last_transform_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        _check(L.jxlhip_enc_forward_rerun(self._h, times), "jxlhip_enc_forward_rerun")
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(L.jxlhip_enc_last_ms(self._h, ctypes.byref(a)), "jxlhip_enc_last_ms")
        _check(L.jxlhip_enc_last_transform_ms(self._h, ctypes.byref(b)), "jxlhip_enc_last_transform_ms")
        return a.value, b.value

    def enc_aq_ms(self):
        """Measurement: ms of the two adaptive-quant kernels in the last forward pass made with adaptive_quant=1."""
        L = lib()
        L.jxlhip_enc_aq_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        a = ctypes.c_float()
        _check(L.jxlhip_enc_aq_last_ms(self._h, ctypes.byref(a)), "jxlhip_enc_aq_last_ms")
        return a.value

    def enc_masking_ms(self):
        """Measurement: ms of the kernel of the last masking_1x1 on this context."""
        L = lib()
        L.jxlhip_enc_masking_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        a = ctypes.c_float()
        _check(L.jxlhip_enc_masking_last_ms(self._h, ctypes.byref(a)), "jxlhip_enc_masking_last_ms")
        return a.value

    def enc_search_ms(self):
        """Measurement: ms of (mask1x1, all estimate launches, the walk) in the last forward pass made with acs_search 1 or 2."""
        L = lib()
        L.jxlhip_enc_search_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        a = (ctypes.c_float * 3)()
        _check(L.jxlhip_enc_search_last_ms(self._h, a), "jxlhip_enc_search_last_ms")
        return tuple(a)

    def enc_estimate_ms(self):
        """Measurement: ms of the kernels of the last estimate_entropy on this context."""
        L = lib()
        L.jxlhip_enc_estimate_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        a = ctypes.c_float()
        _check(L.jxlhip_enc_estimate_last_ms(self._h, ctypes.byref(a)), "jxlhip_enc_estimate_last_ms")
        return a.value

    def debug_ans_write(self, tokens, tables, capacity=None):
        """Test access: rANS-codes `tokens` ((n, 2) uint32 {context, value} pairs) as one section with the device's entropy
        kernels and the code `tables` (an AnsTables). Returns (the bit string as bytes, its length in bits); `capacity`
        bytes of room for it (default: enough)."""
        L = lib()
        L.jxlhip_debug_ans_write.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(EncAnsDesc), ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        tokens = np.ascontiguousarray(tokens, np.uint32).reshape(-1, 2)
        cap = 16 + 8 * len(tokens) if capacity is None else int(capacity)
        out = np.zeros(max(1, cap), np.uint8)
        bits = ctypes.c_uint64()
        d = tables.desc()
        _check(L.jxlhip_debug_ans_write(self._h, tokens.ctypes.data, len(tokens), ctypes.byref(d), out.ctypes.data, cap, ctypes.byref(bits)),
               "jxlhip_debug_ans_write")
        return out[:(bits.value + 7) // 8].tobytes(), int(bits.value)

    def enc_histograms(self, num_ctx, cfg=(4, 2, 0)):
        """Symbol counts of the resident tokens (the last device tokenisation, or debug_ans_write's): ((num_ctx, 256) uint32,
        the largest symbol)."""
        L = lib()
        L.jxlhip_enc_histograms.argtypes = [ctypes.c_void_p, ctypes.POINTER(EncHistDesc), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        counts = np.zeros((num_ctx, 256), np.uint32)
        mx = ctypes.c_uint32()
        d = EncHistDesc(cfg[0], cfg[1], cfg[2], num_ctx)
        _check(L.jxlhip_enc_histograms(self._h, ctypes.byref(d), counts.ctypes.data, ctypes.byref(mx)), "jxlhip_enc_histograms")
        return counts, int(mx.value)

    def enc_entropy_ms(self):
        """Kernel milliseconds of the last histogram pass and of the last rANS sizes + write passes on this context."""
        L = lib()
        L.jxlhip_enc_entropy_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        ms = (ctypes.c_float * 2)()
        _check(L.jxlhip_enc_entropy_last_ms(self._h, ms), "jxlhip_enc_entropy_last_ms")
        return float(ms[0]), float(ms[1])

    def upload_modular(self, mframe):
        _check(lib().jxlamd_modframe_upload(mframe._h, self._h), "jxlamd_modframe_upload")
        self.frame_info = dict(mframe.info)
        self.frame_info["out_xsize"], self.frame_info["out_ysize"] = mframe.info["xsize"], mframe.info["ysize"]

    def upload_modular_desc(self, desc, num_streams, xsize, ysize):
        """jxlhip_modular_upload of a hand-made descriptor: `desc` is a ctypes structure laid out as JxlHipModFrameDesc
        (include/jxl_amd_hip.h) whose arrays the caller keeps alive for the call."""
        L = lib()
        L.jxlhip_modular_upload.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _check(L.jxlhip_modular_upload(self._h, ctypes.byref(desc)), "jxlhip_modular_upload")
        self.frame_info = dict(num_streams=int(num_streams), xsize=int(xsize), ysize=int(ysize), out_xsize=int(xsize), out_ysize=int(ysize))

    def run_modular(self):
        _check(lib().jxlhip_modular_run(self._h), "jxlhip_modular_run")

    def modular_status(self):
        n = self.frame_info["num_streams"]
        st = (ctypes.c_uint32 * max(n, 1))()
        eb = (ctypes.c_uint32 * max(n, 1))()
        r = lib().jxlhip_modular_status(self._h, st, eb, n)
        return r, list(st)[:n], list(eb)[:n]

    def modular_buffer(self, index, shape=None):
        """Channel buffer `index` after the run; shape = (h, w) of a buffer that does not have the frame's size."""
        h, w = shape if shape is not None else (self.frame_info["ysize"], self.frame_info["xsize"])
        need = w * h
        out = np.empty(max(need, 1), np.int32)
        _check(lib().jxlhip_modular_download_buffer(self._h, index, out.ctypes.data, need), "jxlhip_modular_download_buffer")
        return out[:need].reshape(h, w)

    def pixels(self):
        """The interleaved result in the format of set_output_format (default RGB8)."""
        fi = self.frame_info
        dt, nc = getattr(self, "_out", (2, 3))
        np_dt = {0: np.float32, 2: np.uint8, 3: np.uint16, 5: np.float16}[dt]
        oxs, oys = fi["out_xsize"], fi["out_ysize"]
        if getattr(self, "_transposed", False):
            oxs, oys = oys, oxs
        out = np.empty((oys, oxs, nc), np_dt)
        _check(lib().jxlhip_download_pixels(self._h, out.ctypes.data, oxs * nc * out.itemsize), "jxlhip_download_pixels")
        return out

    def rgb8_rows(self, y0, y1):
        fi = self.frame_info
        out = np.empty((y1 - y0, fi["out_xsize"], 3), np.uint8)
        _check(lib().jxlhip_download_rgb8_rows(self._h, out.ctypes.data, fi["out_xsize"] * 3, y0, y1), "jxlhip_download_rgb8_rows")
        return out

    def run_entropy(self):
        _check(lib().jxlhip_run_entropy(self._h), "jxlhip_run_entropy")

    def run_transform(self):
        _check(lib().jxlhip_run_transform(self._h), "jxlhip_run_transform")

    def run_filter_color(self):
        _check(lib().jxlhip_run_filter_color(self._h), "jxlhip_run_filter_color")

    def run_all(self):
        _check(lib().jxlhip_run_all(self._h), "jxlhip_run_all")

    def sync(self):
        _check(lib().jxlhip_sync(self._h), "jxlhip_sync")

    def errors(self):
        n = self.frame_info["num_groups"]
        flags = (ctypes.c_uint32 * n)()
        r = lib().jxlhip_get_errors(self._h, flags, n)
        return r, list(flags)

    def entropy_route(self):
        """Test access: the kernel run_entropy launches for the uploaded frame: 0 k_entropy_lanes, 1 k_entropy_uni,
        2 k_entropy_ans, 3 k_entropy_generic."""
        L = lib()
        L.jxlhip_debug_entropy_route.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        r = ctypes.c_uint32()
        _check(L.jxlhip_debug_entropy_route(self._h, ctypes.byref(r)), "jxlhip_debug_entropy_route")
        return int(r.value)

    def entropy_order(self, room=65536):
        """Test access (jxlhip_debug_entropy_order): of the lane-kernel batch last prepared with this context first, the unit
        of every workgroup in dispatch order and the estimated length of that unit."""
        L = lib()
        L.jxlhip_debug_entropy_order.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        unit, est = np.zeros(room, np.uint32), np.zeros(room, np.uint64)
        _check(L.jxlhip_debug_entropy_order(self._h, unit.ctypes.data, est.ctypes.data, room), "jxlhip_debug_entropy_order")
        n = int((unit != 0xFFFFFFFF).sum())
        return unit[:n].copy(), est[:n].copy()

    def entropy_timeline(self, back=0):
        """Measurement aid (jxlhip_debug_entropy_timeline, JXLHIP_LANES_PROF=2): the (workgroups, 8) uint64 records of the
        lane-kernel launch `back` launches ago on this context."""
        L = lib()
        L.jxlhip_debug_entropy_timeline.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                                    ctypes.POINTER(ctypes.c_size_t)]
        n = ctypes.c_size_t()
        _check(L.jxlhip_debug_entropy_timeline(self._h, back, None, 0, ctypes.byref(n)), "jxlhip_debug_entropy_timeline")
        rec = np.zeros((n.value, 8), np.uint64)
        _check(L.jxlhip_debug_entropy_timeline(self._h, back, rec.ctypes.data, n.value, ctypes.byref(n)), "jxlhip_debug_entropy_timeline")
        return rec

    def section_end_bits(self):
        """jxlhip_get_section_end_bits: [pass][group], the bit (from the section's first byte) where the entropy stage's
        coefficient walk ended."""
        L = lib()
        L.jxlhip_get_section_end_bits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        n = self.frame_info["num_groups"]
        bits = np.zeros(n * self.frame_info.get("num_passes", 1), np.uint32)
        _check(L.jxlhip_get_section_end_bits(self._h, bits.ctypes.data, bits.size), "jxlhip_get_section_end_bits")
        return bits.reshape(-1, n)

    def stage_ms(self, which):
        ms = ctypes.c_float()
        _check(lib().jxlhip_last_stage_ms(self._h, which, ctypes.byref(ms)), "jxlhip_last_stage_ms")
        return ms.value

    def rgb8(self):
        fi = self.frame_info
        out = np.empty((fi["out_ysize"], fi["out_xsize"], 3), np.uint8)
        _check(lib().jxlhip_download_rgb8(self._h, out.ctypes.data, fi["out_xsize"] * 3), "jxlhip_download_rgb8")
        return out

    def download(self, name):
        fi = self.frame_info
        need = ctypes.c_size_t()
        _check(lib().jxlhip_download(self._h, name.encode(), None, 0, ctypes.byref(need)), "jxlhip_download")
        buf = np.empty(need.value, np.uint8)
        _check(lib().jxlhip_download(self._h, name.encode(), buf.ctypes.data, need.value, None), "jxlhip_download")
        if name == "coeffs":
            dt = np.int16 if fi["coef_bits"] == 16 else np.int32
            return buf.view(dt).reshape(fi["num_groups"], 3, 65536)
        if name == "kend":  # [varblock][channel]
            return buf.view(np.uint32).reshape(-1, 3)
        if name == "transform_lists":  # [entry] = (strategy, varblock), launch order
            return buf.view(np.uint32).reshape(-1, 2)
        if name == "xyb_upsampled":  # the image's size, rows padded to 8
            return buf.view(np.float32).reshape(3, fi["out_ysize"], (fi["out_xsize"] + 7) // 8 * 8)
        if name in ("dc", "inv_sigma"):  # block-resolution planes as the transform / filter stages read them
            return buf.view(np.float32)
        return buf.view(np.float32).reshape(3, fi["ysize_blocks"] * 8, fi["xsize_blocks"] * 8)


def run_entropy_batch(ctxs):
    """Entropy stage of several resident frames as one kernel launch (jxlhip_run_entropy_batch)."""
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(lib().jxlhip_run_entropy_batch(arr, len(ctxs)), "jxlhip_run_entropy_batch")


def halo_pack_batch(ctxs, side, device_ptr, block_bytes, transport_stream=0):
    """jxlhip_halo_pack_batch: block i (frame i of the set) at device_ptr + i * block_bytes; whatever is enqueued on
    `transport_stream` (a hipStream_t as an integer; 0 = the null stream) afterwards follows the copies. No host wait."""
    L = lib()
    L.jxlhip_halo_pack_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(L.jxlhip_halo_pack_batch(arr, len(ctxs), side, device_ptr, block_bytes, transport_stream), "jxlhip_halo_pack_batch")


def halo_unpack_batch(ctxs, side, device_ptr, block_bytes, transport_stream=0):
    """jxlhip_halo_unpack_batch: the copies follow what `transport_stream` holds now (the receive); the set's filter launch
    follows the copies. No host wait."""
    L = lib()
    L.jxlhip_halo_unpack_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(L.jxlhip_halo_unpack_batch(arr, len(ctxs), side, device_ptr, block_bytes, transport_stream), "jxlhip_halo_unpack_batch")


def run_transform_batch(ctxs):
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(lib().jxlhip_run_transform_batch(arr, len(ctxs)), "jxlhip_run_transform_batch")


def run_filter_color_batch(ctxs):
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(lib().jxlhip_run_filter_color_batch(arr, len(ctxs)), "jxlhip_run_filter_color_batch")


def run_modular_batch(ctxs):
    """Every stream of several resident Modular frames as one launch (jxlhip_modular_run_batch)."""
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(lib().jxlhip_modular_run_batch(arr, len(ctxs)), "jxlhip_modular_run_batch")


def run_reduced_batch(ctxs):
    """The reduced images of several contexts (upload_reduced) in one kernel launch (jxlhip_reduced_run_batch)."""
    L = lib()
    L.jxlhip_reduced_run_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(L.jxlhip_reduced_run_batch(arr, len(ctxs)), "jxlhip_reduced_run_batch")


def decode_reduced(data, data_type=2, num_channels=3, device=0, threads=0):
    """One-shot helper: the image at 1/8 scale from the DC sections of a VarDCT codestream (or a prefix of at least
    frame_dc_extent(data) bytes) -> ceil(H / 8) x ceil(W / 8) x C samples. Gaborish, EPF and noise are not applied. Raises
    JxlAmdError with the parser's text for a stream the reduced parse refuses; there is no fallback to a full decode."""
    f = Frame(data, threads, reduced=True)
    c = HipContext(device)
    try:
        c.set_output_format(data_type, num_channels)
        c.upload_reduced(f)
        c.run_reduced()
        return c.pixels()
    finally:
        c.close()
        f.close()


def decode_lossless(data, num_channels=3, data_type=2, device=0):
    """One-shot helper: Modular (lossless) codestream -> HxWxC samples through the GPU path."""
    f = ModFrame(data)
    c = HipContext(device)
    try:
        c.set_output_format(data_type, num_channels)
        c.upload_modular(f)
        c.run_modular()
        r, status, _ = c.modular_status()
        if r:
            raise JxlAmdError("corrupt Modular streams: %r" % [(i, s) for i, s in enumerate(status) if s])
        return c.pixels()
    finally:
        c.close()
        f.close()


def decode_rgb8(data, device=0, threads=0):
    """One-shot helper: codestream bytes -> HxWx3 uint8 through the GPU path."""
    f = Frame(data, threads)
    c = HipContext(device)
    try:
        c.upload(f)
        c.run_all()
        r, flags = c.errors()
        if r:
            raise JxlAmdError("corrupt AC sections: %r" % [(g, e) for g, e in enumerate(flags) if e])
        return c.rgb8()
    finally:
        c.close()
        f.close()


# ----------------------------------------------------------------------------------------------- synthetic streams
class EncParams(ctypes.Structure):
    _fields_ = [("distance", ctypes.c_float), ("epf_iters", ctypes.c_int32), ("gab", ctypes.c_int32),
                ("strategy_mode", ctypes.c_int32), ("strategy_mask", ctypes.c_uint32), ("seed", ctypes.c_uint32),
                ("max_clusters", ctypes.c_int32), ("skip_dc_smoothing", ctypes.c_int32), ("random_cmap", ctypes.c_int32),
                ("zero_ac", ctypes.c_int32), ("num_histograms", ctypes.c_int32), ("big_coeffs", ctypes.c_int32), ("num_passes", ctypes.c_int32), ("upsampling", ctypes.c_int32), ("custom_orders", ctypes.c_int32), ("custom_bctx", ctypes.c_int32),
                ("custom_cmap", ctypes.c_int32), ("custom_lf", ctypes.c_int32), ("ac_code_mode", ctypes.c_int32),
                ("noise", ctypes.c_int32), ("cfl_fit", ctypes.c_int32), ("color_transform", ctypes.c_int32), ("raw_quant", ctypes.c_int32),
                ("chroma_subsampling", ctypes.c_int32), ("ec_upsampling", ctypes.c_int32), ("adaptive_quant", ctypes.c_int32),
                ("acs_search", ctypes.c_int32)]


class EncHistDesc(ctypes.Structure):  # JxlHipEncHistDesc
    _fields_ = [("split_exp", ctypes.c_uint32), ("msb_in_token", ctypes.c_uint32), ("lsb_in_token", ctypes.c_uint32), ("num_ctx", ctypes.c_uint32)]


class EncAnsDesc(ctypes.Structure):  # JxlHipEncAnsDesc
    _fields_ = [("split_exp", ctypes.c_uint32), ("msb_in_token", ctypes.c_uint32), ("lsb_in_token", ctypes.c_uint32), ("num_ctx", ctypes.c_uint32),
                ("ctx_map", ctypes.c_void_p), ("num_clusters", ctypes.c_uint32), ("log_alpha", ctypes.c_uint32), ("freq", ctypes.c_void_p),
                ("rev_start", ctypes.c_void_p), ("rev", ctypes.c_void_p), ("prefix_count", ctypes.c_void_p), ("prefix_value", ctypes.c_void_p)]


class EncTokDesc(ctypes.Structure):  # JxlHipEncTokDesc
    _fields_ = [("orders", ctypes.c_void_p), ("orders_size", ctypes.c_uint32), ("order_offset", ctypes.c_uint32 * 13),
                ("ctx_map", ctypes.c_uint8 * 39), ("num_ctxs", ctypes.c_uint32), ("num_hist", ctypes.c_uint32)]


class CpuEncContext:
    """Test access: a JxlEncCpuCtx, the context of the jxlenc_cpu_* doubles of the encoder hooks. It keeps the model of
    the last enc_forward_model(img, this) for enc_tokens."""

    def __init__(self):
        self._h = _enc_lib().jxlenc_cpu_ctx_new()

    def close(self):
        if self._h:
            _enc_lib().jxlenc_cpu_ctx_free(self._h)
            self._h = None


def enc_tokens(ctx, orders, order_offset, ctx_map, num_ctxs, num_hist=1, guard=4):
    """Test access: the AC tokens of the last forward call on `ctx`, from jxlhip_enc_token_counts / jxlhip_enc_tokens (a
    HipContext) or the jxlenc_cpu_* pair (a CpuEncContext), under one JxlHipEncTokDesc: orders (uint16, bucket b at
    order_offset[b]), ctx_map[39], num_ctxs, num_hist. Returns (totals, per group an (n, 2) uint32 array of {context,
    value}, the `guard` pairs behind `capacity`, which were set to 0xA5A5A5A5 before the call)."""
    orders = np.ascontiguousarray(orders, np.uint16)
    d = EncTokDesc(orders.ctypes.data, orders.size, (ctypes.c_uint32 * 13)(*[int(v) for v in order_offset]),
                   (ctypes.c_uint8 * 39)(*[int(v) for v in ctx_map]), int(num_ctxs), int(num_hist))
    if isinstance(ctx, CpuEncContext):
        E = _enc_lib()
        counts, emit, what = E.jxlenc_cpu_token_counts, E.jxlenc_cpu_tokens, "jxlenc_cpu_token"
    else:
        L = lib()
        counts, emit, what = L.jxlhip_enc_token_counts, L.jxlhip_enc_tokens, "jxlhip_enc_token"
        counts.argtypes, emit.argtypes = [ctypes.c_void_p] * 3, [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    ng = ((ctx.enc_size[0] + 255) // 256) * ((ctx.enc_size[1] + 255) // 256)
    totals = np.zeros(ng, np.uint32)
    r = counts(ctx._h, ctypes.byref(d), totals.ctypes.data)
    if r:
        raise JxlAmdError("%s_counts failed: %d" % (what, r))
    bases = np.concatenate([[0], np.cumsum(totals)]).astype(np.uint32)
    total = int(totals.sum())
    buf = np.full((total + guard, 2), 0xA5A5A5A5, np.uint32)
    r = emit(ctx._h, bases.ctypes.data, buf.ctypes.data, total)
    if r:
        raise JxlAmdError("%ss failed: %d" % (what, r))
    return totals, [buf[int(bases[g]):int(bases[g + 1])].copy() for g in range(ng)], buf[total:].copy()


class EncHooks(ctypes.Structure):  # JxlEncHooks: forward; token_counts + tokens; histograms + ans_sizes + ans_write
    _fields_ = [(k, ctypes.c_void_p) for k in ("forward", "token_counts", "tokens", "histograms", "ans_sizes", "ans_write")]


class EncHookStats(ctypes.Structure):  # JxlEncHookStats
    _fields_ = [("forward_s", ctypes.c_double), ("assemble_s", ctypes.c_double), ("device_tokens", ctypes.c_uint64),
                ("device_coded", ctypes.c_uint64)]


class AnsTables:
    """An ANS code in the flat form the entropy entry points take: ctx_map (num_ctx,) uint8, freq and rev_start
    (clusters, 256) uint16, rev (clusters, 4096) uint16, log_alpha, the hybrid-uint configuration (split_exp, msb, lsb) and
    the prefix (bit count, value) written ahead of the coder state."""

    def __init__(self, ctx_map, freq, rev_start, rev, log_alpha, cfg=(4, 2, 0), prefix=(0, 0)):
        self.ctx_map = np.ascontiguousarray(ctx_map, np.uint8)
        self.freq = np.ascontiguousarray(freq, np.uint16).reshape(-1, 256)
        self.rev_start = np.ascontiguousarray(rev_start, np.uint16).reshape(-1, 256)
        self.rev = np.ascontiguousarray(rev, np.uint16).reshape(-1, 4096)
        self.log_alpha, self.cfg = int(log_alpha), tuple(cfg)
        self.prefix = (np.array([prefix[0]], np.uint8), np.array([prefix[1]], np.uint8))

    def desc(self):
        return EncAnsDesc(self.cfg[0], self.cfg[1], self.cfg[2], len(self.ctx_map), self.ctx_map.ctypes.data, len(self.freq), self.log_alpha,
                          self.freq.ctypes.data, self.rev_start.ctypes.data, self.rev.ctypes.data, self.prefix[0].ctypes.data,
                          self.prefix[1].ctypes.data)


def ans_write_tokens(tokens, tables, capacity=None):
    """The host rANS writer (jxlenc_ans_write_tokens) on (n, 2) uint32 {context, value} pairs and an AnsTables code:
    (the bit string as bytes, its length in bits)."""
    E = _enc_lib()
    tokens = np.ascontiguousarray(tokens, np.uint32).reshape(-1, 2)
    cap = 16 + 8 * len(tokens) if capacity is None else int(capacity)
    out = np.zeros(max(1, cap), np.uint8)
    bits = ctypes.c_uint64()
    d = tables.desc()
    r = E.jxlenc_ans_write_tokens(tokens.ctypes.data, len(tokens), ctypes.byref(d), out.ctypes.data, cap, ctypes.byref(bits))
    if r:
        raise JxlAmdError("jxlenc_ans_write_tokens failed: %d" % r)
    return out[:(bits.value + 7) // 8].tobytes(), int(bits.value)


def _enc_lib():
    """libjxlenc.so with the signature of every jxlenc_* entry declared, here and nowhere else."""
    global _enc
    if _enc is None:
        if not os.path.exists(ENC_PATH):
            raise JxlAmdError("%s is missing: run libjxl_amd.build()" % ENC_PATH)
        E = ctypes.CDLL(ENC_PATH)
        c_int, u32, vp, sz, cp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
        i32p, szp, pp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(sz), ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
        image = [cp, u32, u32, ctypes.POINTER(EncParams)]
        color = [c_int] + [u32] * 6 + [i32p]
        sigs = {  # name: (restype, argtypes)
            "encode_rgb8": (c_int, image + [pp, szp]),
            "encode_rgba8": (c_int, image + [pp, szp]),
            "encode_rgb8_hooks": (c_int, image + [ctypes.POINTER(EncHooks), vp, pp, szp, ctypes.POINTER(EncHookStats)]),
            "encode_lossless": (c_int, [cp] + [u32] * 5 + [pp, szp]),
            "encode_lossless_samples": (c_int, [vp] + [u32] * 7 + [pp, szp]),
            "encode_random": (c_int, image[1:] + [pp, szp]),
            "forward_model": (c_int, image + [vp] * 6),
            "ans_write_tokens": (c_int, [vp, sz, ctypes.POINTER(EncAnsDesc), vp, sz, ctypes.POINTER(ctypes.c_uint64)]),
            "synth_image": (None, [u32, u32, u32, vp]),
            "free": (None, [ctypes.POINTER(ctypes.c_uint8)]),
            "last_header_bytes": (sz, []),
            # the CPU doubles of the hooks (jxlhip_enc_* signatures, a JxlEncCpuCtx or NULL where those take the context)
            "cpu_ctx_new": (vp, []),
            "cpu_ctx_free": (None, [vp]),
            "cpu_forward": (c_int, [vp, vp, sz] + [vp] * 5),
            "cpu_token_counts": (c_int, [vp] * 3),
            "cpu_tokens": (c_int, [vp] * 3 + [sz]),
            "cpu_histograms": (c_int, [vp] * 4),
            "cpu_ans_sizes": (c_int, [vp] * 3),
            "cpu_ans_write": (c_int, [vp] * 3 + [sz]),
            "cpu_initial_quant_field": (c_int, [vp, u32, u32, ctypes.c_float, ctypes.c_float, vp, vp]),
            "cpu_masking_1x1": (c_int, [vp, u32, u32, vp]),
            "cpu_estimate_entropy": (c_int, [vp, vp, sz, vp, vp]),
            # (fn, ctx, xyb, xsize, ysize, quant_field, mask1x1, ytox, ytob, distance, candidates, n, estimates, scaled)
            "estimate_entropy": (c_int, [vp, vp, vp, u32, u32, vp, vp, vp, vp, ctypes.c_float, vp, sz, vp, vp]),
            "cpu_acs_walk": (c_int, [vp] * 4),
            "acs_walk_candidates": (ctypes.c_int64, [u32, u32, u32, vp, vp, sz]),
            "cpu_debug_enc_search": (c_int, [vp] * 6),
            # what the next streams carry (test aids)
            "set_custom_upsampling": (None, [u32, u32]),
            "set_embedded_icc": (None, [cp, sz, sz]),
            "set_color_encoding": (None, color),
            "set_xyb_color_encoding": (None, color + [ctypes.c_float]),
            "set_xyb_gray": (None, [c_int]),
            "set_frame_name": (None, [cp]),
            "set_orientation": (None, [u32]),
            "set_splines": (None, [i32p, sz]),
            "set_patches": (None, [i32p, sz]),
            "set_animation": (None, [c_int] + [u32] * 4 + [c_int]),
            "set_layer": (None, [c_int, ctypes.c_int32, ctypes.c_int32] + [u32] * 8 + [c_int]),
            "set_preview": (None, [c_int, u32, u32]),
            "set_alpha_premultiplied": (None, [c_int]),
            "set_reference_frame": (None, [c_int]),
            "set_image_size": (None, [u32, u32]),
            "set_dc_frame": (None, [c_int]),
            "set_use_dc_frame": (None, [c_int]),
        }
        for name, (restype, argtypes) in sigs.items():
            fn = getattr(E, "jxlenc_" + name)
            fn.restype, fn.argtypes = restype, argtypes
        _enc = E
    return _enc


def _params(**kw):
    p = EncParams()
    p.distance, p.epf_iters, p.gab, p.strategy_mode, p.strategy_mask, p.seed = 1.0, -1, -1, 1, 0, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def icc_decode(coded):
    """Coded ICC profile (the stream behind an image's headers) -> (profile bytes, exact length of the coded form in bits)."""
    L = lib()
    L.jxlamd_icc_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                    ctypes.POINTER(ctypes.c_size_t)]
    n, bits = ctypes.c_size_t(), ctypes.c_size_t()
    _check(L.jxlamd_icc_decode(coded, len(coded), None, 0, ctypes.byref(n), ctypes.byref(bits)), "jxlamd_icc_decode")
    out = ctypes.create_string_buffer(max(1, n.value))
    _check(L.jxlamd_icc_decode(coded, len(coded), out, n.value, ctypes.byref(n), ctypes.byref(bits)), "jxlamd_icc_decode")
    return out.raw[:n.value], bits.value


def set_custom_upsampling(mask=0, seed=1):
    """Test aid: the next VarDCT streams code their own upsampling weights (CustomTransformData, image_metadata.cc:87-214):
    bit k of `mask` = the 2^(k+1)-fold weight matrix is coded (seeded variations of the default weights); 0 = default again."""
    E = _enc_lib()
    E.jxlenc_set_custom_upsampling(mask, seed)


def set_embedded_icc(coded=None):
    """Test aid: the synthetic encoders embed this coded ICC profile (want_icc) in the streams they write from now on
    (None: no profile again)."""
    E = _enc_lib()
    if not coded:
        E.jxlenc_set_embedded_icc(b"", 0, 0)
        return
    _, bits = icc_decode(coded)
    E.jxlenc_set_embedded_icc(coded, len(coded), bits)


def set_color_encoding(white_point=None, primaries=1, transfer_function=13, gamma=None, intent=1, xy=None):
    """Test aid: the next LOSSLESS streams declare this enum colour encoding (values of jxl/color_encoding.h: white point
    1 D65 / 2 custom / 10 E / 11 DCI; primaries 1 sRGB / 2 custom / 9 Rec.2100 / 11 P3; transfer function 1 709 / 8 linear /
    13 sRGB / 16 PQ / 17 DCI / 18 HLG, or gamma as a float; xy = 8 custom chromaticities white, red, green, blue).
    white_point=None: sRGB again."""
    E = _enc_lib()
    if white_point is None:
        E.jxlenc_set_color_encoding(0, 1, 1, 0, 0, 13, 1, None)
        return
    arr = (ctypes.c_int32 * 8)(*[int(round(v * 1e6)) for v in (xy or [0] * 8)])
    E.jxlenc_set_color_encoding(1, white_point, primaries, 1 if gamma is not None else 0, int(round((gamma or 0) * 1e7)), transfer_function,
                                intent, arr)


def set_xyb_gray(on=True):
    """Test aid: the next streams of an XYB image (VarDCT, or encode_lossless with MODULAR_XYB) declare colour space Gray
    (with set_xyb_color_encoding's / set_color_encoding's white point and transfer function, D65 sRGB without). The body is
    the same three-channel XYB frame: a decoder renders its luminance."""
    E = _enc_lib()
    E.jxlenc_set_xyb_gray(1 if on else 0)


def set_xyb_color_encoding(white_point=None, primaries=1, transfer_function=13, gamma=None, intent=1, xy=None, intensity_target=255.0,
                           gray=False):
    """Test aid: the next VarDCT (XYB) streams declare this enum colour encoding (values as set_color_encoding) and, when it
    is not 255, this intensity target (ToneMapping). The coded samples do not change: the tag only changes how a decoder
    renders the same XYB body. gray: colour space Gray (no primaries) instead of RGB (set_xyb_gray). white_point=None:
    untagged again (the streams are then byte-identical to before)."""
    E = _enc_lib()
    set_xyb_gray(gray and white_point is not None)
    if white_point is None:
        E.jxlenc_set_xyb_color_encoding(0, 1, 1, 0, 0, 13, 1, None, 255.0)
        return
    arr = (ctypes.c_int32 * 8)(*[int(round(v * 1e6)) for v in (xy or [0] * 8)])
    E.jxlenc_set_xyb_color_encoding(1, white_point, primaries, 1 if gamma is not None else 0, int(round((gamma or 0) * 1e7)),
                                    transfer_function, intent, arr, float(intensity_target))


def set_frame_name(name=""):
    """Test aid: the frames written from now on carry this name (empty: none again)."""
    E = _enc_lib()
    E.jxlenc_set_frame_name(name.encode())


def set_orientation(orientation=1):
    """Test aid: the synthetic encoders declare this image orientation (1..8, EXIF numbering) in the streams they write
    from now on (1: none again)."""
    E = _enc_lib()
    E.jxlenc_set_orientation(int(orientation))


def set_splines(splines=None, quantization_adjustment=0):
    """Test aid: the next streams carry these quantised splines (None: none again). Each spline is a dict: points (list of
    integer (x, y) control points), color ([3][32] integer DCT coefficients of X, Y, B along the arc) and sigma ([32])."""
    E = _enc_lib()
    if not splines:
        E.jxlenc_set_splines(None, 0)
        return
    flat = [int(quantization_adjustment), len(splines)]
    for sp in splines:
        pts = [(int(x), int(y)) for x, y in sp["points"]]
        flat += [pts[0][0], pts[0][1], len(pts) - 1]
        pdx = pdy = 0
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):  # double deltas (splines.cc:411-431)
            dx, dy = x1 - x0, y1 - y0
            flat += [dx - pdx, dy - pdy]
            pdx, pdy = dx, dy
        for c in range(3):
            flat += [int(v) for v in sp["color"][c]]
        flat += [int(v) for v in sp["sigma"]]
    arr = (ctypes.c_int32 * len(flat))(*flat)
    E.jxlenc_set_splines(arr, len(flat))


def encode_animation(frames, durations, tps=(10, 1), num_loops=0, lossless=False, **kw):
    """Test aid: an animation of full-size frames that replace each other (no layers, blending, crops or references):
    frames[i] (HxWx3 or HxWx4 uint8, all of one size) is shown for durations[i] ticks of tps[0] / tps[1] per second."""
    E = _enc_lib()
    out = b""
    try:
        for i, (img, dur) in enumerate(zip(frames, durations)):
            E.jxlenc_set_animation(1, tps[0], tps[1], num_loops, dur, 1 if i == len(frames) - 1 else 0)
            if lossless:
                d = encode_lossless(img, **kw)
            elif img.shape[2] == 4:
                d = encode_rgba8(img, **kw)
            else:
                d = encode_rgb8(img, **kw)
            out += d if i == 0 else d[E.jxlenc_last_header_bytes():]
    finally:
        E.jxlenc_set_animation(0, 10, 1, 0, 0, 1)
    return out


def encode_layers(layers, tps=None, num_loops=0, lossless=False, premultiplied=False, **kw):
    """Test aid: a codestream of several frames composed on a canvas (blending.cc): layers[i] is a dict with img (HxWx3 or
    HxWx4 uint8; layers[0] covers the whole canvas at the origin and gives its size) and optionally x0, y0 (crop origin),
    mode / alpha_mode (BlendMode of colour / alpha: 0 replace, 1 add, 2 blend, 3 alpha-weighted add, 4 multiply), source /
    alpha_source (reference slots), clamp, save_as (slot the blended canvas is kept in) and duration. tps = (numerator,
    denominator) makes it an animation (frames with duration > 0 are shown); tps = None a layered still (only the last
    frame is shown)."""
    E = _enc_lib()
    ch, cw = layers[0]["img"].shape[:2]
    out = b""
    E.jxlenc_set_alpha_premultiplied(1 if premultiplied else 0)  # (the alpha channel is declared associated; samples as given)
    try:
        for i, L in enumerate(layers):
            img = L["img"]
            E.jxlenc_set_animation(1, tps[0] if tps else 10, tps[1] if tps else 1, num_loops, L.get("duration", 0),
                                   1 if i == len(layers) - 1 else 0)
            E.jxlenc_set_layer(1, L.get("x0", 0), L.get("y0", 0), cw, ch, L.get("mode", 0), L.get("alpha_mode", 0), L.get("source", 0),
                               L.get("alpha_source", L.get("source", 0)), L.get("clamp", 0), L.get("save_as", 0), 1 if tps else 0)
            if lossless:
                d = encode_lossless(img, **kw)
            elif img.shape[2] == 4:
                d = encode_rgba8(img, **kw)
            else:
                d = encode_rgb8(img, **kw)
            out += d if i == 0 else d[E.jxlenc_last_header_bytes():]
    finally:
        E.jxlenc_set_layer(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)
        E.jxlenc_set_animation(0, 10, 1, 0, 0, 1)
        E.jxlenc_set_alpha_premultiplied(0)
    return out


def encode_with_preview(img, preview, **kw):
    """Test aid: `img` (HxWx3 uint8, VarDCT) with a VarDCT preview frame (hxwx3 uint8):
    the image header announces the preview's size (headers.cc:155-183) and the preview is the codestream's first frame, a
    regular frame that is not the last (decode.cc:1266-1268)."""
    E = _enc_lib()
    try:
        E.jxlenc_set_animation(1, 10, 1, 0, 0, 0)  # (multi-frame ...
        E.jxlenc_set_layer(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)  # ... untimed: a frame header with is_last = false, no duration)
        p = encode_rgb8(preview)
        pframe = p[E.jxlenc_last_header_bytes():]
        E.jxlenc_set_animation(0, 10, 1, 0, 0, 1)
        E.jxlenc_set_preview(1, preview.shape[1], preview.shape[0])
        m = encode_rgb8(img, **kw)
        h = E.jxlenc_last_header_bytes()
    finally:
        E.jxlenc_set_animation(0, 10, 1, 0, 0, 1)
        E.jxlenc_set_layer(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)
        E.jxlenc_set_preview(0, 0, 0)
    return m[:h] + pframe + m[h:]


def encode_patched(img, atlas, patches, slot=1, atlas_vardct=False, lossless=False, premultiplied=False, lossless_flags=None, **kw):
    """Test aid: a reference-only frame holding `atlas` (HxWx3 uint8; coded as an XYB Modular frame like libjxl's patch
    frames, or as a VarDCT frame) kept in `slot`, then `img` coded with a patch dictionary. patches: list of dicts with
    x0, y0, xsize, ysize (rectangle in the atlas) and positions: list of (x, y, mode, clamp[, alpha mode, alpha clamp]) with
    PatchBlendMode 0 none, 1 replace, 2 add, 3 multiply, 4 / 5 blend above / below, 6 / 7 alpha-weighted add above / below
    (dec_patch_dictionary.h:32-58); the last two apply to the image's alpha channel (RGBA `img` and `atlas`, VarDCT atlas).
    The patches are drawn over the decoded frame; nothing is subtracted when encoding."""
    E = _enc_lib()
    flat = [len(patches)]
    for p in patches:
        flat += [slot, p["x0"], p["y0"], p["xsize"], p["ysize"], len(p["positions"])]
        for pos in p["positions"]:
            flat += list(pos) + [0] * (6 - len(pos))
    try:
        E.jxlenc_set_alpha_premultiplied(1 if premultiplied else 0)  # (the alpha channel is declared associated; samples as given)
        E.jxlenc_set_image_size(img.shape[1], img.shape[0])
        E.jxlenc_set_reference_frame(slot)
        mflags = MODULAR_XYB if lossless_flags is None else lossless_flags  # (lossless_flags: both frames Modular, e.g. plain RGB with an RCT)
        first = (encode_rgba8(atlas, **kw) if atlas.shape[2] == 4 else encode_rgb8(atlas, **kw)) if atlas_vardct else encode_lossless(atlas, mflags)
        E.jxlenc_set_reference_frame(-1)
        arr = (ctypes.c_int32 * len(flat))(*flat)
        E.jxlenc_set_patches(arr, len(flat))
        second = encode_lossless(img, mflags) if lossless else (encode_rgba8(img, **kw) if img.shape[2] == 4 else encode_rgb8(img, **kw))
        return first + second[E.jxlenc_last_header_bytes():]
    finally:
        E.jxlenc_set_alpha_premultiplied(0)
        E.jxlenc_set_reference_frame(-1)
        E.jxlenc_set_patches(None, 0)
        E.jxlenc_set_image_size(0, 0)


def encode_with_dc_frame(img, dc_vardct=False, **kw):
    """Test aid: what `cjxl --progressive_dc` lays out: a kDCFrame of level 1 (the image's 8x8 block means, 1/8 size; coded as
    an XYB Modular frame like libjxl's DC frames, or as a VarDCT frame), then `img` as a VarDCT frame with kUseDcFrame, whose
    DC groups carry no DC stream: its DC image is the DC frame's output (frame_header.h:348, passes_state.cc:62-77)."""
    E = _enc_lib()
    h, w = img.shape[:2]
    xb, yb = (w + 7) // 8, (h + 7) // 8
    pad = np.pad(img, ((0, yb * 8 - h), (0, xb * 8 - w), (0, 0)), mode="edge")
    small = np.ascontiguousarray(pad.reshape(yb, 8, xb, 8, 3).mean(axis=(1, 3)).round().astype(np.uint8))
    try:
        E.jxlenc_set_image_size(w, h)
        E.jxlenc_set_dc_frame(1)
        first = encode_rgb8(small, **kw) if dc_vardct else encode_lossless(small, MODULAR_XYB)
        E.jxlenc_set_dc_frame(0)
        E.jxlenc_set_use_dc_frame(1)
        second = encode_rgb8(img, **kw)
        return first + second[E.jxlenc_last_header_bytes():]
    finally:
        E.jxlenc_set_dc_frame(0)
        E.jxlenc_set_use_dc_frame(0)
        E.jxlenc_set_image_size(0, 0)


def synth_image(xsize, ysize, seed=177):
    """Deterministic synthetic RGB8 test image (gradient background, rectangles, discs, texture, noise)."""
    a = np.zeros((ysize, xsize, 3), np.uint8)
    _enc_lib().jxlenc_synth_image(xsize, ysize, seed, a.ctypes.data)
    return a


def _finish(E, r, out, n, what):
    if r:
        raise JxlAmdError("%s failed: %d" % (what, r))
    b = ctypes.string_at(out, n.value)
    E.jxlenc_free(out)
    return b


def encode_rgb8(img, **kw):
    """RGB8 image -> VarDCT codestream (distance=1.0, strategy_mode=1 by default)."""
    E = _enc_lib()
    img = np.ascontiguousarray(img, np.uint8)
    p = _params(**kw)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    r = E.jxlenc_encode_rgb8(img.tobytes(), img.shape[1], img.shape[0], ctypes.byref(p), ctypes.byref(out), ctypes.byref(n))
    return _finish(E, r, out, n, "jxlenc_encode_rgb8")


def _encode_hooks(img, p, fns, handle):
    """jxlenc_encode_rgb8_hooks with the functions `fns` (forward[, token_counts, tokens[, histograms, ans_sizes,
    ans_write]]) on the context `handle`: (the stream, its JxlEncHookStats)."""
    E = _enc_lib()
    img = np.ascontiguousarray(img, np.uint8)
    hooks = EncHooks(*[ctypes.cast(f, ctypes.c_void_p).value for f in fns])
    out, n, st = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(), EncHookStats()
    r = E.jxlenc_encode_rgb8_hooks(img.tobytes(), img.shape[1], img.shape[0], ctypes.byref(p), ctypes.byref(hooks), handle, ctypes.byref(out),
                                   ctypes.byref(n), ctypes.byref(st))
    return _finish(E, r, out, n, "jxlenc_encode_rgb8_hooks"), st


def encode_rgb8_hooks_cpu(img, timings=None, **kw):
    """The route of encode_rgb8_gpu(device_entropy=True) with CPU doubles behind every hook (forward, tokens, histograms,
    rANS sizes / write): the plumbing of that route on a machine without a GPU. `timings` receives device_tokens and
    device_entropy as there."""
    E = _enc_lib()
    h = E.jxlenc_cpu_ctx_new()
    try:
        data, st = _encode_hooks(img, _params(**kw), [E.jxlenc_cpu_forward, E.jxlenc_cpu_token_counts, E.jxlenc_cpu_tokens,
                                                      E.jxlenc_cpu_histograms, E.jxlenc_cpu_ans_sizes, E.jxlenc_cpu_ans_write], h)
    finally:
        E.jxlenc_cpu_ctx_free(h)
    if timings is not None:
        timings.update(forward_s=st.forward_s, assemble_s=st.assemble_s, device_tokens=st.device_tokens, device_entropy=st.device_coded)
    return data


def encode_rgb8_gpu(img, ctx, timings=None, device_tokens=False, device_entropy=False, **kw):
    """VarDCT-encodes an RGB8 image with the pixel-domain half (colour, sharpening, transform selection, forward DCT,
    quantisation) on the GPU (jxlhip_enc_forward on `ctx`) and entropy coding / headers on the host. `timings` (a dict)
    receives forward_s (the call, copies included), assemble_s and kernels_ms (HIP events around the launches).
    device_tokens: the coefficients are tokenised on the device too (jxlhip_enc_tokens) and never copied to the host.
    device_entropy (implies device_tokens): the tokens are counted and rANS-coded there as well (jxlhip_enc_histograms,
    jxlhip_enc_ans_sizes / _write): only the counts and the coded AC sections come to the host, which clusters, normalises
    and writes the headers. Prefix codes, LZ77, several passes and coded orders / block contexts fall back to the host
    coder. `timings` then also receives device_entropy (tokens coded on the device, 0 after that fallback) and
    entropy_kernels_ms (the histogram, sizes and write kernels). The stream is the same bytes in all three forms."""
    L = lib()
    L.jxlhip_enc_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    fns = [L.jxlhip_enc_forward]
    if device_tokens or device_entropy:
        fns += [L.jxlhip_enc_token_counts, L.jxlhip_enc_tokens]
    if device_entropy:
        fns += [L.jxlhip_enc_histograms, L.jxlhip_enc_ans_sizes, L.jxlhip_enc_ans_write]
    data, st = _encode_hooks(img, _params(**kw), fns, ctx._h)
    if timings is not None:
        ms = ctypes.c_float()
        _check(L.jxlhip_enc_last_ms(ctx._h, ctypes.byref(ms)), "jxlhip_enc_last_ms")
        timings.update(forward_s=st.forward_s, assemble_s=st.assemble_s, kernels_ms=ms.value, device_tokens=st.device_tokens)
        if device_entropy:
            timings.update(device_entropy=st.device_coded, entropy_kernels_ms=sum(ctx.enc_entropy_ms()) if st.device_coded else 0.0)
    return data


def enc_forward_model(img, ctx=None, **kw):
    """Test access: the raw outputs of one forward call (acs, qf, dc, coeffs) from the GPU path on `ctx`, or from the
    CPU stream writer's own model code when ctx is None or a CpuEncContext (which keeps the model, for enc_tokens)."""
    E = _enc_lib()
    img = np.ascontiguousarray(img, np.uint8)
    ys, xs = img.shape[:2]
    xb, yb, ng = (xs + 7) // 8, (ys + 7) // 8, ((xs + 255) // 256) * ((ys + 255) // 256)
    acs, qf = np.zeros((yb, xb), np.uint8), np.zeros((yb, xb), np.int32)
    dc, co = np.zeros((3, yb, xb), np.int32), np.zeros((ng, 3, 65536), np.int32)
    p = _params(**kw)
    cpu = ctx is None or isinstance(ctx, CpuEncContext)
    fn = ctypes.cast(E.jxlenc_cpu_forward if cpu else lib().jxlhip_enc_forward, ctypes.c_void_p)
    r = E.jxlenc_forward_model(img.tobytes(), xs, ys, ctypes.byref(p), fn, ctx._h if ctx is not None else None, acs.ctypes.data,
                               qf.ctypes.data, dc.ctypes.data, co.ctypes.data)
    if r:
        raise JxlAmdError("jxlenc_forward_model failed (%d)" % r)
    if ctx is not None:
        ctx.enc_size = (xs, ys)
    return dict(acs=acs, qf=qf, dc=dc, coeffs=co)


def initial_quant_field(xyb, distance, ctx=None, rescale=1.0):
    """The reference's initial adaptive quant field of X, Y, B planes [3][ysize][xsize] (float32, sizes multiples of 8) built
    for `distance` (the frame's, or 0.62 of it for a frame without Gaborish): (aq_map, mask), both [ysize / 8][xsize / 8].
    On the GPU (jxlhip_enc_initial_quant_field on `ctx`), or from the CPU stream writer's own code when ctx is None."""
    xyb = np.ascontiguousarray(xyb, np.float32)
    if xyb.ndim != 3 or xyb.shape[0] != 3:
        raise ValueError("xyb: [3][ysize][xsize]")
    ys, xs = xyb.shape[1:]
    aq, mask = np.zeros((ys // 8, xs // 8), np.float32), np.zeros((ys // 8, xs // 8), np.float32)
    tail = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    args = (xyb.ctypes.data, xs, ys, float(distance), float(rescale), aq.ctypes.data, mask.ctypes.data)
    if ctx is not None:
        L = lib()
        L.jxlhip_enc_initial_quant_field.argtypes = [ctypes.c_void_p] + tail
        _check(L.jxlhip_enc_initial_quant_field(ctx._h, *args), "jxlhip_enc_initial_quant_field")
    else:
        E = _enc_lib()
        r = E.jxlenc_cpu_initial_quant_field(*args)
        if r:
            raise JxlAmdError("jxlenc_cpu_initial_quant_field failed (%d)" % r)
    return aq, mask


def masking_1x1(xyb, ctx=None):
    """The per-pixel masking the reference's AC-strategy search reads (mask1x1) of X, Y, B planes [3][ysize][xsize] (float32,
    sizes multiples of 8, before any sharpening): [ysize][xsize] float32. On the GPU (jxlhip_enc_masking_1x1 on `ctx`), or
    from the CPU stream writer's own code when ctx is None."""
    xyb = np.ascontiguousarray(xyb, np.float32)
    if xyb.ndim != 3 or xyb.shape[0] != 3:
        raise ValueError("xyb: [3][ysize][xsize]")
    ys, xs = xyb.shape[1:]
    out = np.zeros((ys, xs), np.float32)
    args = (xyb.ctypes.data, xs, ys, out.ctypes.data)
    if ctx is not None:
        L = lib()
        L.jxlhip_enc_masking_1x1.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        _check(L.jxlhip_enc_masking_1x1(ctx._h, *args), "jxlhip_enc_masking_1x1")
    else:
        r = _enc_lib().jxlenc_cpu_masking_1x1(*args)
        if r:
            raise JxlAmdError("jxlenc_cpu_masking_1x1 failed (%d)" % r)
    return out


# JxlHipEncAcsCandidate; the blocks (x, y) the pure-DCT strategies of estimate_entropy cover
ACS_CANDIDATE = np.dtype([("strategy", "<u4"), ("bx", "<u4"), ("by", "<u4"), ("entropy_mul", "<f4")])
ACS_ESTIMATE_COVERED = {0: (1, 1), 4: (2, 2), 5: (4, 4), 6: (1, 2), 7: (2, 1), 8: (1, 4), 9: (4, 1), 10: (2, 4), 11: (4, 2),
                        18: (8, 8), 19: (4, 8), 20: (8, 4)}


def estimate_entropy(xyb, quant_field, mask1x1, ytox, ytob, distance, candidates, ctx=None, want_scaled=False):
    """The cost estimate of the reference's AC-strategy search (EstimateEntropy) of `candidates`, (strategy, bx, by,
    entropy_mul) each (or an ACS_CANDIDATE array), on X, Y, B planes [3][ysize][xsize] (float32, sizes multiples of 8) with
    the quant field [ysize / 8][xsize / 8] of initial_quant_field, the masking of masking_1x1 and one int8 chroma-from-luma
    factor per 64x64 tile: float32 estimates [n], or (estimates, scaled) where scaled holds per candidate [3][R][C] the
    quantised values before rounding, candidates back to back. On the GPU (jxlhip_enc_estimate_entropy on `ctx`), or from
    the CPU stream writer's own code when ctx is None; both on the default library's dequantisation tables."""
    xyb = np.ascontiguousarray(xyb, np.float32)
    if xyb.ndim != 3 or xyb.shape[0] != 3:
        raise ValueError("xyb: [3][ysize][xsize]")
    ys, xs = xyb.shape[1:]
    tiles = ((ys + 63) // 64) * ((xs + 63) // 64)
    qf = np.ascontiguousarray(quant_field, np.float32)
    m = np.ascontiguousarray(mask1x1, np.float32)
    tx, tb = np.ascontiguousarray(ytox, np.int8).ravel(), np.ascontiguousarray(ytob, np.int8).ravel()
    if qf.size != (ys // 8) * (xs // 8) or m.size != ys * xs or tx.size != tiles or tb.size != tiles:
        raise ValueError("quant_field [ysize / 8][xsize / 8], mask1x1 [ysize][xsize], ytox / ytob one per 64x64 tile")
    if isinstance(candidates, np.ndarray) and candidates.dtype == ACS_CANDIDATE:
        cand = np.ascontiguousarray(candidates)
    else:
        cand = np.array([tuple(c) for c in candidates], ACS_CANDIDATE)
    n = len(cand)
    est = np.zeros(n, np.float32)
    scaled = None
    if want_scaled:
        area = sum(64 * ACS_ESTIMATE_COVERED.get(int(s), (0, 0))[0] * ACS_ESTIMATE_COVERED.get(int(s), (0, 0))[1] for s in cand["strategy"])
        scaled = np.zeros(3 * area, np.float32)
    fn = None
    if ctx is not None:
        fn = ctypes.cast(lib().jxlhip_enc_estimate_entropy, ctypes.c_void_p)
    r = _enc_lib().jxlenc_estimate_entropy(fn, ctx._h if ctx is not None else None, xyb.ctypes.data, xs, ys, qf.ctypes.data, m.ctypes.data,
                                           tx.ctypes.data, tb.ctypes.data, float(distance), cand.ctypes.data, n, est.ctypes.data,
                                           scaled.ctypes.data if want_scaled else None)
    if r:
        if ctx is not None:
            _check(r, "jxlhip_enc_estimate_entropy")
        raise JxlAmdError("jxlenc_cpu_estimate_entropy failed (%d)" % r)
    return (est, scaled) if want_scaled else est


class AcsWalkDesc(ctypes.Structure):  # JxlHipEncAcsWalkDesc
    _fields_ = [("xb", ctypes.c_uint32), ("yb", ctypes.c_uint32), ("distance", ctypes.c_float), ("floating", ctypes.c_uint32)]


# the ten kinds of the walk's table in its order, as AcStrategy numbers (rows x columns: 8x8, 16x8, 8x16, 16x16, 32x16, 16x32,
# 32x32, 64x32, 32x64, 64x64)
ACS_WALK_STRATEGIES = (0, 6, 7, 4, 10, 11, 5, 19, 20, 18)


def acs_walk_candidates(xb, yb, floating=0):
    """The candidates the reference's merge walk over a frame of xb x yb blocks can ask for, with the multipliers it attaches:
    (an ACS_CANDIDATE array grouped by kind, the uint32 place of each in the walk's table [tile][kind][cy][cx])."""
    E = _enc_lib()
    n = E.jxlenc_acs_walk_candidates(int(xb), int(yb), int(floating), None, None, 0)
    if n < 0:
        raise JxlAmdError("jxlenc_acs_walk_candidates failed (%d)" % n)
    cand, index = np.zeros(n, ACS_CANDIDATE), np.zeros(n, np.uint32)
    E.jxlenc_acs_walk_candidates(int(xb), int(yb), int(floating), cand.ctypes.data, index.ctypes.data, n)
    return cand, index


def ac_strategy_walk(estimates, xb, yb, distance, floating=0, ctx=None, want_entropy=False):
    """The merge walk of the reference's AC-strategy search on a table of estimates, float32 [tiles][10][8][8] (tiles of 64x64
    in raster order; see acs_walk_candidates): acs [yb][xb] uint8 = (strategy << 1) | first, or (acs, the walk's final
    entropy estimate per block [yb][xb]). On the GPU (jxlhip_enc_acs_walk on `ctx`), or the CPU double when ctx is None."""
    tiles = ((int(xb) + 7) // 8) * ((int(yb) + 7) // 8)
    est = np.ascontiguousarray(estimates, np.float32)
    if est.size != tiles * 640:
        raise ValueError("estimates: [tiles][10][8][8]")
    d = AcsWalkDesc(int(xb), int(yb), float(distance), int(floating))
    acs = np.zeros((max(int(yb), 0), max(int(xb), 0)), np.uint8)
    ent = np.zeros(acs.shape, np.float32)
    if ctx is not None:
        L = lib()
        L.jxlhip_enc_acs_walk.argtypes = [ctypes.c_void_p, ctypes.POINTER(AcsWalkDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.jxlhip_enc_acs_walk(ctx._h, ctypes.byref(d), est.ctypes.data, acs.ctypes.data, ent.ctypes.data if want_entropy else None),
               "jxlhip_enc_acs_walk")
    else:
        r = _enc_lib().jxlenc_cpu_acs_walk(ctypes.byref(d), est.ctypes.data, acs.ctypes.data, ent.ctypes.data if want_entropy else None)
        if r:
            raise JxlAmdError("jxlenc_cpu_acs_walk failed (%d)" % r)
    return (acs, ent) if want_entropy else acs


def enc_search_debug(ctx):
    """Test access: what the search of the last enc_forward_model(img, ctx, adaptive_quant=1, acs_search=1 or 2) read and
    wrote (ctx a HipContext or a CpuEncContext): dict of before / after (the XYB planes [3][yp][xp] before and after the
    sharpening), aq_map [yb][xb], mask1x1 [yp][xp] and estimates [tiles][10][8][8]."""
    xs, ys = ctx.enc_size
    xb, yb = (xs + 7) // 8, (ys + 7) // 8
    tiles = ((xb + 7) // 8) * ((yb + 7) // 8)
    out = dict(before=np.zeros((3, yb * 8, xb * 8), np.float32), after=np.zeros((3, yb * 8, xb * 8), np.float32),
               aq_map=np.zeros((yb, xb), np.float32), mask1x1=np.zeros((yb * 8, xb * 8), np.float32),
               estimates=np.zeros((tiles, 10, 8, 8), np.float32))
    args = [out[k].ctypes.data for k in ("before", "after", "aq_map", "mask1x1", "estimates")]
    if isinstance(ctx, CpuEncContext):
        r = _enc_lib().jxlenc_cpu_debug_enc_search(ctx._h, *args)
        if r:
            raise JxlAmdError("jxlenc_cpu_debug_enc_search failed (%d)" % r)
    else:
        L = lib()
        L.jxlhip_debug_enc_search.argtypes = [ctypes.c_void_p] * 6
        _check(L.jxlhip_debug_enc_search(ctx._h, *args), "jxlhip_debug_enc_search")
    return out


def encode_rgba8(img, **kw):
    """RGBA8 image -> VarDCT codestream with alpha as a (lossless) Modular-coded extra channel."""
    E = _enc_lib()
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 4
    p = _params(**kw)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    r = E.jxlenc_encode_rgba8(img.tobytes(), img.shape[1], img.shape[0], ctypes.byref(p), ctypes.byref(out), ctypes.byref(n))
    return _finish(E, r, out, n, "jxlenc_encode_rgba8")


LOSSLESS_PREFIX, LOSSLESS_LZ77, LOSSLESS_WP, LOSSLESS_SQUEEZE, LOSSLESS_RCT, LOSSLESS_ALL_PREDICTORS, LOSSLESS_PREV_CHANNEL = 1, 2, 4, 8, 16, 32, 64
MODULAR_XYB = 128  # the frame codes XYB integers (Y, X, B - Y): "lossy Modular", not lossless any more
# transforms in the group headers, each group on its own rectangle (frames of more than one group): an RCT (seed 0: YCoCg,
# else types and permutations by seed and group); palettes (all colour channels when the group has at most `palette_colors`
# colours, else one per colour channel with at most that many values); default Squeeze; a palette with ONE explicit entry
# whose other colours must all be implicit ones (the call fails otherwise)
LOSSLESS_LOCAL_RCT, LOSSLESS_LOCAL_PALETTE, LOSSLESS_LOCAL_SQUEEZE, LOSSLESS_LOCAL_IMPLICIT = 256, 512, 1024, 2048


def _lossless_flags(flags, palette_colors):
    if not 0 <= palette_colors < 65536:
        raise ValueError("palette_colors: 0 (= 256) .. 65535")
    return (flags & 0xFFFF) | (palette_colors << 16)


def encode_lossless(img, flags=LOSSLESS_RCT, seed=0, palette_colors=0):
    """HxWxC uint8 image (C = 1..4: grey, grey + alpha, RGB, RGBA) -> lossless Modular codestream. flags: LOSSLESS_*."""
    flags = _lossless_flags(flags, palette_colors)
    E = _enc_lib()
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    r = E.jxlenc_encode_lossless(img.tobytes(), img.shape[1], img.shape[0], img.shape[2], flags, seed, ctypes.byref(out), ctypes.byref(n))
    return _finish(E, r, out, n, "jxlenc_encode_lossless")


def encode_lossless_samples(samples, bits, exp_bits=0, flags=0, seed=0, palette_colors=0):
    """HxWxC int32 samples (C = 1..4) -> lossless Modular codestream of an image with `bits`-bit integer samples, or
    (exp_bits != 0) float samples of `bits` bits whose bit patterns the integers are (32 / 8: float32 viewed as int32,
    16 / 5: float16 viewed as uint16). An alpha channel (C = 2 or 4) stays 8-bit."""
    E = _enc_lib()
    flags = _lossless_flags(flags, palette_colors)
    a = np.ascontiguousarray(samples, np.int32)
    if a.ndim == 2:
        a = a[..., None]
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    r = E.jxlenc_encode_lossless_samples(a.ctypes.data, a.shape[1], a.shape[0], a.shape[2], flags, seed, bits, exp_bits,
                                         ctypes.byref(out), ctypes.byref(n))
    return _finish(E, r, out, n, "jxlenc_encode_lossless_samples")


def encode_random(xsize, ysize, **kw):
    """Random valid VarDCT codestream exercising the strategies in strategy_mask (0 = all 27)."""
    E = _enc_lib()
    p = _params(**kw)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    r = E.jxlenc_encode_random(xsize, ysize, ctypes.byref(p), ctypes.byref(out), ctypes.byref(n))
    return _finish(E, r, out, n, "jxlenc_encode_random")
