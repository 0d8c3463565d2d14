"""Decode straight into torch tensors on the device (jxlhip_set_output_tensor): the writer kernels store every sample once,
in the layout and type the consumer asked for, into memory the consumer owns. torch is imported here only.

    img = torch_io.decode_to_tensor(data, dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    batch = torch_io.decode_batch_to_tensor(datas, dtype=torch.bfloat16)     # (N, 3, H, W), one launch per stage
    crops = torch_io.decode_batch_to_tensor(datas, size=(224, 224), boxes=boxes)  # any sizes: crop + antialiased resize
    thumbs = torch_io.decode_batch_to_tensor(datas, size=(224, 224), reduce=8)    # from the 1/8-scale DC image: no AC decode

A crop (size and box) of a VarDCT frame decodes only the 256 x 256 groups the box reads (region=True, the default: Frame.
plan_window, HipContext.upload_window); the tensor is bit for bit the one region=False gives, which decodes the whole frame.
One deviation: a damaged AC section in a group the box does not read goes unnoticed.

Float types hold v * (1 / std[c]) + (-mean[c] / std[c]) of the decoder's float sample v in [0, 1] (scale and bias computed
in float32, the product and the sum each rounded to float32, then to the type); uint8 holds the dithered 8-bit sample.
The tensor's stream (torch.cuda.current_stream() unless given) is ordered before and behind the writes on the device:
no host synchronisation happens, and work queued on that stream afterwards sees the pixels.
"""
import numpy as np
import torch

import libjxl_amd as J

_DTYPES = {torch.uint8: J.TENSOR_U8, torch.float16: J.TENSOR_F16, torch.bfloat16: J.TENSOR_BF16, torch.float32: J.TENSOR_F32}


def affine(mean, std, channels):
    """scale = 1 / std and bias = -mean / std per channel, computed in float32. None: mean 0 / std 1; a scalar serves every
    colour channel; channels behind those given (alpha behind three colour values) keep mean 0 / std 1."""
    def per_channel(v, default):
        out = np.full(channels, default, np.float32)
        if v is not None:
            v = np.atleast_1d(np.asarray(v, np.float32))
            if v.size == 1:
                v = np.repeat(v, 1 if channels < 3 else 3)
            if v.size > channels:
                raise ValueError("%d values for %d channels" % (v.size, channels))
            out[:v.size] = v
        return out
    m, s = per_channel(mean, 0.0), per_channel(std, 1.0)
    return (np.float32(1) / s).astype(np.float32), (-m / s).astype(np.float32)


def bind(ctx, tensor, layout="CHW", mean=None, std=None, clamp=False, stream=None):
    """Binds a 3-d device tensor (any strides: a slice of a batch, a padded pitch, channels-last storage) as the output of
    ctx's next uploads; layout names its dimensions. The tensor must stay alive until the decode that fills it has been
    queued and its consumers have been queued behind it on `stream`."""
    if layout not in ("CHW", "HWC"):
        raise ValueError("layout is 'CHW' or 'HWC'")
    if tensor.dim() != 3 or not tensor.is_cuda or tensor.dtype not in _DTYPES:
        raise ValueError("a 3-d uint8 / float16 / bfloat16 / float32 tensor on the device")
    st = tensor.stride()
    sc, sy, sx = (st[0], st[1], st[2]) if layout == "CHW" else (st[2], st[0], st[1])
    channels = tensor.shape[0] if layout == "CHW" else tensor.shape[2]
    scale, bias = affine(mean, std, channels)
    if stream is None:
        stream = torch.cuda.current_stream(tensor.device)
    # room behind the first element: what the tensor's own storage holds from there on
    room = tensor.untyped_storage().nbytes() - tensor.storage_offset() * tensor.element_size()
    ctx.set_output_tensor(tensor.data_ptr(), room, _DTYPES[tensor.dtype], channels, (sc, sy, sx), scale, bias, clamp,
                          getattr(stream, "cuda_stream", stream))
    ctx._bound_tensor = tensor  # keeps the memory alive while it is bound


def bind_resized(ctx, tensor, layout="CHW", box=None, mean=None, std=None, clamp=False, stream=None):
    """Binds a 3-d device tensor as the output of ctx's next uploads like bind(), but the image is cropped to box =
    (x0, y0, xsize, ysize) of the oriented output image (None: the whole image) and resized, with the antialiased triangle
    filter of torch.nn.functional.interpolate(mode="bilinear", antialias=True), to the tensor's own height and width
    (jxlhip_set_output_resized). uint8 holds the undithered 8-bit sample."""
    if layout not in ("CHW", "HWC"):
        raise ValueError("layout is 'CHW' or 'HWC'")
    if tensor.dim() != 3 or not tensor.is_cuda or tensor.dtype not in _DTYPES:
        raise ValueError("a 3-d uint8 / float16 / bfloat16 / float32 tensor on the device")
    if box is not None and (len(box) != 4 or min(box) < 0 or box[2] == 0 or box[3] == 0):
        raise ValueError("box is (x0, y0, xsize, ysize) with non-zero extents, or None for the whole image")
    st = tensor.stride()
    sc, sy, sx = (st[0], st[1], st[2]) if layout == "CHW" else (st[2], st[0], st[1])
    channels = tensor.shape[0] if layout == "CHW" else tensor.shape[2]
    h, w = _image_size(tensor, layout)
    scale, bias = affine(mean, std, channels)
    if stream is None:
        stream = torch.cuda.current_stream(tensor.device)
    room = tensor.untyped_storage().nbytes() - tensor.storage_offset() * tensor.element_size()
    ctx.set_output_resized(tensor.data_ptr(), room, _DTYPES[tensor.dtype], channels, (sc, sy, sx), (w, h),
                           None if box is None else tuple(int(v) for v in box), scale, bias, clamp, getattr(stream, "cuda_stream", stream))
    ctx._bound_tensor = tensor  # keeps the memory alive while it is bound


def _upload_crop(c, f, out, layout, box, mean, std, clamp, channels, region):
    """The VarDCT upload of a crop: binds `out` as the resized output of `box` and uploads the frame; with `region` and a
    box, only the window of groups the box needs (the box translated into the window image). Returns the frame's group
    number of every group the context holds."""
    if region and box is not None:
        w = f.plan_window(box, channels)
        bind_resized(c, out, layout, w["box"], mean, std, clamp)
        c.upload_window(f, w)
        return w["groups"]
    bind_resized(c, out, layout, box, mean, std, clamp)
    c.upload(f)
    return list(range(f.info["num_groups"]))


def _alloc(shape_chw, dtype, layout, device):
    c, h, w = shape_chw
    return torch.empty((c, h, w) if layout == "CHW" else (h, w, c), dtype=dtype, device="cuda:%d" % device)


def _image_size(out, layout):
    return (out.shape[1], out.shape[2]) if layout == "CHW" else (out.shape[0], out.shape[1])


def _check_reduce(reduce):
    if reduce not in (1, 8):
        raise ValueError("reduce is 1 (the image) or 8 (its 1/8-scale DC image)")


def _decode_reduced(datas, outs, layout, mean, std, clamp, boxes, resized):
    """The reduced route of decode_to_tensor / decode_batch_to_tensor: frame i's 1/8-scale image into outs[i] (bound whole,
    or resized from boxes[i] of the reduced image), one kernel launch for the set. Every stream is parsed once; `outs` is a
    list, its entries tensors or callables (w, h) -> tensor, or one callable (the frames' reduced sizes) -> such a list. A
    stream the reduced parse refuses raises JxlAmdError with the parser's text: no fallback to a full decode."""
    frames, ctxs, made = [], [], []
    try:
        for d in datas:
            frames.append(J.Frame(d, reduced=True))
        if callable(outs):
            outs = outs([f.reduced_size() for f in frames])
        for i, f in enumerate(frames):
            w, h = f.reduced_size()
            o = outs[i](w, h) if callable(outs[i]) else outs[i]
            made.append(o)
            c = J.HipContext(o.device.index or 0)
            ctxs.append(c)
            if resized:
                bind_resized(c, o, layout, boxes[i], mean, std, clamp)
            else:
                if _image_size(o, layout) != (h, w):
                    raise ValueError("out is %r for a reduced image of %d x %d" % (tuple(o.shape), w, h))
                bind(c, o, layout, mean, std, clamp)
            c.upload_reduced(f)
        J.run_reduced_batch(ctxs)
        return made
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()


def decode_to_tensor(data, dtype=torch.float16, layout="CHW", mean=None, std=None, clamp=False, channels=3, device=0, out=None,
                     size=None, box=None, reduce=1, region=True):
    """One-shot: a VarDCT or Modular codestream's first frame -> a device tensor (allocated unless `out` is given).
    size = (height, width): the image, or box = (x0, y0, xsize, ysize) of it, is resized to that size on the device
    (bind_resized); an `out` given with it must have that size. Without `size` the tensor has the image's own size.
    reduce=8: from the frame's 1/8-scale DC image instead (VarDCT frames; `data` may be a prefix of frame_dc_extent(data)
    bytes): the tensor is (C, ceil(H / 8), ceil(W / 8)) without `size`, and `box` is in reduced-image coordinates.
    region=True: with `size` and `box`, a VarDCT frame decodes only the groups the box reads (the same tensor, bit for bit;
    a damaged section elsewhere in the frame is then not seen); region=False decodes the whole frame.
    Raises JxlAmdError on sections or streams the kernels flagged as corrupt."""
    if box is not None and size is None:
        raise ValueError("box needs size")
    _check_reduce(reduce)
    if reduce == 8:
        if size is not None:
            if out is None:
                out = _alloc((channels, int(size[0]), int(size[1])), dtype, layout, device)
            elif _image_size(out, layout) != (int(size[0]), int(size[1])):
                raise ValueError("out is %r for size %r" % (tuple(out.shape), tuple(size)))
            target = out
        else:
            target = out if out is not None else (lambda w, h: _alloc((channels, h, w), dtype, layout, device))
        return _decode_reduced([data], [target], layout, mean, std, clamp, [box], size is not None)[0]
    modular = J.frame_is_modular(data)
    f = J.ModFrame(data) if modular else J.Frame(data)
    c = J.HipContext(device)
    try:
        w, h = (f.info["xsize"], f.info["ysize"]) if modular else (f.info["out_xsize"], f.info["out_ysize"])
        if size is not None:
            if out is None:
                out = _alloc((channels, int(size[0]), int(size[1])), dtype, layout, device)
            elif _image_size(out, layout) != (int(size[0]), int(size[1])):
                raise ValueError("out is %r for size %r" % (tuple(out.shape), tuple(size)))
            if modular:
                bind_resized(c, out, layout, box, mean, std, clamp)
        else:
            if out is None:
                out = _alloc((channels, h, w), dtype, layout, device)
            elif _image_size(out, layout) != (h, w):
                raise ValueError("out is %r for an image of %d x %d" % (tuple(out.shape), w, h))
            bind(c, out, layout, mean, std, clamp)
        if modular:
            c.upload_modular(f)
            c.run_modular()
            r, status, _ = c.modular_status()
            if r:
                raise J.JxlAmdError("corrupt Modular streams: %r" % [(i, s) for i, s in enumerate(status) if s])
        else:
            if size is not None:
                groups = _upload_crop(c, f, out, layout, box, mean, std, clamp, channels, region)
            else:
                c.upload(f)
                groups = list(range(f.info["num_groups"]))
            c.run_all()
            r, flags = c.errors()
            if r:  # (frame group numbers: a window's groups are mapped back)
                raise J.JxlAmdError("corrupt AC sections: %r" % [(groups[g], e) for g, e in enumerate(flags) if e])
        return out
    finally:
        c.close()
        f.close()


def _decode_batch_resized(datas, out, dtype, mean, std, clamp, channels, device, size, boxes, region):
    """decode_batch_to_tensor with `size`: frames of any size, VarDCT and Modular mixed, each cropped to its box and resized
    into out[i]. The VarDCT contexts share the three batched stage launches, the Modular ones run_modular_batch; the resample
    passes are one launch pair per family."""
    n = len(datas)
    hh, ww = int(size[0]), int(size[1])
    if boxes is None:
        boxes = [None] * n
    if len(boxes) != n:
        raise ValueError("%d boxes for %d frames" % (len(boxes), n))
    if out is None:
        out = torch.empty((n, channels, hh, ww), dtype=dtype, device="cuda:%d" % device)
    elif tuple(out.shape) != (n, channels, hh, ww):
        raise ValueError("out is %r, size %r needs %r" % (tuple(out.shape), tuple(size), (n, channels, hh, ww)))
    modular = [J.frame_is_modular(d) for d in datas]
    frames, ctxs, groups = [], [], []
    try:
        for d, m in zip(datas, modular):
            frames.append(J.ModFrame(d) if m else J.Frame(d))
        for i, f in enumerate(frames):
            c = J.HipContext(device)
            ctxs.append(c)
            if modular[i]:
                bind_resized(c, out[i], "CHW", boxes[i], mean, std, clamp)
                c.upload_modular(f)
                groups.append(None)
            else:
                groups.append(_upload_crop(c, f, out[i], "CHW", boxes[i], mean, std, clamp, channels, region))
        var = [c for c, m in zip(ctxs, modular) if not m]
        mod = [c for c, m in zip(ctxs, modular) if m]
        if var:
            J.run_entropy_batch(var)
            J.run_transform_batch(var)
            J.run_filter_color_batch(var)
        if mod:
            J.run_modular_batch(mod)
        for i, c in enumerate(ctxs):
            if modular[i]:
                r, status, _ = c.modular_status()
                if r:
                    raise J.JxlAmdError("frame %d: corrupt Modular streams: %r" % (i, [(k, s) for k, s in enumerate(status) if s]))
            else:
                r, flags = c.errors()
                if r:
                    raise J.JxlAmdError("frame %d: corrupt AC sections: %r" % (i, [(groups[i][g], e) for g, e in enumerate(flags) if e]))
        return out
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()


def _decode_batch_reduced(datas, out, dtype, mean, std, clamp, channels, device, size, boxes):
    """decode_batch_to_tensor with reduce=8: without `size`, frames of one reduced size; with it, of any."""
    n = len(datas)
    if size is None and boxes is not None:
        raise ValueError("boxes needs size")
    if boxes is None:
        boxes = [None] * n
    if len(boxes) != n:
        raise ValueError("%d boxes for %d frames" % (len(boxes), n))
    batch = []

    def images(sizes):  # (called with the parsed frames' reduced sizes: the batch tensor, one image per frame)
        if size is None:
            if len(set(sizes)) != 1:
                raise ValueError("frames of one size: %r" % sorted(set(sizes)))
            shape = (n, channels, sizes[0][1], sizes[0][0])
        else:
            shape = (n, channels, int(size[0]), int(size[1]))
        if out is not None and tuple(out.shape) != shape:
            raise ValueError("out is %r, the frames need %r" % (tuple(out.shape), shape))
        batch.append(out if out is not None else torch.empty(shape, dtype=dtype, device="cuda:%d" % device))
        return [batch[0][i] for i in range(n)]

    _decode_reduced(datas, images, "CHW", mean, std, clamp, boxes, size is not None)
    return batch[0]


def decode_batch_to_tensor(datas, out=None, dtype=torch.float16, mean=None, std=None, clamp=False, channels=3, device=0, size=None,
                           boxes=None, reduce=1, region=True):
    """VarDCT frames of one size -> one (N, C, H, W) tensor: a context per frame, each bound to out[i], and one launch per
    stage for the whole set (run_entropy_batch / run_transform_batch / run_filter_color_batch). With size = (height, width)
    the frames may differ in size and kind (VarDCT, Modular); each is resized to that size, frame i cropped to boxes[i] first
    (a box (x0, y0, xsize, ysize) or None per frame). reduce=8: every frame's 1/8-scale DC image instead (VarDCT frames;
    datas[i] may be a prefix of frame_dc_extent bytes; boxes in reduced-image coordinates), one launch for the set.
    region=True: with `size`, a VarDCT frame that has a box decodes only the groups the box reads, as in decode_to_tensor."""
    _check_reduce(reduce)
    if reduce == 8:
        return _decode_batch_reduced(datas, out, dtype, mean, std, clamp, channels, device, size, boxes)
    if size is not None:
        return _decode_batch_resized(datas, out, dtype, mean, std, clamp, channels, device, size, boxes, region)
    if boxes is not None:
        raise ValueError("boxes needs size")
    frames = [J.Frame(d) for d in datas]
    ctxs = []
    try:
        sizes = {(f.info["out_xsize"], f.info["out_ysize"]) for f in frames}
        if len(sizes) != 1:
            raise ValueError("frames of one size: %r" % sorted(sizes))
        (w, h), = sizes
        if out is None:
            out = torch.empty((len(frames), channels, h, w), dtype=dtype, device="cuda:%d" % device)
        elif tuple(out.shape) != (len(frames), channels, h, w):
            raise ValueError("out is %r, the frames need %r" % (tuple(out.shape), (len(frames), channels, h, w)))
        for i, f in enumerate(frames):
            c = J.HipContext(device)
            ctxs.append(c)
            bind(c, out[i], "CHW", mean, std, clamp)
            c.upload(f)
        J.run_entropy_batch(ctxs)
        J.run_transform_batch(ctxs)
        J.run_filter_color_batch(ctxs)
        for i, c in enumerate(ctxs):
            r, flags = c.errors()
            if r:
                raise J.JxlAmdError("frame %d: corrupt AC sections: %r" % (i, [(g, e) for g, e in enumerate(flags) if e]))
        return out
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()
