"""Decode straight into torch tensors on the device (jxlhip_set_output_tensor): the writer kernels store every sample once,
in the layout and type the consumer asked for, into memory the consumer owns. torch is imported here only.

    img = torch_io.decode_to_tensor(data, dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    batch = torch_io.decode_batch_to_tensor(datas, dtype=torch.bfloat16)     # (N, 3, H, W), one launch per stage

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


def _alloc(shape_chw, dtype, layout, device):
    c, h, w = shape_chw
    return torch.empty((c, h, w) if layout == "CHW" else (h, w, c), dtype=dtype, device="cuda:%d" % device)


def _image_size(out, layout):
    return (out.shape[1], out.shape[2]) if layout == "CHW" else (out.shape[0], out.shape[1])


def decode_to_tensor(data, dtype=torch.float16, layout="CHW", mean=None, std=None, clamp=False, channels=3, device=0, out=None):
    """One-shot: a VarDCT or Modular codestream's first frame -> a device tensor (allocated unless `out` is given).
    Raises JxlAmdError on sections or streams the kernels flagged as corrupt."""
    modular = J.frame_is_modular(data)
    f = J.ModFrame(data) if modular else J.Frame(data)
    c = J.HipContext(device)
    try:
        w, h = (f.info["xsize"], f.info["ysize"]) if modular else (f.info["out_xsize"], f.info["out_ysize"])
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
            c.upload(f)
            c.run_all()
            r, flags = c.errors()
            if r:
                raise J.JxlAmdError("corrupt AC sections: %r" % [(g, e) for g, e in enumerate(flags) if e])
        return out
    finally:
        c.close()
        f.close()


def decode_batch_to_tensor(datas, out=None, dtype=torch.float16, mean=None, std=None, clamp=False, channels=3, device=0):
    """VarDCT frames of one size -> one (N, C, H, W) tensor: a context per frame, each bound to out[i], and one launch per
    stage for the whole set (run_entropy_batch / run_transform_batch / run_filter_color_batch)."""
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
