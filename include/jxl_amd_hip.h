/* libjxl_amd — thin extern "C" HIP layer for the JPEG XL VarDCT decode hot path on MI355X (gfx950).
 *
 * Plain C ABI: pointers and sizes only, no C++ or torch types. One JxlHipContext owns one HIP stream and the
 * device buffers of one frame; all calls on a context are asynchronous on its stream unless noted.
 *
 * This is the internal seam of the reference that the GPU path replaces:
 *   - jxlhip_run_entropy()      replaces the entropy half of DecodeGroup():
 *                               lib/jxl/dec_group.cc:469-542 (DecodeACVarBlock), :594-660 (GetBlockFromBitstream),
 *                               lib/jxl/dec_ans.h:170-257 (rANS + hybrid uint), lib/jxl/dec_bit_reader.h:84-144.
 *   - jxlhip_run_transform()    replaces the reconstruction half of DecodeGroupImpl():
 *                               lib/jxl/dec_group.cc:115-181 (dequant + chroma-from-luma), :433-450,
 *                               lib/jxl/dec_transforms-inl.h:456-818 (TransformToPixels, LowestFrequenciesFromDC),
 *                               lib/jxl/dct-inl.h:376-397.
 *   - jxlhip_run_filter_color() replaces RenderPipelineInput::Done() for the VarDCT stage list:
 *                               lib/jxl/render_pipeline/stage_gaborish.cc:56-100, stage_epf.cc:82-494,
 *                               stage_xyb.cc:80-92, stage_from_linear.cc:114-144, stage_write.cc:266-286,548-590,
 *                               low_memory_render_pipeline.cc:475-517 (edge mirroring).
 * The public drop-in boundary (JxlDecoder* / JxlParallelRunner) is declared in include/jxl/decode.h and
 * include/jxl/parallel_runner.h and is implemented on top of this layer.
 *
 * All functions return 0 on success, a negative hipError_t on a HIP failure, or a positive JXLHIP_ERR_* code.
 */
#ifndef JXL_AMD_HIP_H_
#define JXL_AMD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JXLHIP_ERR_INVALID_ARGUMENT 1
#define JXLHIP_ERR_NO_FRAME 2
#define JXLHIP_ERR_STREAM 3 /* the entropy kernel flagged a corrupt AC section; see jxlhip_get_errors */
#define JXLHIP_ERR_UNSUPPORTED 4
#define JXLHIP_ERR_GUARD 5 /* a test entry found a write outside the buffer it watches */

typedef struct JxlHipContext JxlHipContext;

/* One varblock in the decode order of its 256x256 group. */
typedef struct JxlHipVarBlock {
  uint16_t bx, by;      /* absolute position of the top-left 8x8 block */
  uint8_t strategy;     /* AcStrategy raw value 0..26 */
  uint8_t quant_dc_ctx; /* DC-derived bucket of the block context map */
  uint16_t qf;          /* raw quant field 1..256 */
  uint32_t coef_offset; /* offset of the block's coefficients in its group's per-channel plane */
} JxlHipVarBlock;

/* Entropy-code tables of one pass (rANS only). */
typedef struct JxlHipPassDesc {
  uint32_t log_alpha;
  uint32_t num_clusters;
  const uint8_t* ctx_map;     /* num_histograms * num_ac_contexts + 16 */
  uint32_t ctx_map_size;
  const void* alias;          /* num_clusters << log_alpha entries of 8 bytes:
                                 u8 cutoff, u8 right_value, u16 freq0, u16 offsets1, u16 freq1 */
  const uint32_t* uint_cfg;   /* per cluster: split_exponent | msb_in_token << 8 | lsb_in_token << 16 */
  const uint16_t* orders;     /* coefficient orders of the used (bucket, channel) pairs */
  uint32_t orders_size;
  uint32_t order_offset[39];  /* [bucket * 3 + channel] -> first entry in `orders` */
  uint32_t shift;             /* left shift applied to this pass's coefficients */
  /* Prefix-coded streams (dec_huffman.h:28-41; libjxl's fastest efforts) instead of rANS, as two-level lookup tables
   * (like the reference's own decoder, dec_huffman.cc): per cluster prefix_offset[cluster] = first entry of its root
   * table | root index bits R << 24 (R = min(8, longest code); 0 = one symbol, no bits). Root entry, indexed by the next
   * R bits of the stream (first bit = bit 0): code of <= R bits: symbol << 8 | code length; longer codes: (second-level
   * table, relative to the root's first entry) << 8 | 0x80 | S; second-level entry, indexed by the S bits after the
   * first R: symbol << 8 | total code length. alias / log_alpha are unused then. */
  uint32_t use_prefix;
  const uint32_t* prefix_table;
  uint32_t prefix_table_size;
  const uint32_t* prefix_offset;
  /* LZ77 (dec_ans.h:288-353): tokens >= lz_min_symbol start a copy of lz_min_length + hybrid(lz_len_cfg) earlier values at
   * a distance read with cluster lz_dist_ctx. lz_len_cfg is packed like uint_cfg. */
  uint32_t lz77, lz_min_symbol, lz_min_length, lz_len_cfg, lz_dist_ctx;
} JxlHipPassDesc;

/* The draw cache of a frame's splines: segments of 8 floats {centre x, centre y, maximum distance, 1 / sigma,
 * sigma / 4 * intensity, colour X, Y, B} (splines.h:44-51); row y draws segments row_segments[row_start[y] ..
 * row_start[y + 1]) in that order. num_segments = 0: no splines. */
typedef struct JxlHipSplines {
  uint32_t num_segments, num_row_segments;
  const float* segments;
  const uint32_t* row_start; /* ysize + 1 entries */
  const uint32_t* row_segments;
} JxlHipSplines;

/* The patches of a frame (lib/jxl/dec_patch_dictionary.cc): 8 u32 per position {x, y, xsize, ysize, x0 and y0 in the
 * reference frame, reference slot, PatchBlendMode of the colour channels (0 none, 1 replace, 2 add, 3 multiply) | clamp
 * << 8}; row y applies positions row_list[row_start[y] .. row_start[y + 1]) in that order. The reference frames are XYB
 * planes on the device ([3][slot_h][slot_w], from jxlhip_canvas_xyb_source). num_positions = 0: no patches. */
typedef struct JxlHipPatches {
  uint32_t num_positions, num_row_entries;
  const uint32_t* records;
  const uint32_t* row_start; /* ysize + 1 entries */
  const uint32_t* row_list;
  const float* slot_planes[4];
  uint32_t slot_w[4], slot_h[4];
  /* Patches that blend through alpha or change the alpha channel (PatchBlendMode 4..7: blend above / below, alpha-weighted
   * add above / below, dec_patch_dictionary.h:32-58; blending.cc:40-190), for images whose one extra channel is alpha:
   * records[7] also carries the alpha channel's own mode << 16 | its clamp << 24; uses_alpha != 0: some record needs the
   * alpha planes: slot_alpha[slot] = the reference frame's alpha, slot_h x slot_w floats on the device (jxlhip_canvas_xyb_alpha),
   * and the frame's own alpha plane must have been set (jxlhip_set_alpha) before the filter stage runs; the stage then leaves
   * the blended alpha for the pixel writer, the canvas and jxlhip_download_alpha. premultiplied = ExtraChannelInfo::
   * alpha_associated. Not on upsampled frames. Without uses_alpha modes 4 / 5 replace and 6 / 7 add (an image without alpha:
   * blending.cc:154-168). */
  uint32_t uses_alpha, premultiplied;
  const float* slot_alpha[4];
} JxlHipPatches;

typedef struct JxlHipColorTarget JxlHipColorTarget;
typedef struct JxlHipFrameDesc {
  uint32_t xsize, ysize;
  uint32_t xsize_blocks, ysize_blocks;
  uint32_t xsize_groups, num_groups;
  uint32_t num_passes;
  uint32_t coef_bits; /* 16 or 32: storage type of quantised coefficients */
  /* compressed AC sections; index pass * num_groups + group */
  const uint8_t* codestream;
  const uint64_t* section_offset;
  const uint32_t* section_size;
  uint32_t first_section_bit_offset; /* single-section frames only, else 0 */
  const JxlHipPassDesc* passes;
  /* varblocks */
  const JxlHipVarBlock* blocks;
  uint32_t num_blocks;
  const uint32_t* group_block_begin; /* num_groups + 1 */
  /* block context map */
  const uint8_t* block_ctx_lut; /* [c][order bucket][qf bucket][dc bucket] */
  uint32_t block_ctx_lut_size;
  uint32_t num_block_ctxs, num_dc_ctxs, num_qf_thresholds;
  uint32_t qf_thresholds[16];
  uint32_t num_histograms;
  /* dequantisation tables: for table kind k, channel c: dequant[dequant_offset[k] + c * dequant_size[k] + i] */
  const float* dequant;
  uint32_t dequant_floats;
  uint32_t dequant_offset[17], dequant_size[17];
  /* block-resolution planes */
  const float* dc;        /* 3 planes X, Y, B of xsize_blocks * ysize_blocks */
  const float* inv_sigma; /* xsize_blocks * ysize_blocks */
  const int8_t* ytox;     /* ceil(xsize_blocks / 8) * ceil(ysize_blocks / 8) */
  const int8_t* ytob;
  /* scalars */
  float inv_global_scale, x_dm, b_dm;
  float color_scale, base_corr_x, base_corr_b;
  float quant_biases[4];
  /* loop filter */
  int32_t gab;
  float gab_w[6]; /* per channel {w1, w2} */
  int32_t epf_iters;
  float epf_channel_scale[3];
  float epf_pass0_sigma_scale, epf_pass2_sigma_scale, epf_border_sad_mul;
  /* colour */
  float opsin_inv[9]; /* inverse opsin matrix, already scaled by 255 / intensity_target */
  float opsin_bias[3];
  /* the colour stage behind the filters: 0 = XYB -> linear sRGB -> sRGB transfer function, 1 = XYB -> linear sRGB;
   * frames of images that are not xyb_encoded (frame_header.h ColorTransform; dec_cache.cc:256-263): 2 = kYCbCr (full-range
   * BT.601, stage_ycbcr.cc:41-60: channels Cb, Y, Cr), 3 = kNone (the channels are the samples); no transfer function
   * follows either (the samples are in the image's own colour space) */
  int32_t linear_output;
  /* Band decode (one frame split over several GPUs by rows of 256x256 groups): produce only the pixel
   * rows of group rows [band_group_row_begin, band_group_row_end). The context then also decodes and transforms the
   * one group row above and below the band (the loop filters need up to 7 rows of their output), so no exchange
   * between devices is needed. 0, 0 = the whole frame. */
  uint32_t band_group_row_begin, band_group_row_end;
  /* Upsampling of the decoded frame by 2, 4 or 8 before the colour conversion (stage_upsampling.cc:49-282; 0 or 1 = none):
   * xsize / ysize above are the coded frame, out_xsize / out_ysize the image (in (factor * (frame - 1), factor * frame]),
   * upsampling_kernel the factor * factor 5x5 kernels, [factor * oy + ox][5 * (iy + 2) + ix + 2]. */
  uint32_t upsampling, out_xsize, out_ysize;
  const float* upsampling_kernel;
  /* Noise synthesis (frame flag kNoise; dec_noise.cc:43-164, render_pipeline/stage_noise.cc:64-310): has_noise != 0 adds
   * noise to the filtered X, Y, B before the colour conversion, strength from the pixel's intensity through the 8-point
   * LUT; the generators are seeded with the frame's visible / non-visible index and each 256x256 group's origin. Only
   * for frames that are not upsampled. */
  uint32_t has_noise;
  float noise_lut[8];
  uint32_t noise_frame_index[2];
  /* Splines (render_pipeline/stage_splines.cc; the draw cache of lib/jxl/splines.cc:661-768, built by the host): drawn
   * over the filtered planes before noise and colour conversion. Only for frames that are not upsampled. */
  JxlHipSplines splines;
  /* Patches: drawn over the filtered planes before the splines (dec_cache.cc:193-201). Not for upsampled frames. */
  JxlHipPatches patches;
  /* A frame whose bytes are not all there yet (JxlDecoderFlushImage; lib/jxl/dec_frame.cc:735-795 Flush): NULL, or one byte
   * per group, non-zero = the group's AC sections are missing. Such a group is not entropy-decoded (its section sizes must
   * be 0); its blocks are rendered from the DC image alone, as the reference draws them with zero passes. */
  const uint8_t* group_absent;
  /* The block-resolution stencils of the DC path on the device (lib/jxl/compressed_dc.cc:130-198 AdaptiveDCSmoothing,
   * lib/jxl/epf.cc:39-81 ComputeSigma), so that the host front-end does no per-block float work:
   *  dc_smoothing != 0: `dc` is the dequantised DC image BEFORE smoothing; the upload smooths it (dc_step = the DC
   *    quantisation step of X, Y, B, i.e. inv_global_scale / quant_dc * dc_quant[c]). 0: `dc` is used as it is (a caller
   *    that holds libjxl's own state passes its smoothed image, or the frame has kSkipAdaptiveDCSmoothing).
   *  inv_sigma == NULL and epf_iters > 0: 1 / sigma per block is computed by the upload from `sharpness` (one byte 0..7 per
   *    block, row-major like `dc`), the varblocks' qf, quant_scale (= global_scale / 65536), epf_quant_mul and epf_sharp_lut. */
  uint32_t dc_smoothing;
  float dc_step[3];
  /* DequantDC on the device (compressed_dc.cc:201-296): dc_quantised != NULL hands over the three coded integer planes
   * (X, Y, B; each xsize_blocks * ysize_blocks) instead of `dc` (which may then be NULL); the upload forms
   * Y = q_y * step_y, X = Y * dc_cfl_x + q_x * step_x, B = Y * dc_cfl_b + q_b * step_b with step = dc_step[c] / 2^e, e =
   * dc_extra_precision[DC group] (one byte per group of 256 x 256 blocks, row-major; NULL = 0). */
  const int32_t* dc_quantised;
  const uint8_t* dc_extra_precision;
  float dc_cfl_x, dc_cfl_b;
  /* kUseDcFrame (frame_header.h:348, passes_state.cc:62-77): the DC image is an earlier DC frame's output, resident on
   * this device as 3 planes of xsize_blocks * ysize_blocks floats (jxlhip_canvas_xyb_source of slot 4 + level); `dc` may
   * then be NULL and no smoothing runs. The planes must stay valid until the transform stage has run. */
  const float* dc_device;
  const uint8_t* sharpness;
  float quant_scale, epf_quant_mul;
  float epf_sharp_lut[8];
  /* Chroma subsampling of a YCbCr frame (frame_header.h:81-166 YCbCrChromaSubsampling; linear_output 2 only, else all 0):
   * channel c (Cb, Y, Cr) has (xsize_blocks >> chroma_hshift[c]) x (ysize_blocks >> chroma_vshift[c]) blocks, shifts 0 or 1.
   * Its block at (sx, sy) is coded with the varblock at (sx << hshift, sy << vshift) (dec_group.cc:568-578: the other
   * varblocks carry nothing for it), its DC samples (`dc_quantised` / `dc`) sit in the top-left part of its plane with the
   * plane's row stride, and DequantDC applies no chroma from luma (compressed_dc.cc:232-250). xsize_blocks / ysize_blocks
   * are then whole MCUs (multiples of 1 << the largest shift); only varblocks of one block, every group's in raster order
   * (the block context of a channel takes the quant field at the channel's own column, dec_group.cc:492); dc_smoothing must be 0
   * (dec_frame.cc:206-212). The decoded channel is upsampled in front of the loop filters
   * (render_pipeline/stage_chroma_upsampling.cc:29-111, dec_cache.cc:138-150). */
  uint8_t chroma_hshift[3], chroma_vshift[3];
  /* An XYB frame's output encoding when it is not (linear) sRGB or tone mapping applies (JxlHipColorTarget, below; copied by
   * the upload): NULL = none. linear_output must then be 1 and opsin_inv the target's matrix. */
  const struct JxlHipColorTarget* color_target;
} JxlHipFrameDesc;

int jxlhip_device_count(void);
int jxlhip_ctx_create(int device, JxlHipContext** ctx);
void jxlhip_ctx_destroy(JxlHipContext* ctx);

/* Copies every table and the AC sections of the frame to the device; everything the call keeps has been copied when it
 * returns (the host arrays may be released). Re-uses device buffers across frames when they fit. */
int jxlhip_frame_upload(JxlHipContext* ctx, const JxlHipFrameDesc* desc);

/* The three stages of the hot path. Inputs must be resident (jxlhip_frame_upload). */
int jxlhip_run_entropy(JxlHipContext* ctx);
int jxlhip_run_transform(JxlHipContext* ctx);
int jxlhip_run_filter_color(JxlHipContext* ctx);
/* Convenience: all three, in order. */
int jxlhip_run_all(JxlHipContext* ctx);
/* Entropy stage of `n` resident frames (contexts on one device) as ONE kernel launch on ctxs[0]'s stream, so that the
 * per-section serial decoders of all frames fill the machine together; the other contexts' streams are made to wait
 * for it. Stage time is then available from ctxs[0] (which == 0). Falls back to n separate launches when the frames
 * cannot share a launch. */
int jxlhip_run_entropy_batch(JxlHipContext* const* ctxs, size_t n);
/* Transform stage / filter+colour stage of `n` resident frames with one launch per kernel for the whole set (on
 * ctxs[0]'s stream; stage times from ctxs[0]). The frames must share the device and the coefficient storage type.
 * jxlhip_run_transform(ctx) and jxlhip_run_filter_color(ctx) are the n = 1 case. */
int jxlhip_run_transform_batch(JxlHipContext* const* ctxs, size_t n);
int jxlhip_run_filter_color_batch(JxlHipContext* const* ctxs, size_t n);

/* Blocks until the context's stream is idle. */
int jxlhip_sync(JxlHipContext* ctx);

/* Copies the interleaved RGB8 result (row stride in bytes) to host memory; synchronous. The result has the frame's
 * size, or out_xsize x out_ysize for an upsampled frame. */
int jxlhip_download_rgb8(JxlHipContext* ctx, uint8_t* dst, size_t stride);
/* Output pixel format of the filter + colour stage (reference render_pipeline/stage_write.cc:266-286,334-370,548-590;
 * call before jxlhip_frame_upload; default RGB8). data_type uses the JxlDataType values (0 = f32, 2 = u8, 3 = u16,
 * 5 = f16), num_channels 1..4 (2 and 4 carry alpha: jxlhip_set_alpha, else opaque), bits_per_sample the depth of the
 * unsigned types (0 = full width), big_endian swaps the bytes of multi-byte samples. RGB8 is written by every filter
 * kernel, RGB f32 and one 8-bit sRGB channel (channel 0: the pixel of a grey image) by the row-streaming one (the d1.0
 * configuration); other formats cost one more pass over the planes. */
int jxlhip_set_output_format(JxlHipContext* ctx, uint32_t data_type, uint32_t num_channels, uint32_t bits_per_sample, int big_endian);
/* The pixels are written with the image's orientation undone (JxlOrientation / EXIF numbering 1..8; 1 = as coded), the
 * way the reference's write stage does it (render_pipeline/stage_write.cc:292-306,441-458,664-699): for 5..8 the rows
 * of the output are columns of the image (jxlhip_download_pixels then hands out xsize rows of ysize pixels). Call before
 * the upload. */
int jxlhip_set_output_orientation(JxlHipContext* ctx, uint32_t orientation);
/* 2- and 4-channel output: the colour samples are divided by max(alpha, 2^-26) as they are written, after the transfer
 * function (what JxlDecoderSetUnpremultiplyAlpha asks of an image whose alpha is associated:
 * render_pipeline/stage_write.cc:359-361,460-482, dec_frame.h:209-211). Call before the upload; 0 = off (the default). */
int jxlhip_set_output_unpremultiply(JxlHipContext* ctx, int on);
/* Alpha plane of the image (f32 in [0, 1], xsize * ysize, host memory; copied synchronously) for 2- and 4-channel output;
 * NULL = opaque again. */
int jxlhip_set_alpha(JxlHipContext* ctx, const float* alpha, uint32_t xsize, uint32_t ysize);
/* An extra channel that is coded smaller than the image (JxlHipFrameDesc-independent; dec_cache.cc:172-190, 203-212: the
 * upsampling stage, stage_upsampling.cc:49-282, on that one channel): `plane` = xsize * ysize floats in host memory, `kernels`
 * = factor * factor * 25 weights (factor 2, 4 or 8), the result out_xsize x out_ysize with out in (factor * (size - 1),
 * factor * size]. as_alpha != 0: the result becomes the context's alpha plane (as after jxlhip_set_alpha); host_out != NULL:
 * it is copied there (out_xsize * out_ysize floats). Synchronous. */
/* The context's alpha plane as the filter stage left it (the patches of the frame may have blended into it), out_xsize *
 * out_ysize floats to host memory; synchronous. */
int jxlhip_download_alpha(JxlHipContext* ctx, float* dst);
int jxlhip_upsample_plane(JxlHipContext* ctx, const float* plane, uint32_t xsize, uint32_t ysize, uint32_t factor, const float* kernels,
                          uint32_t out_xsize, uint32_t out_ysize, int as_alpha, float* host_out);
/* Copies the interleaved result in the format of jxlhip_set_output_format (row stride in bytes); synchronous. */
int jxlhip_download_pixels(JxlHipContext* ctx, void* dst, size_t stride);
/* Same for pixel rows [y_begin, y_end) only (dst receives y_end - y_begin rows): the rows a band context produced. */
int jxlhip_download_rgb8_rows(JxlHipContext* ctx, uint8_t* dst, size_t stride, uint32_t y_begin, uint32_t y_end);
/* Device pointer of the RGB8 result (xsize * 3 bytes per row, tightly packed). */
const uint8_t* jxlhip_rgb8_device_ptr(JxlHipContext* ctx);

/* ---- Output into device memory the caller owns (a tensor of the framework that consumes the image), instead of the
 * context's own interleaved buffer. Element (c, y, x) of the OUTPUT image (after jxlhip_set_output_orientation) goes to
 * data[c * stride_c + y * stride_y + x * stride_x], strides in elements: planar (CHW), interleaved (HWC), padded pitches
 * and one image of an NCHW batch are all this map. The library never writes outside [data, data + bytes).
 *   v = the float the f32 writer of jxlhip_set_output_format(ctx, 0, num_channels, 0, 0) stores for the same frame and
 *       options (alpha as the last of 2 / 4 channels, un-premultiplication, R for 1 / 2 channels of a colour image).
 *   Float types: v = fmin(fmax(v, 0), 1) first when clamp01 is set (a NaN becomes 0); then t = v * scale[c] rounded to
 *       float, then t + bias[c] rounded to float (two operations, never a fused one), then round-to-nearest-even to dtype.
 *   JXLHIP_TENSOR_U8: scale 1, bias 0 and clamp01 0 only; the sample is the 8-bit sample of the generic writer (v * 255
 *       plus the dither cell of interleave index c at the oriented position, each rounded; clamped; nearest even).
 * While a tensor is bound the context allocates no pixel buffer, jxlhip_download_pixels / _rgb8 / _rgb8_rows answer
 * JXLHIP_ERR_INVALID_ARGUMENT and jxlhip_rgb8_device_ptr NULL, band uploads and the jxlhip_canvas_* calls that take the
 * context answer JXLHIP_ERR_UNSUPPORTED, and jxlhip_set_output_format is not consulted. Call before the upload, which checks
 * the descriptor again against the image's size (a refused one launches nothing). NULL: the context's own buffer again.
 * A context that is destroyed drops its binding.
 * Ordering, without any host wait: the first launch that writes the tensor waits for what consumer_stream holds at that
 * call (the consumer's earlier fill or read of the tensor), and consumer_stream waits for the last such launch of the
 * call (jxlhip_run_filter_color[_batch], jxlhip_modular_run[_batch]; in a batch every context's own consumer_stream).
 * With a float dtype, three channels, stride_x 1 and no orientation, a frame that would get RGB f32 from the row-streaming
 * filter kernel gets the tensor from that kernel too (jxlhip_debug_pixel_route: 3); everything else goes through the
 * generic writer. */
#define JXLHIP_TENSOR_F32 0u
#define JXLHIP_TENSOR_U8 2u
#define JXLHIP_TENSOR_F16 5u
#define JXLHIP_TENSOR_BF16 6u
typedef struct {
  void* data;                         /* device memory on the context's device */
  size_t bytes;                       /* room behind data */
  uint32_t dtype;                     /* JXLHIP_TENSOR_* */
  uint32_t num_channels;              /* 1..4, as jxlhip_set_output_format's */
  int64_t stride_c, stride_y, stride_x; /* in elements, > 0 */
  float scale[4], bias[4];
  uint32_t clamp01;
  void* consumer_stream;              /* hipStream_t (0 = the null stream) */
} JxlHipTensorOut;
int jxlhip_set_output_tensor(JxlHipContext* ctx, const JxlHipTensorOut* tensor);

/* ---- The same, cropped and resized on the way: a box of the oriented output image, resampled to out_xsize x out_ysize,
 * goes to the caller's tensor, whose extents are the OUTPUT size (every rule of JxlHipTensorOut holds at that size).
 *   Source sample v: as above, the float the f32 writer of jxlhip_set_output_format(ctx, 0, num_channels, 0, 0) stores.
 *   Filter: the separable antialiased triangle filter of the box alone (samples outside the box do not exist, as if the
 *       image had been cropped first). Per axis, n_in the box extent and n_out the output extent, in double on the host:
 *         scale = n_in / n_out, support = max(scale, 1), center = scale * (i + 0.5),
 *         lo = max(0, trunc(center - support + 0.5)), hi = min(n_in, trunc(center + support + 0.5)),
 *         w_j = max(0, 1 - |(j - center + 0.5) / support|) for j in [lo, hi), divided by their sum, then rounded to float:
 *       torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) of the cropped image in
 *       float64, and Pillow's rule. The kernels accumulate in float32 (two passes, a float32 value between them).
 *   Float types: then the arithmetic of jxlhip_set_output_tensor (clamp01, * scale[c], + bias[c], each rounded; to dtype).
 *   JXLHIP_TENSOR_U8: scale 1, bias 0, no clamp; the sample is v * 255 rounded to float, clamped to [0, 255], rounded to
 *       nearest even. NO dither: a dither cell has no meaning at a resampled position.
 * While the binding is set the context renders as for jxlhip_set_output_format(ctx, 0, num_channels, 0, 0) into a pixel
 * buffer of its own, which stays private: jxlhip_download_pixels / _rgb8 / _rgb8_rows answer JXLHIP_ERR_INVALID_ARGUMENT and
 * jxlhip_rgb8_device_ptr NULL, band uploads and the jxlhip_canvas_* calls JXLHIP_ERR_UNSUPPORTED, as for a bound tensor.
 * The two resample launches are the tail of jxlhip_run_filter_color[_batch] / jxlhip_modular_run[_batch] (one launch per
 * pass for all the contexts of a batch that have such a binding), inside the ordering described above. Setting this
 * binding clears a bound tensor and the other way round; a destroyed context drops it. The upload checks the descriptor
 * again at the image's size (a refused one launches nothing). NULL: unbound. Output extents up to 16384. */
#define JXLHIP_RESAMPLE_TRIANGLE 0u
typedef struct {
  JxlHipTensorOut tensor;                          /* extents: out_xsize x out_ysize */
  uint32_t out_xsize, out_ysize;
  uint32_t box_x0, box_y0, box_xsize, box_ysize;   /* in the oriented output image; all 0: the whole image */
  uint32_t filter;                                 /* JXLHIP_RESAMPLE_TRIANGLE */
} JxlHipResizedOut;
int jxlhip_set_output_resized(JxlHipContext* ctx, const JxlHipResizedOut* out);

/* Per-group error flags written by the entropy kernel: bit0 invalid nzeros, bit1 ANS final state,
 * bit2 section over-read, bit3 invalid histogram selector. Synchronous. `flags` has num_groups entries.
 * Returns JXLHIP_ERR_STREAM if any flag is set. */
int jxlhip_get_errors(JxlHipContext* ctx, uint32_t* flags, size_t n);

/* Where every AC section's coefficient stream ended: bits[pass * num_groups + group] = bit position from the section's
 * first byte (after the entropy stage; synchronous). Sections of frames with extra channels carry Modular data behind
 * the coefficients (reference dec_frame.cc:511-542), which the host front-end decodes from there. */
int jxlhip_get_section_end_bits(JxlHipContext* ctx, uint32_t* bits, size_t n);

/* Test/debug access to intermediates; synchronous copies to host.
 *   "coeffs"       quantised coefficients, int16 or int32 [num_groups][3][65536]
 *   "xyb_idct"     float [3][ysize_padded][xsize_padded] after the inverse transforms
 *   "xyb_filtered" float [3][ysize_padded][xsize_padded] after Gaborish/EPF (rows < ysize, columns < xsize valid;
 *                  only with option "keep_filtered")
 *   "xyb_upsampled" float [3][out_ysize][out_xsize padded to 8] of an upsampled frame, behind the upsampling and the noise
 *                  (only with option "keep_upsampled")
 *   "kend"         uint32 [num_blocks][3]: scan position after the last non-zero coefficient of a (varblock, channel);
 *                  frames decoded in scan order only (after the entropy stage)
 *   "transform_lists" uint32 [entries][2] = {strategy, varblock index}: the transform work lists in launch order
 *   "dc"           float [3][ysize_blocks][xsize_blocks]: the DC image after smoothing, as the transform stage reads it; of a
 *                  reduced upload (jxlhip_reduced_upload) after its run, only with option "keep_dc"
 *   "inv_sigma"    float [ysize_blocks][xsize_blocks]: 1 / sigma of the EPF per block
 * Returns the number of bytes the buffer needs through *needed when dst is NULL. */
int jxlhip_download(JxlHipContext* ctx, const char* name, void* dst, size_t dst_size, size_t* needed);

/* Options (set before jxlhip_frame_upload): "keep_filtered" = 1 makes jxlhip_run_filter_color also store the filtered
 * XYB planes for jxlhip_download("xyb_filtered") (test aid; costs one extra plane set and 12 B/pixel of writes). Switched
 * on only after the upload of a frame that writes one 8-bit channel from the filter kernel (rows of 1 byte per pixel,
 * which no other writer may fill), it makes the filter launch fail with JXLHIP_ERR_INVALID_ARGUMENT: upload again.
 * "keep_upsampled" = 1 (test aid): an upsampled frame takes the route a noisy upsampled frame takes (k_upsample_color
 * writes X, Y, B at the image's size, then k_color_out makes the pixels) and keeps those planes for
 * jxlhip_download("xyb_upsampled"). Off: launches and jxlhip_debug_pixel_route are as they were.
 * "transform_dense" = 1 (test aid): the transform kernels treat every coefficient extent as full, i.e. take none of the
 * shortcuts they decide from the coefficient counts. The same kernels, the same results.
 * "filter_async" = 1 (on the FIRST context of a set; may be changed at any time): jxlhip_run_filter_color_batch launches
 * on that context's second stream, ordered after the work its first stream holds. The call sequence entropy_batch,
 * transform_batch, filter_color_batch, entropy_batch, ... on one frame set then overlaps every filter + colour launch
 * with the next entropy launch (which touches neither planes nor pixels): the LDS-hungry entropy and transform kernels
 * never share the GPU, the LDS-free filter fills the gaps of the latency-bound entropy kernel. The library keeps the
 * order: the next transform, upload, download or sync of any frame of the set waits for the filter launch.
 * "entropy_gate" = 1 on the FIRST context of a frame set, for callers that keep a set's batched entropy launch and other
 * sets' batched transform / filter launches in flight together: the entropy launch must get the machine first (its few,
 * LDS-heavy workgroups find no room behind a stream of small ones: 133 ms instead of 62), so the transform / filter
 * launches enqueued after it wait ON THE DEVICE (hipStreamWaitValue64) until its workgroups are resident. The wait has no
 * bound, hence off by default, and the library ignores the option when the runtime may run kernels one at a time
 * (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING, GPU_MAX_HW_QUEUES=1, counter collection by rocprofv3).
 * "keep_dc" = 1 (test aid; takes effect at the next jxlhip_reduced_upload): k_reduced_pixels also stores its smoothed DC
 * planes for jxlhip_download("dc").
 * "blocking_sync" = 1 (process-wide for the context's device): host threads that wait for the device sleep instead of
 * spinning; for servers that pipeline frames over more host threads than they have CPUs to spare. */
int jxlhip_set_option(JxlHipContext* ctx, const char* name, int value);

/* ---- Bands of one frame on several devices (multi-GPU split of very large frames; replaces nothing in the reference,
 * whose LowMemoryRenderPipeline keeps the rows between groups in one address space: low_memory_render_pipeline.cc:475-517).
 * jxlhip_set_option(ctx, "band_halo", 1) before the upload of a band: the context entropy-decodes and transforms ONLY the
 * band's own rows of groups; the rows of the neighbouring bands that its filters read (jxlhip_halo_rows: Gaborish 1,
 * EPF 2 / 3 / 6 more) are exchanged after the transform stage: the neighbour packs them (side 0 = its first rows,
 * side 1 = its last rows) into a dense [3][rows][padded xsize] f32 block of DEVICE memory, any device-to-device transport
 * (hipMemcpyPeerAsync, an RCCL send / recv) moves the block, and jxlhip_halo_unpack writes it beside the band (side 0 =
 * above it, side 1 = below it). Both calls run behind the context's transform stage and are complete when they return
 * (one host synchronisation per call); the filter stage follows them.
 * The _batch forms take every frame of a set (the contexts of one jxlhip_run_transform_batch call, in that order; block i
 * of `block_bytes` bytes at `device + i * block_bytes`) and never block the host: `transport_stream` is the hipStream_t the
 * caller's transport is enqueued on (for torch.distributed over RCCL: torch's current stream, which c10d orders its
 * communication stream against). pack: the copies follow the set's transform launch, and everything enqueued on
 * transport_stream after the call follows the copies. unpack: the copies follow everything enqueued on transport_stream
 * BEFORE the call (the receive), the set's filter launch follows the copies, and work enqueued on transport_stream after
 * the call (re-use of the blocks) follows them too. */
int jxlhip_halo_rows(JxlHipContext* ctx, uint32_t* rows);
int jxlhip_halo_pack(JxlHipContext* ctx, int side, void* dst_device, size_t dst_bytes);
int jxlhip_halo_unpack(JxlHipContext* ctx, int side, const void* src_device, size_t src_bytes);
int jxlhip_halo_pack_batch(JxlHipContext* const* ctxs, size_t n, int side, void* dst_device, size_t block_bytes, void* transport_stream);
int jxlhip_halo_unpack_batch(JxlHipContext* const* ctxs, size_t n, int side, const void* src_device, size_t block_bytes,
                             void* transport_stream);

/* Test entry: runs the colour stage alone (XYB -> linear RGB -> sRGB transfer function unless linear_output) on n
 * XYB triples, planar [3][n], with the opsin parameters of the frame the context last uploaded; interleaved f32 RGB out.
 * For the reference's closed-form colour tests (lib/jxl/opsin_image_test.cc) against the kernel itself. */
int jxlhip_debug_color(JxlHipContext* ctx, const float* xyb, size_t n, int linear_output, float* rgb);

/* ---- Output colour encodings of XYB images other than (linear) sRGB (lib/jxl/dec_xyb.cc:127-250,
 * render_pipeline/stage_tone_mapping.cc:30-120, stage_from_linear.cc:37-168). The host builds the description
 * (jxlamd_color_output in jxl_amd.h); the primaries and white point live in `matrix`, which replaces the frame's
 * opsin_inv. A target whose transfer function is sRGB or linear and that needs no tone mapping is the matrix alone
 * (tf = JXLHIP_TF_NONE: the frame keeps the filter kernels' own colour stage); any other makes the filter leave the
 * filtered XYB planes and the generic writer (k_color_out, k_upsample_color, k_modular_output) compute, per pixel:
 * matrix -> tone mapping -> transfer function. */
#define JXLHIP_TF_NONE 0   /* the frame's linear_output decides (sRGB curve or none) */
#define JXLHIP_TF_LINEAR 1
#define JXLHIP_TF_SRGB 2
#define JXLHIP_TF_PQ 3     /* SMPTE ST 2084, 1.0 = pq_display_scale * 10000 cd/m2 */
#define JXLHIP_TF_HLG 4    /* BT.2100 HLG, after the scene-light OOTF of hlg_exponent */
#define JXLHIP_TF_709 5
#define JXLHIP_TF_GAMMA 6  /* x^inv_gamma, values <= 1e-5 to 0 (DCI: inv_gamma = 1 / 2.6) */
#define JXLHIP_TONE_NONE 0
#define JXLHIP_TONE_REC2408 1  /* Rec2408ToneMapper, then GamutMap (cms/tone_mapping.h:23-113, tone_mapping-inl.h) */
#define JXLHIP_TONE_HLG_OOTF 2 /* HlgOOTF from the image's intensity target to the desired one; GamutMap when gamut_map */
struct JxlHipColorTarget {
  float matrix[9];         /* the inverse opsin matrix towards the target primaries, scaled by 255 / intensity target */
  uint32_t tf, tone, gamut_map;
  float luminances[3];     /* Y row of the target primaries' RGB -> XYZ matrix (dec_xyb.cc:212) */
  float pre_scale, post_scale; /* around the tone mapping: 10000 / orig and desired / 10000 for a PQ target, else 1 */
  float pq_display_scale;  /* TF_PQ(orig_intensity_target): display intensity / 10000 */
  float inv_gamma;         /* JXLHIP_TF_GAMMA */
  float hlg_exponent;      /* JXLHIP_TF_HLG: HlgOOTF::ToSceneLight(desired) exponent; 0 = no OOTF */
  float tone_exponent;     /* JXLHIP_TONE_HLG_OOTF exponent (gamma - 1) */
  /* JXLHIP_TONE_REC2408: Rec2408ToneMapperBase's constants (cms/tone_mapping.h:87-111) */
  float tm_source_peak, tm_target_peak, tm_pq_min, tm_pq_range, tm_inv_pq_range, tm_min_lum, tm_max_lum, tm_ks,
      tm_inv_one_minus_ks, tm_normalizer, tm_inv_target_peak;
};
/* Test entry: the generic writer's colour stage alone on n XYB triples (planar [3][n]) with `target` (its matrix; the
 * opsin biases of the frame the context last uploaded); interleaved f32 RGB out. */
int jxlhip_debug_color_target(JxlHipContext* ctx, const float* xyb, size_t n, const JxlHipColorTarget* target, float* rgb);

/* Test entry: noise synthesis alone (k_noise_random, then k_noise_add on rows [y_begin, y_end)) on caller-supplied planes:
 * xyb / xyb_out = [3][ysize][xsize] floats, dense, in host memory (rows outside the band come back as they went in);
 * seed0 / seed1 = the visible / non-visible frame index; lut = the 8 strengths; ytox / ytob = the base colour
 * correlation; raw_out (may be NULL) = the three random planes in front of the high-pass, same layout. Refuses empty or
 * oversized planes (more than 2^24 samples), an empty or outlying band and values that are not finite. */
int jxlhip_debug_noise(JxlHipContext* ctx, const float* xyb, uint32_t xsize, uint32_t ysize, uint32_t seed0, uint32_t seed1,
                       const float* lut, float ytox, float ytob, uint32_t y_begin, uint32_t y_end, float* raw_out, float* xyb_out);

/* Test entry: the two resample passes alone (k_resample_rows, then k_resample_columns) on `src`, host memory, interleaved
 * [ysize][xsize][nc] floats, into the descriptor's tensor, ordered against its consumer_stream as a decode is; complete
 * when it returns. Refuses whatever the descriptor's check refuses for an image of xsize x ysize, an nc that is not the
 * tensor's num_channels, and sources of more than 2^26 samples, before any launch. */
int jxlhip_debug_resample(JxlHipContext* ctx, const float* src, uint32_t xsize, uint32_t ysize, uint32_t nc, const JxlHipResizedOut* out);

/* Test access: who writes the pixels of the VarDCT frame the context last uploaded. *route = 0: the generic writer behind
 * the filter kernel (k_color_out / k_upsample_color), 1: the filter kernel itself (RGB8, RGB f32), 2: the one-channel
 * 8-bit form of the row-streaming filter kernel (k_filter_rows2<true, EPF, GAB, true>), 3: its tensor form
 * (k_filter_rows2<false, EPF, GAB, false, true>, jxlhip_set_output_tensor). */
int jxlhip_debug_pixel_route(JxlHipContext* ctx, uint32_t* route);
/* Test access: which kernel jxlhip_run_entropy launches for the VarDCT frame the context last uploaded. *route = 0:
 * k_entropy_lanes (the frame is kept in scan order when it has one pass), 1: k_entropy_uni, 2: k_entropy_ans (alias tables
 * beyond the LDS budget, read in place), 3: k_entropy_generic (prefix codes and / or LZ77). */
int jxlhip_debug_entropy_route(JxlHipContext* ctx, uint32_t* route);
/* Test access: the order in which the lane kernel's workgroups of the batch last prepared on `ctx0` (the first context of a
 * jxlhip_run_entropy_batch call) are dispatched. wg_unit[p] = the unit (sections of one frame that share a histogram set,
 * numbered in frame order) of the p-th workgroup, est[p] = that unit's estimated length (1/16 token; longest first unless
 * JXLHIP_WG_ORDER says otherwise). `n` is the room in both arrays, at least the batch's workgroups; the entries past them
 * are set to 0xFFFFFFFF / 0. */
int jxlhip_debug_entropy_order(JxlHipContext* ctx0, uint32_t* wg_unit, uint64_t* est, size_t n);
/* Measurement aid: the per-wave records of a lane-kernel launch made on `ctx0` under JXLHIP_LANES_PROF=2 (records are kept,
 * not printed, and the launch is not waited for): eight uint64 per workgroup, [1] and [7] = the wave's first and last
 * instruction on the clock all XCDs share (100 MHz), [6] = HW_ID | XCC_ID << 32. `back` = 0 is the last launch, 1 the one
 * before it, ... up to 7. Waits for the stream. *workgroups = the launch's
 * workgroups; `records` (may be NULL) has room for `n` of them. */
int jxlhip_debug_entropy_timeline(JxlHipContext* ctx0, uint32_t back, uint64_t* records, size_t n, size_t* workgroups);

/* Debug aid: with JXLHIP_GUARD=1 in the environment every device buffer of a context is allocated with a 4 KiB guard
 * band either side, filled with a pattern. Waits for the device, then *touched = 0 when every band is intact, else
 * (1-based buffer index << 2) | (1 = band before, 2 = band after) of the first buffer a kernel wrote next to. */
int jxlhip_check_guards(JxlHipContext* ctx, uint32_t* touched);

/* Memory sharing for pipelined frame sets (call before jxlhip_frame_upload): `ctx` keeps its inverse-transform output (the
 * 3 f32 XYB planes, 12 B/pixel: the largest buffer of a context) in `lender`'s plane buffer instead of allocating its
 * own; lender = NULL undoes it. The planes only live between a frame's transform and its filter + colour stage, so
 * frames whose downstream stages never run at the same time (e.g. the two frame sets of a software pipeline: one set is
 * in the entropy stage while the other is transformed and filtered) can share them. The library orders the launches: a
 * transform that overwrites shared planes waits for the filter launch that last read them, also across streams. The
 * lender must have uploaded a frame at least as large and must outlive the borrower's use. */
int jxlhip_share_planes(JxlHipContext* ctx, JxlHipContext* lender);

/* ---- Modular (lossless) frames: reference lib/jxl/dec_modular.cc:209-425,564-793, modular/encoding/encoding.cc:148-724,
 * modular/transform/{rct,palette,squeeze}.cc. The host front-end parses headers, trees and histograms and every stream's
 * group header; the sample decode, the inverse transforms and the conversion to output samples run on the device. ---- */
typedef struct JxlHipModTreeNode {  /* MA tree node (dec_ma.cc:107-159); property -1 = leaf */
  int32_t property, splitval;
  uint32_t lchild, rchild; /* leaves: lchild = context */
  uint32_t predictor;
  int32_t offset;
  uint32_t multiplier, pad;
} JxlHipModTreeNode;
typedef struct JxlHipModCode {  /* one entropy code: the global one or a stream's own */
  const uint8_t* ctx_map;
  uint32_t ctx_map_size, num_clusters;
  uint32_t use_prefix, log_alpha;
  const void* alias;             /* ANS: num_clusters << log_alpha entries of 8 bytes (as JxlHipPassDesc::alias) */
  const uint32_t* uint_cfg;      /* per cluster */
  const uint32_t* prefix_table;  /* prefix codes: as JxlHipPassDesc */
  uint32_t prefix_table_size;
  const uint32_t* prefix_offset;
  uint32_t lz77, lz_min_symbol, lz_min_length, lz_len_cfg, lz_dist_ctx;
} JxlHipModCode;
typedef struct JxlHipModRect {  /* a stream's channel: rectangle of channel buffer `buffer` */
  uint32_t buffer, x0, y0, w, h, sig;
} JxlHipModRect;
typedef struct JxlHipModStream {
  uint32_t section;      /* index into the frame's section list */
  uint32_t bit_offset;   /* sample data start, from the section's first byte */
  uint32_t stream_id, first_channel_index;
  uint32_t tree, code;   /* indices into trees / codes */
  uint32_t first_rect, num_rects;
  int32_t wp[11];
  uint32_t uses_wp, num_props, dist_multiplier, max_width, num_samples;
} JxlHipModStream;
typedef struct JxlHipModBuffer {  /* a channel buffer: w x h int32 samples (the device pool is laid out by the library) */
  uint32_t w, h;
} JxlHipModBuffer;
typedef struct JxlHipModOp {  /* one inverse-transform step */
  uint32_t kind;          /* 0 = RCT, 1 = palette lookup, 2 = horizontal unsqueeze, 3 = vertical unsqueeze */
  uint32_t buf[6];        /* RCT: 3 channels; palette: palette, index, outputs (buf[2..]); unsqueeze: averages, residuals, output */
  uint32_t ox[6], oy[6];  /* per buffer: where its rectangle starts (whole channels: 0, 0; the palette itself is always whole) */
  uint32_t w, h;          /* RCT, palette: the rectangle of every channel; unsqueeze: the OUTPUT rectangle, the averages are
                             (n + 1) / 2 and the residuals n / 2 samples along the step's direction, n = w or h */
  uint32_t param, nb, bit_depth;  /* RCT type / palette width; palette channels, sample depth */
  /* Schedule. local = 1: the operation undoes a transform of one group stream (group-sized rectangles, private
   * buffers); all local operations of a set of frames run before any other, those of one `level` and kind in ONE launch,
   * so operations that share a level must not touch overlapping samples. local = 0: the frame's own transforms, one
   * level per list entry, after the deepest local level.
   * What jxlhip_modular_upload checks is stated rule by rule in enum ModRule (libjxl_amd/csrc/host/jxh_modular_upload_plan.h:
   * kModRuleOpFields .. kModRuleUnsqueezeAlias for operations): every rectangle lies inside its buffer and an unsqueeze
   * output is not one of its inputs, so no operation reads or writes outside the pool. It does NOT check the schedule: that
   * operations sharing a level are disjoint, or that palette outputs 1.. do not alias the index rectangle. A description
   * that breaks this decodes to wrong samples (a race), not to an error. */
  uint32_t level, local;
} JxlHipModOp;
typedef struct JxlHipModFrameDesc {
  uint32_t xsize, ysize;
  const uint8_t* codestream;
  const uint64_t* section_offset;
  const uint32_t* section_size;
  uint32_t num_sections;
  const JxlHipModTreeNode* const* trees;
  const uint32_t* tree_size;
  uint32_t num_trees;
  const JxlHipModCode* codes;
  uint32_t num_codes;
  const JxlHipModBuffer* buffers;
  uint32_t num_buffers;
  const JxlHipModRect* rects;
  uint32_t num_rects;
  const JxlHipModStream* streams;
  uint32_t num_streams;
  const JxlHipModOp* ops;
  uint32_t num_ops;
  /* output: the buffers holding the final colour channels (1 or 3) and alpha (or 0xFFFFFFFF) */
  uint32_t out_buffer[4];
  /* bits: low byte = bits per colour sample (integers: 1..31), bits 8..15 = exponent bits when the samples are floats of
   * that width (0 = integers; image_metadata.cc BitDepth, dec_modular.cc:128-185); alpha_bits: integer alpha, 1..24 */
  uint32_t num_color, has_alpha, bits, alpha_bits;
  /* splines over the three colour channels (as floats, before the sample conversion); colour images only */
  JxlHipSplines splines;
  /* patches over the three colour channels, before the splines (dec_cache.cc:193-201), from the reference slots' planes; colour
   * images only; not the modes that blend through the frame's alpha channel (uses_alpha must be 0) */
  JxlHipPatches patches;
  /* XYB Modular frames (dec_modular.cc:583-631): the colour buffers hold Y, X, B - Y as integers in units of
   * xyb_factor[] = the DC quantisation steps of X, Y, B; the colour stage (opsin_inv scaled by 255 / intensity_target,
   * opsin_bias, linear_output as in JxlHipFrameDesc) makes the samples. */
  uint32_t xyb;
  float xyb_factor[3];
  float opsin_inv[9];
  float opsin_bias[3];
  int32_t linear_output;
  const struct JxlHipColorTarget* color_target; /* as JxlHipFrameDesc::color_target (XYB frames only) */
} JxlHipModFrameDesc;
/* Copies a Modular frame's tables and sections to the device (the arrays may be released afterwards). A descriptor that
 * breaks a rule of enum ModRule is refused before any device call: the context keeps its tables but has no frame to run. */
int jxlhip_modular_upload(JxlHipContext* ctx, const JxlHipModFrameDesc* desc);
/* Decodes every stream (one lane each), undoes the transforms and writes the pixels in the format of
 * jxlhip_set_output_format; results through jxlhip_download_pixels / jxlhip_download_rgb8. Stage time: which = 0. */
int jxlhip_modular_run(JxlHipContext* ctx);
/* Same for `n` resident frames: ONE streams launch for all their streams. */
int jxlhip_modular_run_batch(JxlHipContext* const* ctxs, size_t n);
/* Per-stream status words (0 = ok) and end bit positions after a run; synchronous. Returns JXLHIP_ERR_STREAM if any is set. */
int jxlhip_modular_status(JxlHipContext* ctx, uint32_t* status, uint32_t* end_bits, size_t n);
/* Test access: a channel buffer's int32 samples (w * h) after the run; synchronous. */
int jxlhip_modular_download_buffer(JxlHipContext* ctx, uint32_t buffer, int32_t* dst, size_t n);

/* ---- Reduced output: the 1/8-scale image of a VarDCT frame from its DC image alone (jxl_amd.h states what the image is).
 * No AC entropy, no inverse transform, no loop filter: one kernel (k_reduced_pixels, csrc/hip/jxl_hip_reduced.h)
 * dequantises the three coded integer planes (DequantDC), smooths them (AdaptiveDCSmoothing), runs the frame's colour stage
 * and stores through the generic pixel writer, for all the contexts of a batch in one launch. The arithmetic is that of
 * jxlhip_frame_upload's k_dc_dequant and k_dc_smooth (shared device functions): the DC planes agree bit for bit. */
typedef struct JxlHipReducedDesc {
  uint32_t xsize_blocks, ysize_blocks;   /* the size of the reduced image */
  const int32_t* dc_quantised;           /* [3][ysize_blocks][xsize_blocks]: the coded integers of X, Y, B */
  const uint8_t* dc_extra_precision;     /* per DC group of 256 x 256 blocks, row-major: the integers are in units of step /
                                          * 2^this; NULL = 0, for a frame of one DC group only */
  float dc_step[3];                      /* DC quantisation step of X, Y, B */
  float dc_cfl_x, dc_cfl_b;              /* chroma from luma at DC */
  uint32_t dc_smoothing;                 /* != 0: AdaptiveDCSmoothing (the frame has no kSkipAdaptiveDCSmoothing) */
  float opsin_inv[9], opsin_bias[3];     /* the colour stage, as JxlHipFrameDesc's */
  int32_t linear_output;                 /* 0 = sRGB transfer function, 1 = linear (XYB frames only) */
  const struct JxlHipColorTarget* color_target; /* as JxlHipFrameDesc::color_target */
} JxlHipReducedDesc;
/* Copies the integers, the precision bytes and the kernel's descriptor to the device in ONE staged copy; allocates no
 * coefficient buffer, no full-resolution plane and no AC table. The context's output settings apply at the reduced size:
 * jxlhip_set_output_format (every type; 1 or 3 channels: 2 and 4 answer JXLHIP_ERR_UNSUPPORTED, the reduced image is opaque
 * colour), _orientation, jxlhip_set_output_tensor, and jxlhip_set_output_resized with the box in reduced-image coordinates;
 * the descriptor, the tensor and the resized binding are checked on the host at the reduced size (csrc/host/
 * jxh_reduced_plan.h enum ReducedRule) and a refused one launches nothing. Output settings changed after the upload make
 * jxlhip_reduced_run answer JXLHIP_ERR_INVALID_ARGUMENT: upload again.
 * While a context holds a reduced upload, jxlhip_run_entropy / _transform / _filter_color, their _batch forms and
 * jxlhip_run_all, jxlhip_halo_*, the jxlhip_canvas_* calls that take the context and jxlhip_download of anything but "dc"
 * answer JXLHIP_ERR_UNSUPPORTED and launch nothing; jxlhip_frame_upload / jxlhip_modular_upload make it an ordinary context
 * again. jxlhip_set_option(ctx, "keep_dc", 1) before the upload (test aid): the kernel also stores its smoothed DC planes
 * for jxlhip_download(ctx, "dc") ([3][ysize_blocks][xsize_blocks] floats); off, the planes exist nowhere. */
int jxlhip_reduced_upload(JxlHipContext* ctx, const JxlHipReducedDesc* desc);
/* Writes the reduced image: jxlhip_download_pixels / _rgb8 hand it out, or the bound tensor holds it; a resized binding's two
 * resample launches follow the kernel (the context renders f32 into its private buffer first, as for a full frame). The
 * ordering against a tensor's consumer stream is jxlhip_set_output_tensor's, without a host wait. JXLHIP_ERR_INVALID_ARGUMENT on a
 * context whose last upload was not a reduced one (JXLHIP_ERR_NO_FRAME: none at all). Stage time: which = 0. */
int jxlhip_reduced_run(JxlHipContext* ctx);
/* Same for `n` contexts of one device that each hold a reduced upload (any sizes, formats and bindings): ONE launch of the
 * kernel, then one launch pair of the resampler for those with a resized binding. */
int jxlhip_reduced_run_batch(JxlHipContext* const* ctxs, size_t n);

/* ---- The DC image of a window of a frame (region decode; jxl_amd.h "Region decode"): a rectangle of whole 256 x 256
 * groups is uploaded as a frame of its own (a JxlHipFrameDesc of the window's size whose dc_device is what this call
 * leaves), but its DC image must be the FRAME's: dequantised with each DC group's precision shift, looked up at the
 * sample's place in the frame, and smoothed with the true neighbours across the window's edge. One kernel (k_dc_window,
 * csrc/hip/jxl_hip_dc_window.h) makes the window's three dense float planes from the `apron`: the coded integers of the
 * window grown by one block on every side and clipped to the frame. Samples on the FRAME's border are copied unsmoothed
 * (compressed_dc.cc:141-147,171-175); samples on the window's edge elsewhere are smoothed from the apron. The arithmetic
 * is DcDequantSample and DcSmoothSample of jxl_hip_dc.h: the planes equal that rectangle of the whole frame's DC image
 * (jxlhip_frame_upload's k_dc_dequant + k_dc_smooth) bit for bit. All rectangles are in 8x8 blocks of the frame. */
typedef struct JxlHipDcWindow {
  uint32_t frame_xsize_blocks, frame_ysize_blocks;
  uint32_t win_x0, win_y0, win_xsize, win_ysize;          /* the window */
  uint32_t apron_x0, apron_y0, apron_xsize, apron_ysize;  /* the window grown by one block and clipped to the frame */
  const int32_t* apron;                  /* host memory, [3][apron_ysize][apron_xsize]: the coded integers of X, Y, B */
  const uint8_t* dc_extra_precision;     /* the FRAME's, per DC group of 256 x 256 blocks, row-major; NULL = 0, for a
                                          * frame of one DC group only */
  uint32_t num_dc_groups;                /* entries of dc_extra_precision */
  float dc_step[3];
  float dc_cfl_x, dc_cfl_b;
  uint32_t dc_smoothing;                 /* != 0: AdaptiveDCSmoothing */
} JxlHipDcWindow;
/* Copies the apron to the device and runs the kernel on the copy stream, where the DC kernels of jxlhip_frame_upload run;
 * complete when it returns. jxlhip_dc_window_planes hands out the [3][win_ysize][win_xsize] floats, in a buffer the
 * context owns (NULL before the first call): valid until the context's next jxlhip_dc_window or its destruction, which
 * covers the lifetime JxlHipFrameDesc::dc_device asks for. The descriptor is checked on the host first (csrc/host/jxh_window_plan.h enum DcWindowRule: a non-empty
 * window inside the frame, the apron as stated, positive steps, a precision byte for every DC group the apron touches,
 * planes of at most 2^24 samples); a refused one makes no device call. */
int jxlhip_dc_window(JxlHipContext* ctx, const JxlHipDcWindow* window);
const float* jxlhip_dc_window_planes(JxlHipContext* ctx);
/* Test entry: the same, and the planes copied to host_out ([3][win_ysize][win_xsize] floats). The context's buffer gets a
 * kilobyte of room behind the planes and is filled with a sentinel first; JXLHIP_ERR_GUARD when the room was written to. */
int jxlhip_debug_dc_window(JxlHipContext* ctx, const JxlHipDcWindow* window, float* host_out);

/* ---- Canvas: the frames of a multi-frame codestream composed on the device (lib/jxl/blending.cc, alpha.cc,
 * render_pipeline/stage_blending.cc; dec_cache.cc:268-290 for where it sits: after the colour conversion, in the output
 * colour space). A frame is decoded by a context into f32 x 4 pixels (jxlhip_set_output_format(ctx, 0, 4, 0, 0), no
 * orientation), blended into the canvas with the reference slot its header names, optionally kept in a slot, and the
 * canvas is what jxlhip_canvas_download converts to the caller's format. */
typedef struct JxlHipCanvas JxlHipCanvas;
int jxlhip_canvas_create(int device, uint32_t xsize, uint32_t ysize, uint32_t has_alpha, uint32_t alpha_premultiplied, JxlHipCanvas** canvas);
void jxlhip_canvas_destroy(JxlHipCanvas* canvas);
typedef struct JxlHipBlend {
  int32_t x0, y0;             /* FrameOrigin: where the frame's top-left sample sits on the canvas (may be outside) */
  uint32_t mode, alpha_mode;  /* BlendMode of colour / alpha: 0 replace, 1 add, 2 blend, 3 alpha-weighted add, 4 multiply */
  uint32_t source, alpha_source; /* reference slots 0..3 the backgrounds come from (never written: zeros) */
  uint32_t clamp, alpha_clamp;
  int32_t save_slot;          /* 0..3: the blended canvas is also kept in this slot; -1: not kept */
} JxlHipBlend;
/* Frames kept BEFORE the colour transform: copies the XYB planes `frame` holds after its last run (VarDCT: the filtered
 * planes; Modular: needs jxlhip_set_option(frame, "keep_xyb_planes", 1) before the upload) into an XYB slot of the canvas:
 * slots 0..3 = the reference slots (kReferenceOnly frames, the sources of patches), slots 4..7 = the DC frames of level
 * 1..4 (kDCFrame; the DC image of a later frame with kUseDcFrame: JxlHipFrameDesc::dc_device). jxlhip_canvas_xyb_source
 * hands the device planes out ([3][h][w]; NULL / 0 while the slot is empty); they stay valid until the slot is written
 * again or the canvas is destroyed. */
int jxlhip_canvas_save_xyb(JxlHipCanvas* canvas, JxlHipContext* frame, uint32_t slot);
int jxlhip_canvas_xyb_source(JxlHipCanvas* canvas, uint32_t slot, const float** planes, uint32_t* xsize, uint32_t* ysize);
/* The alpha plane kept with that slot's frame (ysize x xsize floats), or NULL when the frame had none. */
int jxlhip_canvas_xyb_alpha(JxlHipCanvas* canvas, uint32_t slot, const float** alpha);
/* Blends the pixels `frame` holds (its last run, f32 x 4) into the canvas. */
int jxlhip_canvas_blend(JxlHipCanvas* canvas, JxlHipContext* frame, const JxlHipBlend* blend);
/* The canvas in a sample format (as jxlhip_set_output_format) and orientation (as jxlhip_set_output_orientation), into
 * host memory; rows of `stride` bytes. Synchronous. */
int jxlhip_canvas_download(JxlHipCanvas* canvas, uint32_t data_type, uint32_t num_channels, uint32_t bits_per_sample, int big_endian,
                           uint32_t orientation, void* dst, size_t stride);
/* jxlhip_canvas_download of a canvas with alpha hands out un-premultiplied colour (as jxlhip_set_output_unpremultiply) in its
 * 2- and 4-channel formats; the canvas itself stays as blended. 0 = off (the default). */
int jxlhip_canvas_set_unpremultiply(JxlHipCanvas* canvas, int on);
/* The canvas alpha plane as floats (xsize * ysize, not oriented). Synchronous. */
int jxlhip_canvas_download_alpha(JxlHipCanvas* canvas, float* dst, size_t n);

/* Test entry: the blend kernel alone on `n` caller-supplied samples: bg planar [4][n] (R, G, B, alpha), fg interleaved
 * [n][4], out planar [4][n]; for the reference's own blending vectors (lib/jxl/alpha_test.cc) against the kernel itself. */
int jxlhip_debug_blend(int device, const float* bg, const float* fg, size_t n, const JxlHipBlend* blend, uint32_t has_alpha,
                       uint32_t alpha_premultiplied, float* out);
/* Test entry: the blend kernel as jxlhip_canvas_blend launches it, on host arrays: a canvas of xsize x ysize, the slot the
 * colour background comes from and the slot the alpha background comes from (each planar [4][ysize][xsize]: the first reads
 * planes 0..2, the second plane 3; NULL: a slot never written, zeros), the frame fg (interleaved [fysize][fxsize][4]) placed
 * at blend->x0 / y0, which may lie partly or wholly outside; out planar [4][ysize][xsize]. source / alpha_source / save_slot
 * of `blend` are not used. Sizes of 0 or above 16384, unknown modes and origins beyond +-2^20 are refused before any launch. */
int jxlhip_debug_blend_rect(int device, uint32_t xsize, uint32_t ysize, const float* bg_color, const float* bg_alpha, const float* fg,
                            uint32_t fxsize, uint32_t fysize, const JxlHipBlend* blend, uint32_t has_alpha, uint32_t alpha_premultiplied,
                            float* out);
/* Test entry: the patch kernel alone on dense host planes [3][ysize][xsize] (alpha_in / alpha_out [ysize][xsize], both or
 * neither; given exactly when patches->uses_alpha is set), rows y_begin .. y_end. Here patches->slot_planes[k]
 * ([3][slot_h][slot_w]) and slot_alpha[k] ([slot_h][slot_w]) are HOST arrays. The dictionary is checked like an upload's
 * (rectangles inside their slot and inside the rows of the planes, row lists consistent; a rectangle may reach past xsize,
 * where the kernel clips it, up to column 32768) and refused before any launch otherwise, as are NULLs, sizes of 0 or above
 * 16384, an empty dictionary and y_end > ysize. */
int jxlhip_debug_patches(JxlHipContext* ctx, const float* planes_in, const float* alpha_in, uint32_t xsize, uint32_t ysize,
                         const JxlHipPatches* patches, uint32_t y_begin, uint32_t y_end, float* planes_out, float* alpha_out);
/* Test entry: the spline kernel alone on dense host planes [3][ysize][xsize] and a draw cache in host memory, rows
 * y_begin .. y_end (the other rows come back as given). Refused before any launch: NULLs, sizes of 0 or above 16384, an empty
 * cache, y_end > ysize, row lists that are inconsistent or name a missing segment, a segment value that is not finite, a
 * centre or maximum distance beyond 2^30. */
int jxlhip_debug_splines(JxlHipContext* ctx, const float* planes_in, uint32_t xsize, uint32_t ysize, const JxlHipSplines* splines,
                         uint32_t y_begin, uint32_t y_end, float* planes_out);

/* ---- Forward path (first slice): the pixel-domain half of a VarDCT encode on the device.
 * Replaces, behind lib/jxl/enc_frame.cc:1135-1166's per-group loop: SRGBToXYB (enc_xyb.cc:152-174), the Gaborish
 * sharpening (enc_gaborish.cc:21-70) and ComputeCoefficients (enc_group.cc:380-533: forward transform, DC from the
 * lowest frequencies, AC quantisation with chroma-from-luma from the dequantised Y). Transform selection and the quant
 * field are this library's own simple activity heuristics by default, not the reference's search (enc_ac_strategy.cc,
 * enc_adaptive_quantization.cc): the output is a valid model of a frame, not libjxl's choice of one. With
 * quant_field_mode 1 the quant field is the reference's initial one (what libjxl writes at its default effort before any
 * Butteraugli iteration), under this library's transform choices. Entropy coding and the headers stay on the host
 * (csrc/enc). */
typedef struct {
  uint32_t xsize, ysize;
  float distance;         /* Butteraugli-style target: scales the thresholds of the transform selection */
  uint32_t gaborish;      /* 1: pre-sharpen with the approximate inverse of the decoder's Gaborish blur */
  /* 0: DCT8 only, 1: activity-driven DCT 8..64 incl. rectangles. 2, 3: the reference's AC-strategy search restricted to the
   * pure-DCT kinds 8x8 .. 64x64 (enc_ac_strategy.cc ProcessRectACS; see jxlhip_enc_acs_walk): mask1x1, the cost estimate of
   * every candidate the walk can ask for (on the sharpened planes, the adaptive quant field, chroma-from-luma factors 0)
   * and the walk, all on the device; 2 is the aligned walk, 3 adds the floating passes. Both need quant_field_mode 1. */
  uint32_t strategy_mode;
  uint32_t global_scale, quant_dc; /* Quantizer parameters of the frame (quantizer.h:82-114) */
  float quant_ac;         /* AC quant target the quant field is built around */
  /* 1: fit the chroma-from-luma factors of every 64x64 tile like the reference's fast path (enc_chroma_from_luma.cc:
   * 128-151 FindBestMultiplier, 204-352 ComputeTile) and quantise X / B against them; 0: factors 0 (X), 0 (B on top of
   * the base 1.0). Output: ytox / ytob, one int8 per tile (ceil(xb / 8) * ceil(yb / 8)), host memory, may be NULL. */
  uint32_t cfl_fit;
  int8_t* ytox;
  int8_t* ytob;
  /* dequantisation tables, as JxlHipFrameDesc: kind k, channel c at dequant[dequant_offset[k] + c * dequant_size[k]] */
  const float* dequant;
  uint32_t dequant_floats;
  uint32_t dequant_offset[17], dequant_size[17];
  /* 0: the quant field is this library's activity rule around quant_ac. 1: the reference's initial adaptive quant field
   * (InitialQuantField with butteraugli_distance_for_iqf = distance, or 0.62 * distance without Gaborish, rescale 1, over
   * the XYB planes before the sharpening: enc_heuristics.cc:1118-1129), aggregated per transform by AdjustQuantField and
   * made integer by SetQuantFieldRect under global_scale; quant_ac is not read. The caller passes the global_scale /
   * quant_dc of ComputeGlobalScaleAndQuant(InitialQuantDC(distance), 0.39 / distance, 0). Anything else is
   * JXLHIP_ERR_INVALID_ARGUMENT. */
  uint32_t quant_field_mode;
} JxlHipEncDesc;
/* rgb: interleaved sRGB8 in host memory, `stride` bytes per row. Outputs (host memory): acs[yb * xb] = (strategy << 1) |
 * first-block bit, qf[yb * xb] (quant field at first blocks), dc[3][yb * xb] quantised DC stored X, Y, B, and
 * coeffs[groups][3][65536] quantised AC, block-contiguous per 256x256 group in raster order of the first blocks
 * (xb = ceil(xsize / 8), groups = ceil(xsize / 256) * ceil(ysize / 256)); coeffs may be NULL (the coefficients then stay
 * on the device: a caller that takes the tokens from jxlhip_enc_tokens needs no copy of them). Synchronous. */
int jxlhip_enc_forward(JxlHipContext* ctx, const uint8_t* rgb, size_t stride, const JxlHipEncDesc* desc, uint8_t* acs, int32_t* qf,
                       int32_t* dc, int32_t* coeffs);
/* Tokenisation of the last jxlhip_enc_forward's coefficients on the device (lib/jxl/enc_entropy_coder.cc:153-255
 * TokenizeCoefficients; csrc/hip/jxl_hip_enc.h): the (context, value) pairs the host entropy coder codes, in bitstream order
 * per 256x256 group (block by block in raster order of the first blocks, channels Y, X, B: the non-zero count, then the
 * coefficients from the first scan position behind the lowest-frequency corner to the last non-zero one). Single pass.
 *   orders: the coefficient orders of the 13 order buckets (one per bucket: the same for the three channels), bucket b at
 *   orders[order_offset[b]]; ctx_map: the block context of (channel, order bucket) at [(c < 2 ? c ^ 1 : 2) * 13 + bucket]
 *   (a block context map without quant-field / DC thresholds, ac_context.h:101-143); num_ctxs its number of contexts;
 *   num_hist: histogram sets (group g uses set g % num_hist: its contexts start at (g % num_hist) * num_ctxs * 495).
 * jxlhip_enc_token_counts computes everything but the tokens and returns every group's token count in totals[groups];
 * jxlhip_enc_tokens then writes group g's tokens at tokens[2 * bases[g] ...] as {context, value} pairs of uint32 (the
 * caller's prefix sum of the totals; `capacity` = number of pairs `tokens` holds). Both synchronous. */
typedef struct {
  const uint16_t* orders;
  uint32_t orders_size;
  uint32_t order_offset[13];
  uint8_t ctx_map[39];
  uint32_t num_ctxs, num_hist;
} JxlHipEncTokDesc;
int jxlhip_enc_token_counts(JxlHipContext* ctx, const JxlHipEncTokDesc* desc, uint32_t* totals);
int jxlhip_enc_tokens(JxlHipContext* ctx, const uint32_t* bases, uint32_t* tokens, size_t capacity);
/* Entropy coding of the resident tokens (those of the last jxlhip_enc_tokens, which stay on the device: with tokens = NULL
 * that call copies nothing to the host and `capacity` only bounds the ranges) - csrc/hip/jxl_hip_enc.h, "entropy coding".
 * The host keeps what is small and serial (clustering, normalisation, alias tables, headers); the device counts and writes.
 *
 * jxlhip_enc_histograms: counts[num_ctx][256] receives how often every hybrid-uint symbol (split_exp / msb_in_token /
 * lsb_in_token as in a coded HybridUintConfig, dec_ans.h:64-98) occurs in every context, *max_token the largest symbol.
 * A symbol >= 256 is not counted and makes the call return JXLHIP_ERR_INVALID_ARGUMENT (*max_token then still says which),
 * a token context >= num_ctx likewise.
 *
 * jxlhip_enc_ans_sizes rANS-codes every group's tokens backwards from the final state (ans_params.h: 0x13 << 16) with the
 * caller's code and returns each group's exact length in bits, bit_counts[groups]; jxlhip_enc_ans_write then places group g's
 * bit string (LSB first; the unused bits of its last byte zero) at out[byte_bases[g]], ceil(bit_counts[g] / 8) bytes:
 *   prefix_count[g] (<= 8) bits of prefix_value[g], the 32-bit state, then per token in order the 16-bit chunk it flushed
 *   (if any) and its extra bits: what follows an AC group's histogram selector in the stream (dec_group.cc:594-610).
 * The code: ctx_map[num_ctx] < num_clusters (<= 256); per cluster the frequencies freq[cluster][256] (summing to 4096; 0 =
 * the symbol has no code: a token that needs it makes the call fail, nothing is written for it), rev_start[cluster][256]
 * (the running sum of the frequencies) and rev[cluster][4096], the slot of (symbol, offset) at rev_start + offset: the
 * inverse of the decoder's alias table (ans_common.h:102-142). Every entry is validated at the call.
 * All three synchronous, on the context's stream. */
typedef struct {
  uint32_t split_exp, msb_in_token, lsb_in_token;
  uint32_t num_ctx;
} JxlHipEncHistDesc;
typedef struct {
  uint32_t split_exp, msb_in_token, lsb_in_token;
  uint32_t num_ctx;
  const uint8_t* ctx_map;
  uint32_t num_clusters, log_alpha;
  const uint16_t* freq;
  const uint16_t* rev_start;
  const uint16_t* rev;
  const uint8_t* prefix_count;
  const uint8_t* prefix_value;
} JxlHipEncAnsDesc;
int jxlhip_enc_histograms(JxlHipContext* ctx, const JxlHipEncHistDesc* desc, uint32_t* counts, uint32_t* max_token);
int jxlhip_enc_ans_sizes(JxlHipContext* ctx, const JxlHipEncAnsDesc* desc, uint32_t* bit_counts);
int jxlhip_enc_ans_write(JxlHipContext* ctx, const uint64_t* byte_bases, uint8_t* out, size_t capacity);
/* Test access: makes tokens[2 * n] ({context, value} pairs) the resident tokens, as one group, and runs the two calls above
 * on them (prefix_count / prefix_value: one entry); out receives ceil(*bits / 8) bytes. jxlhip_enc_histograms then counts
 * the same tokens. */
int jxlhip_debug_ans_write(JxlHipContext* ctx, const uint32_t* tokens, size_t n, const JxlHipEncAnsDesc* desc, uint8_t* out, size_t capacity,
                           uint64_t* bits);
/* Kernel time of the last jxlhip_enc_histograms (ms[0]) and of the last jxlhip_enc_ans_sizes + jxlhip_enc_ans_write (ms[1]),
 * milliseconds (HIP events around the launches, copies excluded); 0 for a pass that has not run. */
int jxlhip_enc_entropy_last_ms(JxlHipContext* ctx, float* ms);
/* The reference's initial adaptive quant field alone (lib/jxl/enc_adaptive_quantization.cc InitialQuantField :1264-1271 ->
 * AdaptiveQuantizationMap :664-705, without mask1x1 and its blur): xyb = the X, Y, B planes [3][ysize][xsize] in host
 * memory, xsize and ysize multiples of 8 (the image padded to whole blocks; a neighbour outside is the nearest sample);
 * butteraugli_target = the distance the field is built for (enc_heuristics.cc:1119-1122), rescale as there (1).
 * Outputs, host memory: aq_map[ysize / 8][xsize / 8] the field per block, before AdjustQuantField; mask (may be NULL)
 * the masking image the AC-strategy search reads. log2 / exp2 are exact where the reference approximates them
 * (relative 3e-7). Synchronous; leaves the last jxlhip_enc_forward's state as it was. */
int jxlhip_enc_initial_quant_field(JxlHipContext* ctx, const float* xyb, uint32_t xsize, uint32_t ysize, float butteraugli_target,
                                   float rescale, float* aq_map, float* mask);
/* The per-pixel masking the reference's AC-strategy search reads (mask1x1: enc_adaptive_quantization.cc ComputeTile :498-526
 * and Blur1x1Masking :634-662, borders as convolve_symmetric5.cc has them), alone: xyb as above (only the Y plane is read),
 * taken BEFORE any sharpening, like the quant field; out[ysize][xsize] in host memory. log1p is the exact function, as in the
 * reference. Synchronous; leaves the last jxlhip_enc_forward's state as it was. jxlenc_cpu_masking_1x1 (libjxlenc) is the
 * CPU double with the same arguments less the context. */
int jxlhip_enc_masking_1x1(JxlHipContext* ctx, const float* xyb, uint32_t xsize, uint32_t ysize, float* out);
/* Kernel time of the last jxlhip_enc_masking_1x1 (copies excluded), milliseconds. */
int jxlhip_enc_masking_last_ms(JxlHipContext* ctx, float* ms);
/* The cost estimate of the reference's AC-strategy search (EstimateEntropy, enc_ac_strategy.cc:364-511, with the constants of
 * AcStrategyHeuristics::Init :1107-1123) for a list of candidate transforms, alone. All pointers are host memory. */
typedef struct {
  const float* xyb;         /* [3][ysize][xsize] X, Y, B: the planes the transforms would be taken of */
  uint32_t xsize, ysize;    /* multiples of 8 */
  const float* quant_field; /* [ysize / 8][xsize / 8]: aq_map of jxlhip_enc_initial_quant_field */
  const float* mask1x1;     /* [ysize][xsize]: jxlhip_enc_masking_1x1 */
  const int8_t* ytox;       /* one per 64x64 tile, ceil(xsize / 64) per row: the factors are v / 84 and 1 + v / 84 */
  const int8_t* ytob;
  float distance;           /* the Butteraugli target */
  /* dequantisation tables, as JxlHipEncDesc: kind k, channel c at dequant[dequant_offset[k] + c * dequant_size[k]] */
  const float* dequant;
  uint32_t dequant_floats;
  uint32_t dequant_offset[17], dequant_size[17];
} JxlHipEncEstimateDesc;
/* strategy: an AcStrategy number of the pure-DCT kinds up to 64x64 (0, 4 .. 11, 18 .. 20); (bx, by): its top-left block;
 * entropy_mul: the multiplier of the bit estimate (not of the loss) the caller's walk attaches. */
typedef struct {
  uint32_t strategy, bx, by;
  float entropy_mul;
} JxlHipEncAcsCandidate;
/* estimates[i] = EstimateEntropy of candidates[i]. scaled (may be NULL; for tests) receives per candidate 3 * R * C floats,
 * candidate i starting at 3 * (the areas before it): channel X, Y, B, the quantised value before rounding (`val` of :432) of
 * the coefficient of vertical frequency ky and horizontal frequency kx at ky * C + kx (tall transforms are NOT transposed
 * here). Every candidate must lie inside the planes and inside one 64x64 tile; anything else, a null pointer, a strategy
 * that is not listed, a size that is no multiple of 8 or a table that does not hold a used kind is
 * JXLHIP_ERR_INVALID_ARGUMENT, decided on the host before any device call. powf is exact where the reference has
 * FastPowf (:413). Synchronous; leaves the last jxlhip_enc_forward's state as it was. jxlenc_cpu_estimate_entropy
 * (libjxlenc) is the CPU double with the same arguments less the context. */
int jxlhip_enc_estimate_entropy(JxlHipContext* ctx, const JxlHipEncEstimateDesc* desc, const JxlHipEncAcsCandidate* candidates, size_t n,
                                float* estimates, float* scaled);
/* Kernel time of the last jxlhip_enc_estimate_entropy (all its launches, copies excluded), milliseconds. */
int jxlhip_enc_estimate_last_ms(JxlHipContext* ctx, float* ms);
/* The merge walk of the reference's AC-strategy search (ProcessRectACS, enc_ac_strategy.cc:827-1059, from the 8x8 estimates
 * on, decoding_speed_tier 0, DCT the only 8x8 kind), alone, on a caller's table of estimates in host memory.
 *   estimates: per 64x64 tile in raster order (ceil(xb / 8) per row) [kind 0..9][cy][cx] floats, 640 per tile; kinds 8x8,
 *   16x8, 8x16, 16x16, 32x16, 16x32, 32x32, 64x32, 32x64, 64x64 (rows x columns: AcStrategy 0, 6, 7, 4, 10, 11, 5, 19, 20,
 *   18), (cx, cy) the candidate's top-left block inside the tile, each estimate with its kind's multiplier already applied
 *   (jxlenc_acs_walk_candidates of libjxlenc lists what is read, with those multipliers). Entries nothing asks for are not read.
 *   floating 0: the aligned walk (the reference's effort 5); 1: with the two floating passes (:1033-1057, every position).
 * acs[yb * xb] receives (strategy << 1) | first-block bit, entropy (may be NULL) the walk's final entropy_estimate per block.
 * One deviation, stated in csrc/host/jxh_enc_shared.h (AcsWalkTryMerge): a merge that would cut a transform placed earlier is
 * refused, where the reference writes an overlapping strategy image. A null pointer, a zero size, distance <= 0 or
 * floating > 1 is JXLHIP_ERR_INVALID_ARGUMENT before any device call. Synchronous; leaves the last jxlhip_enc_forward's state
 * as it was. jxlenc_cpu_acs_walk (libjxlenc) is the CPU double with the same arguments less the context. */
typedef struct {
  uint32_t xb, yb;   /* the frame in 8x8 blocks */
  float distance;    /* the Butteraugli target: the 8x8 estimates are multiplied by 1 - 0.4 / (distance + 1.4) */
  uint32_t floating;
} JxlHipEncAcsWalkDesc;
int jxlhip_enc_acs_walk(JxlHipContext* ctx, const JxlHipEncAcsWalkDesc* desc, const float* estimates, uint8_t* acs, float* entropy);
/* Kernel time of the three parts of the search in the last pass of the last jxlhip_enc_forward / _rerun made with
 * strategy_mode 2 or 3: ms[0] the per-pixel masking, ms[1] all estimate launches, ms[2] the walk (they are part of
 * jxlhip_enc_last_ms too). JXLHIP_ERR_NO_FRAME after anything else. */
int jxlhip_enc_search_last_ms(JxlHipContext* ctx, float* ms);
/* Test access: what the search of the last jxlhip_enc_forward made with strategy_mode 2 or 3 read and wrote, to host memory
 * (any pointer may be NULL): the XYB planes before and after the sharpening [3][yp][xp] each (the same without Gaborish),
 * aq_map [yb][xb], mask1x1 [yp][xp] and the estimate table (640 floats per tile; entries nothing asked for are zero). */
int jxlhip_debug_enc_search(JxlHipContext* ctx, float* planes_before, float* planes_after, float* aq_map, float* mask1x1, float* estimates);
/* Kernel time of the two quant-field kernels in the last pass of the last jxlhip_enc_forward / _rerun made with
 * quant_field_mode 1 (they are part of jxlhip_enc_last_ms too), milliseconds. */
int jxlhip_enc_aq_last_ms(JxlHipContext* ctx, float* ms);
/* Measurement: runs the kernel sequence of the last jxlhip_enc_forward `times` more times on its input, which is still
 * resident on the device (no copies); jxlhip_enc_last_ms then gives the time of all `times` passes. Synchronous. */
int jxlhip_enc_forward_rerun(JxlHipContext* ctx, uint32_t times);
/* Kernel time of the last jxlhip_enc_forward (HIP events around the launches, copies excluded), milliseconds. */
int jxlhip_enc_last_ms(JxlHipContext* ctx, float* ms);
/* The forward-transform kernel alone (the last pass of the last call), milliseconds. */
int jxlhip_enc_last_transform_ms(JxlHipContext* ctx, float* ms);

/* Timing of the last run of each stage in milliseconds (HIP events on the context's stream);
 * which: 0 entropy, 1 transform, 2 filter+colour. Synchronous. */
int jxlhip_last_stage_ms(JxlHipContext* ctx, int which, float* ms);

const char* jxlhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JXL_AMD_HIP_H_ */
