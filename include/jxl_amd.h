/* libjxl_amd — frame-level C ABI between the host front-end and the HIP layer. Used by the JxlDecoder
 * implementation, by bench.py and by the parity tests to time the device stages separately from host parsing.
 *
 * jxlamd_frame_parse() does what the reference does once per frame on the host before any group is decoded
 * (lib/jxl/dec_frame.cc:135-434: headers, TOC, DC global, DC groups through the JxlParallelRunner, AC global);
 * jxlamd_frame_upload() hands the resulting tables and the still-compressed AC sections to a JxlHipContext. */
#ifndef JXL_AMD_H_
#define JXL_AMD_H_
#include <jxl/color_encoding.h>
#include <jxl/parallel_runner.h>
#include <stddef.h>
#include <stdint.h>

#include "jxl_amd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct JxlAmdFrame JxlAmdFrame;

/* Parses the first frame of a codestream (bare or in a `jxlc` container). `data` must stay valid until the frame
 * has been uploaded. runner may be NULL (sequential). Returns 0 or a non-zero code; see jxlamd_last_error(). */
int jxlamd_frame_parse(const uint8_t* data, size_t size, JxlParallelRunner runner, void* runner_opaque, JxlAmdFrame** frame);
/* The frame that starts at byte `frame_pos` of the buffer (the jxlamd_frame_end() of the one before it; 0 = the first),
 * `frame_index` its position in the codestream. Frames after the first exist in animations whose frames each replace the
 * whole canvas (decode.cc:1346-1350; full size, BlendMode kReplace, a duration): anything layered, blended, cropped or
 * referenced is refused. */
int jxlamd_frame_parse_at(const uint8_t* data, size_t size, size_t frame_pos, size_t frame_index, JxlParallelRunner runner,
                          void* runner_opaque, JxlAmdFrame** frame);
/* The same from a PREFIX of the frame's bytes (what JxlDecoderFlushImage draws from; lib/jxl/dec_frame.cc:735-795 Flush,
 * decode.cc:2458-2475): succeeds once the frame header, the TOC, the DC image (DC global + DC groups) and the AC global
 * section are whole. A group is drawn from its leading passes whose sections are whole (dec_frame.cc:620-680), from the DC
 * image alone when it has none; *groups_present = the number of groups with at least one pass. Fails ("truncated frame") for frames coded as a single
 * section and for frames with extra channels. jxlamd_frame_is_partial() tells such a frame from a whole one. */
int jxlamd_frame_parse_partial_at(const uint8_t* data, size_t size, size_t frame_pos, size_t frame_index, JxlParallelRunner runner,
                                  void* runner_opaque, JxlAmdFrame** frame, uint32_t* groups_present);
/* How many passes, from the first, EVERY group of the frame would have with `have_bytes` of the buffer there (a whole
 * frame, or one parsed from a prefix: its table of contents is known): what FrameDecoder::NumCompletePasses reports
 * (dec_frame.h:186-200) and JXL_DEC_FRAME_PROGRESSION steps by. info (optional, 10 values): num_passes, num_downsample,
 * downsample[4], last_pass[4] of the frame header's Passes (frame_header.h:286-309). */
uint32_t jxlamd_frame_complete_passes(const JxlAmdFrame* frame, size_t have_bytes, uint32_t* info);
int jxlamd_frame_is_partial(const JxlAmdFrame* frame);
/* Byte offset just behind the frame, and its animation fields {duration in ticks, is_last, timecode}. */
size_t jxlamd_frame_end(const JxlAmdFrame* frame, uint32_t* duration_last_timecode);
/* Where a frame sits on the canvas and how it combines with the reference slots (frame_header.h: FrameOrigin,
 * BlendingInfo, save_as_reference; blending.cc): what a caller needs to compose frames on a JxlHipCanvas. */
typedef struct {
  int32_t x0, y0;
  uint32_t xsize, ysize;
  uint32_t custom_size, frame_type; /* frame_type: 0 regular, 1 DC frame, 2 reference only (kept in XYB for patches), 3 skip-progressive */
  uint32_t mode, alpha_mode, source, alpha_source, clamp, alpha_clamp;
  uint32_t duration, is_last, save_as_reference, save_before_color_transform;
  /* DC frames (frame_header.h:319,348,439): dc_level 1..4 for a kDCFrame (its output, kept before the colour transform, is
   * the DC image of level dc_level - 1); use_dc_frame != 0: this frame's DC image is the DC frame of level dc_level + 1. */
  uint32_t dc_level, use_dc_frame;
} JxlAmdFramePlacement;
void jxlamd_frame_placement(const JxlAmdFrame* frame, JxlAmdFramePlacement* placement);
/* The struct above has grown (dc_level, use_dc_frame) and may grow again; it carries no size field. Callers that are not
 * compiled against THIS header (FFI mirrors, older binaries) use the sized forms: at most `out_size` bytes are written,
 * the return value is sizeof(JxlAmdFramePlacement) as this library knows it (also: jxlamd_sizeof_frame_placement). */
size_t jxlamd_sizeof_frame_placement(void);
size_t jxlamd_frame_placement_sized(const JxlAmdFrame* frame, void* placement, size_t out_size);
/* The frame's position among the shown / invisible frames (seeds its noise: dec_frame.cc:160-168); before upload. */
void jxlamd_frame_set_indices(JxlAmdFrame* frame, uint32_t visible_index, uint32_t nonvisible_index);
/* The reference frames a frame's patches read (device XYB planes of the four slots, jxlhip_canvas_xyb_source); checks every
 * patch rectangle against them. Before upload; returns non-zero (see jxlamd_last_error) when a patch refers to an empty
 * slot or reaches outside its reference frame. */
int jxlamd_frame_set_patch_sources(JxlAmdFrame* frame, const float* const* planes, const uint32_t* xsize, const uint32_t* ysize);
/* ... and their alpha planes (jxlhip_canvas_xyb_alpha; NULL entries: none), for patches that blend through alpha or write the
 * alpha channel (PatchBlendMode 4..7, or a mode on the alpha channel: blending.cc:40-190). Fails when such a patch names a
 * reference frame without alpha, when the frame is upsampled, or when the image's extra channel is not alpha. Call after
 * jxlamd_frame_set_patch_sources, before the upload. */
int jxlamd_frame_set_patch_alpha_sources(JxlAmdFrame* frame, const float* const* alpha);
/* A frame with kUseDcFrame: the device planes of the DC frame it names ([3][ysize][xsize] floats, e.g. from
 * jxlhip_canvas_xyb_source(canvas, 4 + placement.dc_level, ...)); fails unless the size is the frame's size in blocks. */
int jxlamd_frame_set_dc_source(JxlAmdFrame* frame, const float* planes, uint32_t xsize, uint32_t ysize);
void jxlamd_frame_free(JxlAmdFrame* frame);
/* info[0..15]: xsize, ysize, xsize_blocks, ysize_blocks, num_groups, num_dc_groups, num_passes, used_acs mask,
 * epf_iters, gab, coefficient storage bits (16/32), total AC section bytes, then of pass 0: log2 alphabet size,
 * number of clustered histograms, context map bytes; [15] reserved (0). */
void jxlamd_frame_info(const JxlAmdFrame* frame, uint32_t* info);
/* Byte sizes of the frame's AC group sections, [pass * num_groups + group]; returns their number (sizes may be NULL / short). */
size_t jxlamd_frame_section_sizes(const JxlAmdFrame* frame, uint32_t* sizes, size_t n);
/* Size of the decoded image: the frame size, times the upsampling factor of an upsampled frame (cropped to the image). */
void jxlamd_frame_out_size(const JxlAmdFrame* frame, uint32_t* width_height);
int jxlamd_frame_upload(const JxlAmdFrame* frame, JxlHipContext* ctx);
/* Test aid: exchanges what varblocks i and j of the parsed frame say about themselves (position, strategy, quant field, DC
 * context), leaving their coefficient offsets in place: a descriptor whose varblocks are not in raster order, for the
 * upload's validation. Returns 0, or 1 when an index is out of range. */
int jxlamd_frame_debug_swap_blocks(JxlAmdFrame* frame, uint32_t i, uint32_t j);
/* Same, for a band of rows of 256x256 groups [group_row_begin, group_row_end) (see JxlHipFrameDesc); 0, 0 = whole frame. */
int jxlamd_frame_upload_band(const JxlAmdFrame* frame, JxlHipContext* ctx, uint32_t group_row_begin, uint32_t group_row_end);
/* Output transfer function of the frame's pixels: 0 = sRGB, 1 = linear (JxlDecoderSetOutputColorProfile); before upload. */
void jxlamd_frame_set_linear_output(JxlAmdFrame* frame, int linear);
/* The colour stage the JxlDecoder gives a frame of an XYB image whose encoding is tagged by enums (or is grey), for callers
 * of this frame-level API: rendered to `target` (NULL: the image's own encoding; PQ, HLG, P3, grey luminance rows ...)
 * for `desired_intensity` (0 = the image's). Frames of other images keep the sRGB / linear stage. Before upload; returns
 * non-zero (see jxlamd_last_error) for a target the stage cannot render. */
int jxlamd_frame_set_color_output(JxlAmdFrame* frame, const JxlColorEncoding* target, float desired_intensity);

/* ---- Reduced decode: the image at 1/8 scale from the frame's own DC image, which the first sections of the file hold.
 * The reduced image of a frame of xsize_blocks x ysize_blocks 8x8 blocks has that size, ceil(xsize / 8) x ceil(ysize / 8).
 * Sample (bx, by) is the frame's DC sample as a full decode builds it (DequantDC, compressed_dc.cc:201-296, then
 * AdaptiveDCSmoothing unless the frame has kSkipAdaptiveDCSmoothing), through the frame's own colour stage and the output
 * stage of the context (format, orientation, tensor and resized bindings at the reduced size). Gaborish, EPF and noise are
 * NOT applied (noise is zero-mean and is left out silently). By the format's construction this is the 8x8 block mean of the
 * image in XYB, exactly for DCT8 blocks and approximately under larger transforms. The definition is this project's own:
 * the reference has no 1/8-size output (it draws DC-only frames at full size through its 8x upsampler).
 *
 * jxlamd_frame_dc_extent: from the headers and the TOC alone, *need = the number of leading bytes of the buffer that the
 * reduced parse reads: the largest end of TOC sections 0 .. num_dc_groups (DC global and the DC groups; the TOC may be
 * permuted), or the frame's end for a frame coded as one section. The buffer may be a prefix of the file, bare or in a
 * `jxlc` box (a box whose declared end lies beyond the buffer is accepted here and by the reduced parse); too short for the
 * headers and the TOC: fails with "truncated frame header", come back with more. */
int jxlamd_frame_dc_extent(const uint8_t* data, size_t size, size_t* need);
/* Parses the first frame for a reduced decode from the whole file or any prefix of at least `need` bytes ("truncated frame"
 * with fewer): headers, TOC, the DC global section in full (its Modular tree may code the DC streams), then each DC group up
 * to the end of its VarDCT DC stream, through the runner. No AC global section, no block lists. Refused, each with its own
 * jxlamd_last_error text and before any DC group is decoded: a Modular frame; a first frame that is not a regular,
 * full-canvas, is_last, kReplace frame (animations, layers, crops, reference-only and DC frames); kUseDcFrame; patches;
 * splines; frame upsampling above 1; chroma subsampling; an image that is not XYB-encoded; a first frame that is the image's
 * preview. Extra channels are
 * accepted and ignored: the output is opaque colour. jxlamd_frame_upload / _upload_band refuse such a frame. */
int jxlamd_frame_parse_reduced(const uint8_t* data, size_t size, JxlParallelRunner runner, void* runner_opaque, JxlAmdFrame** frame);
int jxlamd_frame_is_reduced(const JxlAmdFrame* frame);
/* width_height = {xsize_blocks, ysize_blocks}: the size of the reduced image (before the context's orientation). */
void jxlamd_frame_reduced_size(const JxlAmdFrame* frame, uint32_t* width_height);
/* Test access, as sized copies: the three coded integer planes X, Y, B ([3][ysize_blocks][xsize_blocks], `n` values of room)
 * and the precision shift of every DC group (`groups` bytes of room); either may be NULL. A reduced frame or a whole one. */
int jxlamd_frame_dc_quantised(const JxlAmdFrame* frame, int32_t* q, size_t n, uint8_t* extra_precision, size_t groups);
/* Hands the DC image to a context (jxlhip_reduced_upload) with the colour description jxlamd_frame_upload would fill; then
 * jxlhip_reduced_run. A reduced frame, or a whole one (it holds the same DC) that the reduced parse would have taken: the same
 * refusals apply to it here. jxlamd_frame_set_linear_output / _set_color_output apply as before. */
int jxlamd_frame_upload_reduced(const JxlAmdFrame* frame, JxlHipContext* ctx);

/* ---- Region decode: only the 256 x 256 groups a box of the output image reads. The window is the smallest rectangle of
 * whole groups that covers the box grown by the reach of the frame's loop filters (0 to 7 pixels: Gaborish 1, EPF 2 / 3 / 6)
 * and clipped to the frame. It is uploaded as a frame of its own (csrc/host/jxh_window_plan.h BuildWindowDesc): the context
 * then IS a frame of the window's size for every later call (the stage launches and their batch forms, downloads, tensor and
 * resized bindings; jxlhip_get_errors is indexed by window group), and every pixel of the caller's box equals the whole
 * decode's bit for bit, since the same kernels run the same arithmetic on the same inputs. The window's DC image is the
 * frame's (jxlhip_dc_window).
 * jxlamd_frame_plan_window needs no device. box = {x0, y0, xsize, ysize} in the oriented output image (what
 * JxlHipResizedOut takes; all zero: the whole image), num_channels as jxlhip_set_output_format's; window->orientation is
 * read: the orientation the context's output undoes (jxlhip_set_output_orientation; 0 or 1: none), everything else is
 * written. Returns non-zero (jxlamd_last_error) for a box jxlhip_set_output_resized would refuse at the image's size.
 * reason != 0 (enum WholeFrameReason of jxh_window_plan.h: 1 partial or reduced parse, 2 upsampling, 3 chroma subsampling,
 * 4 noise, 5 patches, 6 splines, 7 kUseDcFrame, 8 an output with alpha, 9 a single-section frame, 10 a frame of one group,
 * 11 a window that equals the frame): the window is the whole frame, `box` the caller's, and jxlamd_frame_upload_window is
 * jxlamd_frame_upload. A reason is a report, not an error.
 * Deviation from a whole decode: a damaged AC section in a group the window does not read is not seen. */
typedef struct {
  uint32_t orientation;                 /* in: 1..8, EXIF numbering (0 = 1) */
  uint32_t x0, y0, xsize, ysize;        /* the window in frame pixels */
  uint32_t gx0, gy0, gxs, gys;          /* and in groups: frame group (gy0 + i / gxs) * frame groups per row + gx0 + i % gxs
                                         * is the window's group i */
  uint32_t box[4];                      /* the caller's box in the oriented coordinates of the window image: bind this one */
  uint32_t groups_taken, groups_in_frame;
  uint32_t reason;
} JxlAmdWindow;
size_t jxlamd_sizeof_window(void);
int jxlamd_frame_plan_window(const JxlAmdFrame* frame, const uint32_t box[4], uint32_t num_channels, JxlAmdWindow* window);
/* Uploads the window jxlamd_frame_plan_window planned for this frame (the plan is made again from window->orientation and
 * the window's own rectangle, and must agree). Bind the output first, with window->box. */
int jxlamd_frame_upload_window(const JxlAmdFrame* frame, JxlHipContext* ctx, const JxlAmdWindow* window);
/* Extra channels (alpha, ...) of the frame. jxlamd_frame_extra_pending() != 0: their data continues behind the
 * coefficients of the AC group sections; run the entropy stage, then jxlamd_frame_finish_extra() (which reads the section
 * end positions from the context). jxlamd_frame_extra_plane() returns channel `index` as xsize * ysize int32 samples
 * (the frame's size), or NULL while pending / when there is no such channel. */
int jxlamd_frame_extra_pending(const JxlAmdFrame* frame);
int jxlamd_frame_finish_extra(JxlAmdFrame* frame, JxlHipContext* ctx);
/* The same with the groups' Modular streams spread over the caller's runner (NULL: serial). */
int jxlamd_frame_finish_extra_mt(JxlAmdFrame* frame, JxlHipContext* ctx, JxlParallelRunner runner, void* runner_opaque);
const int32_t* jxlamd_frame_extra_plane(const JxlAmdFrame* frame, uint32_t index);
/* An extra channel carries an upsampling factor of its own (frame_header.cc:265-283; dec_modular.cc:262-271): whu[0], whu[1] =
 * the size jxlamd_frame_extra_plane() has, ceil(image / factor); whu[2] = the factor (1, 2, 4, 8). jxlhip_upsample_plane
 * makes the image-sized plane of a factor > 1. Returns 0, or 1 for a bad argument. */
int jxlamd_frame_extra_dims(const JxlAmdFrame* frame, uint32_t index, uint32_t* whu);
/* The factor * factor 5x5 upsampling kernels of the image (its coded weights or the default ones: image_metadata.cc:87-214,
 * stage_upsampling.cc:59-84), factor * factor * 25 floats in JxlHipFrameDesc::upsampling_kernel's layout. */
int jxlamd_upsampling_kernels(const JxlAmdFrame* frame, uint32_t factor, float* kernels);
/* ---- Modular (lossless) frames: host parse into the plan the device decodes (csrc/host/jxh_modframe.h) ---- */
typedef struct JxlAmdModFrame JxlAmdModFrame;
/* Parses the first frame of a codestream as a Modular frame: headers, TOC, global tree and histograms and every stream's
 * group header; no sample is decoded on the host. `data` must stay valid until the frame has been uploaded. */
int jxlamd_modframe_parse(const uint8_t* data, size_t size, JxlAmdModFrame** frame);
/* Which of the two front-ends takes the codestream's first frame, from its frame header alone: *modular = 1 for
 * jxlamd_modframe_parse, 0 for jxlamd_frame_parse. */
int jxlamd_frame_is_modular(const uint8_t* data, size_t size, uint32_t* modular);
/* The reference frames a Modular frame's patches read: as jxlamd_frame_set_patch_sources (before the upload). */
int jxlamd_modframe_set_patch_sources(JxlAmdModFrame* frame, const float* const* planes, const uint32_t* xsize, const uint32_t* ysize);
/* As jxlamd_frame_parse_at / jxlamd_frame_end, for Modular frames. */
int jxlamd_modframe_parse_at(const uint8_t* data, size_t size, size_t frame_pos, size_t frame_index, JxlAmdModFrame** frame);
size_t jxlamd_modframe_end(const JxlAmdModFrame* frame, uint32_t* duration_last_timecode);
void jxlamd_modframe_placement(const JxlAmdModFrame* frame, JxlAmdFramePlacement* placement);
size_t jxlamd_modframe_placement_sized(const JxlAmdModFrame* frame, void* placement, size_t out_size);
/* Test access to a frame's splines, as sized copies (at most out_size bytes are written; the return value is the size of the
 * whole in bytes, 0 for a frame without splines or an unknown `what`). what = 0: the dictionary as parsed, int32 words:
 * quantisation adjustment, number of splines, then per spline its starting point x, y, the number of further control
 * points, their double deltas (x, y each), 3 x 32 colour DCT integers (X, Y, B) and 32 sigma DCT integers. what = 1 .. 3:
 * the draw cache built from it, as JxlHipSplines lays it out: segments (8 floats each), row_start (ysize + 1 uint32),
 * row_segments (uint32). what = 4: four words: the xsize and ysize the cache was built for (the frame's own, also when the
 * frame is upsampled) and, as floats, the y_to_x and y_to_b used (a Modular frame: 0 and 1). */
size_t jxlamd_frame_splines(const JxlAmdFrame* frame, uint32_t what, void* out, size_t out_size);
size_t jxlamd_modframe_splines(const JxlAmdModFrame* frame, uint32_t what, void* out, size_t out_size);
void jxlamd_modframe_free(JxlAmdModFrame* frame);
/* info[0..15]: xsize, ysize, colour channels, has alpha, bits per sample, streams, channel buffers, transform operations,
 * extra channels, compressed bytes of all sections; [10..12] largest symbol-table set (words), LZ77 anywhere, largest
 * tree; [13] launch levels of the inverse transforms (the deepest chain of group-local operations + the frame's own
 * transforms: one launch per level and kind, whatever the number of groups), [14] group-local operations, [15] the deepest
 * group-local chain. */
void jxlamd_modframe_info(const JxlAmdModFrame* frame, uint32_t* info);
/* TOC section `index` (0 = DC global, then the DC groups, then the AC groups; a one-group frame has section 0 only): where
 * it starts in the buffer given to the parser and its size. Returns 0, or 1 when there is no such section. */
int jxlamd_modframe_section(const JxlAmdModFrame* frame, uint32_t index, uint64_t* offset, uint32_t* size);
/* Hands the plan to a context (jxlhip_modular_upload); then jxlhip_modular_run + jxlhip_download_pixels. */
int jxlamd_modframe_upload(const JxlAmdModFrame* frame, JxlHipContext* ctx);
/* Test aid: pushes the first rectangle of inverse-transform operation `op` of the parsed frame one column outside its
 * buffer: a descriptor the upload's validation must refuse. Returns 0, or 1 when there is no such operation. */
int jxlamd_modframe_debug_shift_op(JxlAmdModFrame* frame, uint32_t op);
/* Channel buffer of extra channel `index` after the run (jxlhip_modular_download_buffer), or 0xFFFFFFFF. */
uint32_t jxlamd_modframe_extra_buffer(const JxlAmdModFrame* frame, uint32_t index);
/* Thread-local description of the last failure of a jxlamd_* call ("" if none). */
const char* jxlamd_last_error(void);
/* Decodes a coded ICC profile: the entropy-coded, predicted byte stream that follows the headers of an image whose
 * ImageMetadata.color_encoding has want_icc (lib/jxl/icc_codec.cc:128-428). Returns 0 on success; *profile_size = bytes
 * of the profile, *coded_bits = exact length of the coded form; the profile is copied when out_size is large enough. */
int jxlamd_icc_decode(const uint8_t* coded, size_t size, uint8_t* out, size_t out_size, size_t* profile_size, size_t* coded_bits);
/* Test entry: the output description of the XYB colour stage (lib/jxl/dec_xyb.cc:127-250, stage_tone_mapping.cc:30-76,
 * stage_from_linear.cc:146-168) for an image coded in `source` with intensity target `source_intensity`, rendered to the
 * RGB encoding `target` (or, source and target both D65 grey, to grey: three equal luminance rows) for `desired_intensity`
 * (0 = the image's). inv_opsin: the image's OpsinInverseMatrix, row-major
 * (NULL = the default one). out->tf is the target's transfer function; the decoder hands frames whose target is sRGB or
 * linear without tone mapping the matrix alone. Returns 0, or 1 (see jxlamd_last_error). */
int jxlamd_color_output(const JxlColorEncoding* source, float source_intensity, const JxlColorEncoding* target, float desired_intensity,
                        const float* inv_opsin, JxlHipColorTarget* out);

#ifdef __cplusplus
}
#endif
#endif /* JXL_AMD_H_ */
