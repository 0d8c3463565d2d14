// The HIP layer's entry points that libjxl_amd/csrc/api/jxl_api.cc calls, as "no device" doubles for CPU programs built
// around it (api_fuzz.cc, upload_plan_kats.cc, modular_upload_kats.cc): a decoder that reaches them gets an error, which
// is a valid end. KATS_OWN_FRAME_UPLOAD / KATS_OWN_MODULAR_UPLOAD: the including program defines jxlhip_frame_upload /
// jxlhip_modular_upload itself.
extern "C" {
int jxlhip_device_count(void) { return 0; }
int jxlhip_ctx_create(int, JxlHipContext**) { return JXLHIP_ERR_INVALID_ARGUMENT; }
void jxlhip_ctx_destroy(JxlHipContext*) {}
int jxlhip_download_pixels(JxlHipContext*, void*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
#ifndef KATS_OWN_FRAME_UPLOAD
int jxlhip_frame_upload(JxlHipContext*, const JxlHipFrameDesc*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
#endif
int jxlhip_get_errors(JxlHipContext*, uint32_t*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_get_section_end_bits(JxlHipContext*, uint32_t*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_modular_download_buffer(JxlHipContext*, uint32_t, int32_t*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_modular_run(JxlHipContext*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_modular_status(JxlHipContext*, uint32_t*, uint32_t*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
#ifndef KATS_OWN_MODULAR_UPLOAD
int jxlhip_modular_upload(JxlHipContext*, const JxlHipModFrameDesc*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
#endif
int jxlhip_run_entropy(JxlHipContext*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_run_filter_color(JxlHipContext*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_run_transform(JxlHipContext*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_set_alpha(JxlHipContext*, const float*, uint32_t, uint32_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_set_output_format(JxlHipContext*, uint32_t, uint32_t, uint32_t, int) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_set_output_orientation(JxlHipContext*, uint32_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_set_output_unpremultiply(JxlHipContext*, int) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_set_unpremultiply(JxlHipCanvas*, int) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_create(int, uint32_t, uint32_t, uint32_t, uint32_t, JxlHipCanvas**) { return JXLHIP_ERR_INVALID_ARGUMENT; }
void jxlhip_canvas_destroy(JxlHipCanvas*) {}
int jxlhip_canvas_blend(JxlHipCanvas*, JxlHipContext*, const JxlHipBlend*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_download(JxlHipCanvas*, uint32_t, uint32_t, uint32_t, int, uint32_t, void*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_download_alpha(JxlHipCanvas*, float*, size_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_save_xyb(JxlHipCanvas*, JxlHipContext*, uint32_t) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_xyb_source(JxlHipCanvas*, uint32_t, const float**, uint32_t*, uint32_t*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_canvas_xyb_alpha(JxlHipCanvas*, uint32_t, const float**) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_download_alpha(JxlHipContext*, float*) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_upsample_plane(JxlHipContext*, const float*, uint32_t, uint32_t, uint32_t, const float*, uint32_t, uint32_t, int, float*) {
  return JXLHIP_ERR_INVALID_ARGUMENT;
}
int jxlhip_set_option(JxlHipContext*, const char*, int) { return JXLHIP_ERR_INVALID_ARGUMENT; }
int jxlhip_debug_noise(JxlHipContext*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, const float*, float, float, uint32_t, uint32_t,
                       float*, float*) {
  return JXLHIP_ERR_INVALID_ARGUMENT;
}
}
