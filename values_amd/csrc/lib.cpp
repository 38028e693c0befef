// libvalues_amd.so: version + thread-local error string.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/values_amd.h"

static thread_local char g_err[512] = "";

void vx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static thread_local const char* g_last_kernel = nullptr;
void vx_note_kernel(const char* name) { g_last_kernel = name; }
const char* vx_last_kernel() { return g_last_kernel; }
const char* vx_kname(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  char* p = (char*)malloc(strlen(buf) + 1);   // one per launcher instantiation, never freed
  strcpy(p, buf);
  return p;
}

// ---- configuration: read from the environment exactly once, replaced only by vx_set_config ----
#include <mutex>
#include <stdlib.h>
#include <string.h>

static vx_config g_cfg;
static std::once_flag g_cfg_once;

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  if (!e || !*e) return dflt;
  char* end = nullptr;
  const long v = strtol(e, &end, 0);
  return end == e ? 1 : (int)v;   // VX_S16_NO_DB=yes style switches count as 1
}

static void cfg_from_env() {
  memset(&g_cfg, 0, sizeof(g_cfg));
  g_cfg.conv_fp32 = env_int("VX_CONV_FP32", 0);
  g_cfg.s16_no_prenorm = env_int("VX_S16_NO_PRENORM", 0);
  g_cfg.s16_no_xp8 = env_int("VX_S16_NO_XP8", 0);
  g_cfg.s16_skip_raw = env_int("VX_S16_SKIP_RAW", 1);
  g_cfg.no_head_fusion = env_int("VX_NO_HEAD_FUSION", 0);
  g_cfg.s16_no_upfuse = env_int("VX_S16_NO_UPFUSE", 0);
  g_cfg.s16_no_poolfuse = env_int("VX_S16_NO_POOLFUSE", 0);
  g_cfg.storage16 = env_int("VX_STORAGE16", 0);
  g_cfg.s16_generic = env_int("VX_S16_GENERIC", 0);
  g_cfg.s16_no_zc16 = env_int("VX_S16_NO_ZC16", 0);
  g_cfg.s16_no_halves = env_int("VX_S16_NO_HALVES", 0);
  g_cfg.s16_no_deep = env_int("VX_S16_NO_DEEP", 0);
  g_cfg.s16_no_l1dma = env_int("VX_S16_NO_L1DMA", 0);
  g_cfg.c2s_no_wide = env_int("VX_C2S_NO_WIDE", 0);
  g_cfg.c2s_no_oct = env_int("VX_C2S_NO_OCT", 0);
}

const vx_config& vx_cfg() {
  std::call_once(g_cfg_once, cfg_from_env);
  return g_cfg;
}

extern "C" int vx_get_config(vx_config* out) {
  if (!out) { vx_set_error("vx_get_config: null"); return VX_E_NULL; }
  *out = vx_cfg();
  return VX_OK;
}

extern "C" int vx_set_config(const vx_config* cfg) {
  if (!cfg) { vx_set_error("vx_set_config: null"); return VX_E_NULL; }
  if (cfg->conv_fp32 < 0 || cfg->conv_fp32 > 2) { vx_set_error("vx_set_config: conv_fp32 %d", cfg->conv_fp32); return VX_E_DTYPE; }
  (void)vx_cfg();
  g_cfg = *cfg;
  return VX_OK;
}

extern "C" const char* vx_last_kernel_name(void) { return g_last_kernel ? g_last_kernel : ""; }
extern "C" int vx_version(void) { return 907; /* 0.9.7: vx_val_ssn2d_sums_batched, vx_val_ssn2d_sums_workspace_bytes (the validation reduction of the 2D SSN head, csrc/valstep.hip); 0.9.6: vx_gather_patches_3d, vx_softmax_accumulate_cases, vx_case_composite (the 3D test split on the device: forward batches whose patches come from several cases, csrc/patches3d.hip); 0.9.5: vx_norm_act_drop_pool_route and vx_norm_route_info (the dry run of vx_norm_act_drop_pool and its _bcast / _stats forms: the code the entry point would return before launching, the kernel instance, its grid and its index decode, without touching the HIP runtime; the ten entry points of norm_apply.hip are validate -> route -> launch over csrc/stream3d_route.h; refusals where the size guards used to overflow: INTEGRATION.md); 0.9.4: vx_convT_k2s2_route and vx_convT_route_info (the dry run of vx_convT_k2s2: the code it would return before launching, the kernel it would launch and its grid, without touching the HIP runtime; vx_convT_k2s2 itself is validate -> route -> launch over csrc/convT_route.h; refusals where the size guards used to overflow: INTEGRATION.md); 0.9.3: vx_voxelize_meshes (the toy generator's STL meshes voxelised on the device: column parity with an exact tie rule on ordered edges, float64 with one rounding per operation, labels per mesh, the count of odd columns; capturable, nothing uploaded); 0.9.2: vx_conv2d_route and vx_conv2d_route_info (the dry run of vx_conv2d: the code it would return before launching, the kernel instance it would launch and its launch geometry -- chunks, resident weights, LDS bytes, grid -- without touching the HIP runtime; vx_conv2d itself is validate -> route -> launch over the same host-only routing header, same kernels, same refusals); 0.9.1: vx_pack_conv3d_upfused_zc16, vx_conv3d_upfused_zc16_packed_floats, vx_unet3d_weights.up3_fused appended (upscale3 composed into the weights of expand_2_1's up half; vx_conv3d_args.up_fused is now also taken by the 16-channel z-column kernel, together with acc_in: same instance, same name); 0.9.0: vx_crop_resize_batched, vx_crop_resize_batched_workspace_bytes, vx_p2d_out_size (the GTA / Cityscapes 2D preprocessing on the device: centre crop, cv2.resize's linear and nearest shrink by an even factor, id / colour -> train id tables, palette files gathered through their palette, a batch of mixed sizes and modes in one launch, an item byte-equal alone or in any batch) and vx_png_encode_rgb, vx_png_encode_rgb_workspace_bytes (the PNG encoder fed with RGB bytes; vx_png_encode unchanged); 0.8.9: vx_toy_embed / vx_gauss_blur_axis_f64 / vx_count_ge_f64 / vx_order_stats_f64 / vx_toy_segment / vx_toy_noise (the toy 3D data set generator on the device in float64: the separable Gaussian filter in scipy's order of operations, bit-equal to scipy.ndimage.gaussian_filter; exact float64 order statistics by radix select; rater segmentations from one read; background noise from the library's hash generator); 0.8.8: vx_conv3d_k3_route (the dry run of vx_conv3d_k3: the code it would return before launching and the kernel instance it would launch, without touching the HIP runtime; vx_conv3d_k3 itself is validate -> route -> launch over the same host-only routing header, same kernels, same refusals); 0.8.7: vx_volume_stats_batched / vx_zscore_pad_batched (the 3D preprocessing step on the device: two-pass mean / std / min of a batch of raw volumes of any stored dtype, an item bit-equal alone or in any batch; z-score and pad fused, labels copied with their minimum); 0.8.6: vx_noise_view_3d and vx_tta_views_2d_gen (the TTA noise views drawn on the device from a seed: vx_gauss streams keyed by (seed, global volume / image slot, element), a device seed word for graph replays; view-code bit 5 of the 2D entry); 0.8.5: vx_bn_running_affine (BatchNorm with running statistics as per-channel scale / shift rows, all layers of a model in one launch) and the output epilogue of vx_conv2d (vx_conv2d_args.out_scale / out_shift / out_add / out_add_pitch / out_act appended: fixed affine, residual and ReLU applied as the split-fp16 conv stores, bit-identical to the raw conv followed by vx_affine_gather); 0.8.4: vx_tiff_predict / vx_tiff_lzw_encode / vx_tiff_lzw_pack / vx_tiff_lzw_bound (float32 TIFF maps written as LZW strips on the device: the forward predictors 2 and 3, one wavefront per strip over a hash table in LDS, the strips packed back to back); 0.8.3: vx_tiff_lzw / vx_tiff_unpredict (LZW strips of float32 TIFF maps decoded one wavefront per strip; predictors 2 and 3 undone as a row scan); 0.8.2: vx_one_minus_msr_batched (1 - max softmax for a batch of images whose class planes are separate device arrays, one launch); 0.8.1: the map -> scalar aggregations keep one device path too: the two per-image entry points (the box maximum; the sum and thresholded sum of a map) removed -> vx_aggregate_batched with n_items = 1 (one PATCH spec; one IMAGE or THRESHOLD spec), which gives their numbers bit for bit; it refuses an empty map and a patch whose halo no LDS tile holds, which they took (INTEGRATION.md names them); vx_colorize_u8 moved to png.hip unchanged; 0.8.0: one device path per evaluation score, the per-image entry points removed: vx_ncc_sums -> vx_ncc_batched (n_items = 1; both passes and the means in one call), vx_platt_sums -> vx_platt_sums_batched, vx_calib_bins -> vx_calib_bins_batched, vx_evalmetrics_workspace_bytes -> vx_ncc_batched_workspace_bytes / vx_platt_batched_workspace_bytes / vx_calib_batched_workspace_bytes, vx_select_kth and vx_select_workspace_bytes -> vx_select_segments (one item; both order statistics and the NaN status in one call) and vx_select_segments_workspace_bytes, vx_count_nonzero_u8 -> vx_count_nonzero_batched (one VX_COUNT_B1 item); the remaining calls give the removed ones' numbers bit for bit; 0.7.7: vx_count_nonzero_batched, vx_select_segments and their workspace queries (the threshold search for a batch of masks / all maps of a split in one call each, where the reader left them); 0.7.6: vx_aggregate_batched, vx_aggregate_workspace_bytes (the map -> scalar aggregations of a batch of maps in one call, bit-equal to the per-image entry points of that time); 0.7.5: vx_soft_metric_sums_batched, vx_soft_metric_batched_workspace_bytes (SoftDice + NLL sums of a whole 3D inference step: B volumes in one pass, deterministic and batch-independent); 0.7.4: vx_mask_agreement_batched (class-agreement counts of a whole 2D inference step: B images, up to 32 classes, the ignore label remapped on load); 0.7.3: vx_png_unfilter, vx_png_unfilter_workspace_bytes, vx_rgb_to_trainid (the device reader of the 2D results tree); 0.7.2: vx_inflate, vx_inflate_workspace_bytes (batched gzip / zlib / raw DEFLATE decoder, per-item statuses), vx_nifti_decode, vx_nifti_decode_workspace_bytes (decoded NIfTI payloads to C-order arrays): the device reader of the results tree; 0.7.1: vx_png_encode, vx_png_bound, vx_png_workspace_bytes (device PNG files of label masks: the 2D results writer); 0.7.0: vx_config lost s16_no_upcompose, s16_no_upsplit, s16_no_poolfin, s16_no_presplit, s16_no_dbplain (data-flow switches whose older launch sequences later rounds measured as slower; the kernel paths stay reachable through the arguments); vx_conv3d_k3 refuses in_planar / out_planar where vx_conv3d_k3_planar_ok says 0 before any dispatch; 0.6.0 (round 6): vx_config.s16_no_l1dma, vx_conv3d_args.out_planar / in_planar, vx_conv3d_k3_planar_ok; the dropout generator's key is two words (other masks for a given seed than 0.5.x); 0.5.1 (round 5, second half): vx_config.s16_no_deep, kernel family 7 (Cout % 32 == 0, Cin >= 16: the tile kernel's fragments + the deep-layer kernel's), vx_convT_k2s2 on split-fp16 products for Cin in {64, 128}, vx_stat_src + vx_norm_act_drop_pool_stats / vx_pool_finish_z_stats / vx_prenorm_split_stats; 0.5.0 (round 5): vx_config.s16_no_zc16 / s16_no_halves, vx_conv3d_args.acc_in, vx_unet3d_weights.split_w, vx_pool_finish_z, vx_conv3d_k3_pool_layout, kernel family 6 (Cout = 16, Cin in {8, 16}: the tile kernel's fragments + the z-column kernel's); 0.4.0 (round 4): vx_config lost conv_no_c8, conv_no_xcd, conv_per_cu, s16_per_cu, c8_per_cu, convt_wgs, s16_no_xp, s16_no_db, s16_no_db3, s16_no_epi, s16_no_ty8, s16_no_wall, c2s_no_nt5, convt_no_mfma, s16_range_check, s16_pw, s16_prio (measured-slower variants and tuning knobs, with their instances); + vx_conv3d_k3_presplit_ok; 0.3.3: vx_config.c2s_no_oct, vx_bilinear_softmax_nchw; 0.3.2: vx_config.c2s_no_wide; 0.3.1: vx_prenorm_split, vx_conv3d_args.in_split, vx_config.s16_no_presplit; 0.3.0: vx_config lost conv_dma, s16_ping, s16_dbg, c8_dbg, dma_dbg, dma_nw16, c8_tile16, s16_no_wspec (round 3) */ }
extern "C" const char* vx_last_error_string(void) { return g_err; }
