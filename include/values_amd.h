/*
 * values_amd.h -- C ABI of libvalues_amd.so: the MI355X (gfx950) hot path of ValUES'
 * multi-pass segmentation-uncertainty inference.
 *
 * The reference (IML-DKFZ/values) is pure Python on PyTorch and has no FFI of its own;
 * every entry point below names the reference call site whose device work it replaces.
 * The Python mirror of the reference's interface (the values_amd Python package) binds these with
 * ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = VX_E_* argument error, >0 = hipError_t;
 *     vx_last_error_string() describes the last failure on the calling thread.
 *   - no allocation inside: the caller owns every buffer (device pointers) and passes
 *     an explicit workspace; nothing is freed by the library.
 *   - every launch goes to the caller's stream (hipStream_t passed as void*), nothing
 *     synchronises, so all entry points are capturable into a hipGraph.
 *   - activations inside the library are channels-last ("NDHWC") float32 with an explicit
 *     per-voxel channel pitch; tensors crossing the boundary in the reference's NCDHW
 *     layout are marked so.
 */
#ifndef VALUES_AMD_H
#define VALUES_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vx_stream_t; /* hipStream_t */

enum {
  VX_OK = 0,
  VX_E_NULL = -1,      /* required pointer is null */
  VX_E_SHAPE = -2,     /* unsupported / inconsistent shape */
  VX_E_DTYPE = -3,     /* unsupported dtype / layout / mode enum */
  VX_E_WORKSPACE = -4, /* workspace too small */
  VX_E_ALIGN = -5      /* pointer or pitch not 16-byte aligned */
};

enum { VX_F32 = 0, VX_F64 = 1 };
enum { VX_ACT_NONE = 0, VX_ACT_LRELU = 1 /* slope 0.01 */, VX_ACT_RELU = 2 };
/* dropout (torch.nn.Dropout in training mode, p = 0.5, scale 2):
 *   NONE : identity
 *   HASH : counter-based bit generator keyed by (seed, layer id, sample, element)
 *   MASK : caller-supplied keep-mask, uint8 0/1, channels-last, same geometry as the
 *          tensor it is applied to (parity tests inject the reference's masks) */
enum { VX_DROP_NONE = 0, VX_DROP_HASH = 1, VX_DROP_MASK = 2 };

int vx_version(void);
const char* vx_last_error_string(void);
/* diagnostic: the kernel instance (as rocprofv3 names it) the calling thread's last launch dispatched to, or "" */
const char* vx_last_kernel_name(void);

/* The keep-bits of VX_DROP_HASH as an explicit VX_DROP_MASK mask: mask[n][e] (uint8 0/1) for sample n, channels-last
 * element e = voxel * C + c of dropout layer `layer` (index in DROPOUT order: contr_1_1 .. contr_4_2, center,
 * expand_4_1 .. expand_1_2) under `seed`.  A hash-dropout run can be replayed with explicit masks -- the parity tests
 * hand them to the float64 restatement of unet3D_module.py, so the production bit generator's kernels are what is
 * compared. */
int vx_drop_hash_mask(uint32_t seed, uint32_t layer, int N, int64_t elems_per_sample, uint8_t* mask, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Library configuration: which kernel family runs a layer (and with it the PACKED WEIGHT LAYOUT) plus tuning knobs.
 * Read ONCE from the environment on first use (variable VX_<FIELD NAME IN CAPITALS>, e.g. VX_CONV_FP32=1), never per
 * launch; vx_set_config replaces it (not while launches of another thread are being issued).  Weights are bound to
 * the family they were packed for: see `w_family` in the args structs -- a launch whose weights were packed under a
 * different configuration fails with VX_E_DTYPE instead of computing with the wrong layout. */
typedef struct vx_config {
  int32_t conv_fp32;      /* 0: split-fp16 products on the f16 matrix cores (default); 1: native fp32 matrix kernels (the exact
                             fmaf-chain fallback family: what the fp16 range guard re-runs on); 2: native fp32 only for Cout == 8 layers */
  /* data-flow A/B switches: each selects between kernels / launch sequences that compute the same result, and each is run
   * against the float64 oracle by tests/test_gpu_unet3d.py::test_level0_fusion_variants_vs_oracle_32 */
  int32_t s16_no_prenorm;  /* separate InstanceNorm / LeakyReLU / dropout passes instead of normalise-on-load in the consuming conv */
  int32_t s16_no_xp8;      /* the general tile kernels instead of the z-column kernels on the full-resolution Cout == 8 layers */
  int32_t s16_skip_raw;    /* 1 (default): contr_1_2's raw output goes into the skip half, expand_1_1 normalises it on load */
  int32_t no_head_fusion;  /* separate vx_conv1x1_ncdhw launch instead of the 1x1x1 head in expand_1_2's epilogue */
  int32_t s16_no_upfuse;   /* separate upscale2 launch + concat read instead of the up-convolution fused into expand_1_1 */
  int32_t s16_no_poolfuse; /* separate pooling pass over contr_1_2's output instead of the window maxima from its epilogue */
  int32_t storage16;       /* OPT-IN reduced-precision throughput modes (default 0).  1: expand_1_1's full-resolution output is stored
                              as fp16 and expand_1_2 consumes it unsplit (2 instead of 3 matrix products).  2 (round 6): as 1, and
                              the three full-resolution launches run ONE fp16 product per fp32 product (vx_conv3d_args.products):
                              what BASELINE config 2 calls "bf16".  Maps then differ from the float64 reference by ~1e-3:
                              bench.py --storage16 reports the measured differences of both */
  int32_t s16_generic;     /* the tile kernel's GENERIC instance (run-time epilogue, one LDS image, two barriers per item) wherever a
                              specialised one (compile-time epilogue, double-buffered staggered schedule) would run: the reference
                              of tests/test_gpu_kernels.py::test_conv3d_k3_specialised_instances_equal_generic (bit for bit) */
  int32_t s16_no_zc16;     /* the general tile kernels instead of the role-split z-column kernel (round 5, conv3d_zc16.hip) on the
                              Cout == 16 layers with Cin in {8, 16} and W % 32 == 0; with it the forward also keeps the separate
                              normalise + pool pass of the second contract block */
  int32_t s16_no_halves;   /* expand_2_1 as ONE launch of the tile kernel over the x-blocked concat buffer instead of two launches of the
                              16-channel z-column kernel over its halves (round 5, vx_conv3d_args.acc_in, vx_unet3d_weights.split_w) */
  int32_t s16_no_deep;     /* the general tile kernels instead of the role-split kernel of the deep layers (round 5, conv3d_deep.hip:
                              Cout % 32 == 0, Cin >= 16, volumes of 32^3 voxels and below) */
  int32_t s16_no_l1dma;    /* expand_2_1 -> expand_2_2 as a plain float tensor, staged through registers, instead of the PLANAR pre-split
                              hand-over staged by LDS-DMA (round 6, vx_conv3d_args.out_planar / in_planar) */
  int32_t c2s_no_wide;     /* 2D 3x3 layers of <= 48 input channels: one work item per 16-channel sub-block (round 2) instead of
                              one per tile with all sub-blocks staged together; same bits */
  int32_t c2s_no_oct;      /* 2D 3x3 layers of <= 8 or 17..24 input channels: the sub-block K schedule (5 / 10 steps) instead of
                              the octet-granular one (3 / 7 steps).  Changes the packed layout (vx_conv2d_family) */
} vx_config;
int vx_get_config(vx_config* out);
int vx_set_config(const vx_config* cfg);
/* kernel family (= packed layout) a layer's weights must be packed for under the current configuration; > 0 */
int vx_conv3d_k3_family(int Cin, int Cout);
int vx_conv2d_family(int Cin, int Cout, int KS);

/* ---------------------------------------------------------------------------------
 * K10/K11/K12: fused softmax -> {mean prob, predictive entropy, expected entropy,
 * mutual information, argmax} reduction over T predictions, one pass over the input.
 * Replaces calculate_uncertainty (uncertainty_modeling/test_3D.py:486-518), the mean /
 * argmax of DataCarrier3D.save_data (data_carrier_3D.py:253-255, 281-283) and, with
 * from_logits, the F.softmax of test_3D.py:435,448,472.
 *   x        : [B][T][C][nvox] (planar, the reference's (T,C,*spatial) per volume), f32 or f64
 *   from_logits: 0 = x holds probabilities, 1 = x holds logits (softmax over C fused; C <= 8)
 *   outputs  : per volume b: mean_prob [B][C][nvox] (nullable), pred_entropy / exp_entropy /
 *              mutual_info [B][nvox] f32, argmax [B][nvox] u8 (nullable, first maximal class
 *              like np.argmax), sample_argmax [B][T][nvox] u8 (nullable)
 * NaN products (0 * log 0) are skipped exactly like test_3D.py:493-494, 503-504.
 */
int vx_unc_reduce(const void* x, int dtype, int from_logits, int B, int T, int C, int64_t nvox,
                  float* mean_prob, float* pred_entropy, float* exp_entropy, float* mutual_info,
                  uint8_t* argmax, uint8_t* sample_argmax, vx_stream_t stream);

/* The same pass with its optional extras (all nullable):
 *   variance [B][nvox]: mean over classes of the population variance over the T samples of each class probability
 *            (BASELINE.json north_star's "softmax-variance"; the reference computes none, SURVEY D3: definition is this build's)
 *   in_count [B][nvox]: probabilities are divided by max(count, 1) on load  (sliding-window sums, normalised mode)
 *   out_count[B][nvox]: entropies / MI / mean_prob divided by max(count, 1) on store -- DataCarrier3D.save_data's division
 *            of maps computed on UN-normalised sums (data_carrier_3D.py:323-337); variance by its square */
typedef struct vx_unc_outputs {
  float* mean_prob; float* pred_entropy; float* exp_entropy; float* mutual_info;
  float* variance;
  uint8_t* argmax; uint8_t* sample_argmax;
  const float* in_count; const float* out_count;
} vx_unc_outputs;
int vx_unc_reduce_ex(const void* x, int dtype, int from_logits, int B, int T, int C, int64_t nvox,
                     const vx_unc_outputs* outputs, vx_stream_t stream);

/* The same reduction split for member-/sample-sharded ensembles (BASELINE config C3): every rank
 * ADDS the sufficient statistics of its own passes into stats [B][C+1][nvox] (planes 0..C-1: sum_t p_tc, plane C:
 * sum_t sum_c p_tc log p_tc; zero-initialised by the caller), one sum-reduce over RCCL combines the ranks, and
 * finalize turns the sums of T_total passes into the maps of calculate_uncertainty (test_3D.py:486-518). */
int vx_unc_stats_accumulate(const float* logits, int B, int T, int C, int64_t nvox, float* stats, vx_stream_t stream);
int vx_unc_stats_finalize(const float* stats, int B, int T_total, int C, int64_t nvox, float* mean_prob,
                          float* pred_entropy, float* exp_entropy, float* mutual_info, uint8_t* argmax,
                          vx_stream_t stream);

/* F.softmax(dim=1) of planar logits [R][C][nvox] (test_2D.py:302, 315), for class counts above the fused path's 8. */
int vx_softmax_planar(const float* logits, int64_t R, int C, int64_t nvox, float* out, vx_stream_t stream);

/* calculate_one_minus_msr (test_3D.py:521-525) / ExperimentDataloader.get_max_softmax_pred
 * (evaluation/experiment_dataloader.py:38-49): out[v] = 1 - max_c x[c][v]; x [C][nvox]. */
int vx_one_minus_msr(const void* x, int dtype, int C, int64_t nvox, void* out, vx_stream_t stream);

/* The same score for a whole batch in ONE launch (unc_reduce.hip; DeviceExperimentDataloader's Softmax tree setup, the
 * T = 1 branch of process_output_2d): item i takes its C planes from planes[first_plane .. first_plane + C), separate
 * device arrays of n elements each at any element-aligned address (the tensors the readers return for C files), and
 * out[v] = 1 - max_c planes[c][v] with vx_one_minus_msr's comparison (from plane 0, q > best ? q : best in plane order):
 * every input, NaN and -0.0 included, gives the bits vx_one_minus_msr gives on the same planes stacked contiguously, and
 * an item's result does not depend on its batch mates.  Items may differ in n, C and dtype; an item with n = 0 writes
 * nothing and its pointers are not looked at.  Where an item's planes and out share their 16-byte phase the kernel moves
 * 16 bytes per lane with an element-wise first and last work block, otherwise the item goes element by element; no byte
 * outside [ptr, ptr + n * esize) of a plane or of out is read or written.  Traffic: (C + 1) * n * esize bytes per item.
 * 1 <= n_items <= VX_MSR_MAX_ITEMS, 1 <= n_planes <= VX_MSR_MAX_PLANES; planes may be shared between items.
 * Refused before any device call: a null table, or a null out / plane of an item with n > 0 (VX_E_NULL); n_items or
 * n_planes out of range, n < 0, C < 1, first_plane < 0 or first_plane + C > n_planes (VX_E_SHAPE); an unknown dtype
 * (VX_E_DTYPE); a pointer off its element alignment or a workspace off 16 bytes (VX_E_ALIGN); a short workspace
 * (VX_E_WORKSPACE).  workspace: vx_one_minus_msr_batched_workspace_bytes(n_items, n_planes) bytes, 0 for counts the call
 * refuses.  Both tables go up through a pinned staging buffer inside the call: no wait on the stream (only, if it is
 * still in flight, for the previous call's upload), and the call is not capturable into a hipGraph. */
#define VX_MSR_MAX_ITEMS 65536
#define VX_MSR_MAX_PLANES (1 << 22)
typedef struct vx_msr_item {
  void* out;           /* device, n elements of dtype */
  int64_t n;           /* elements per plane; 0 allowed (then out / planes may be null) */
  int32_t first_plane; /* index into planes[] */
  int32_t C;           /* >= 1 planes: planes[first_plane .. first_plane + C) */
  int32_t dtype;       /* VX_F32 | VX_F64: the planes and out */
  int32_t reserved;
} vx_msr_item;
int64_t vx_one_minus_msr_batched_workspace_bytes(int n_items, int n_planes);
int vx_one_minus_msr_batched(const vx_msr_item* items /* host */, int n_items,
                             const void* const* planes /* host array of device pointers */, int n_planes, void* workspace,
                             int64_t ws_bytes, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Weight packing (one-off, at checkpoint load: load_models_from_checkpoint, test_3D.py:222-247).
 *   conv3d  : torch (Cout, Cin, 3,3,3) f32 -> MFMA fragment order; returns floats needed via *_size
 *   convT   : torch (Cin, Cout, 2,2,2) f32 -> [dz][dy][ci][dx][co]
 */
int64_t vx_conv3d_k3_packed_floats(int Cin, int Cout);
int vx_pack_conv3d_k3(const float* w_torch, float* w_packed, int Cin, int Cout, vx_stream_t stream);
int64_t vx_convT_k2s2_packed_floats(int Cin, int Cout);
int vx_pack_convT_k2s2(const float* w_torch, float* w_packed, int Cin, int Cout, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * K1 (+K3,K4 epilogue, K2 statistics): 3x3x3 convolution, padding 1, channels-last.
 * Replaces nn.Conv3d(k=3,p=1) of the contract / expand / center blocks
 * (models/unet3D_module.py:233, 264, 99-111) with its trailing LeakyReLU / ReLU / Dropout
 * fused when the block has no norm, and with the InstanceNorm statistics (per sample and
 * channel sum / sum of squares per workgroup tile, deterministic, no atomics) emitted
 * for vx_instnorm_finalize when it has.
 */
typedef struct vx_conv3d_args {
  const float* in;      /* in_xblk == 0: [N][D][H][W][in_pitch], channels [0, Cin) used; Cin % 8 == 0
                         * in_xblk  > 0: x-blocked concat buffer [N][D][H][W/xb][2][xb][Cin/2] (see vx_concat layout) */
  const float* w_packed;
  const float* bias;    /* [Cout] */
  float* out;           /* [N][D][H][W][out_pitch], written at channel offset out_coff */
  int32_t in_pitch, out_pitch, out_coff;
  int32_t N, D, H, W, Cin, Cout; /* Cout % 8 == 0 */
  int32_t act;          /* VX_ACT_* applied after bias */
  int32_t drop_mode;    /* VX_DROP_* applied after act */
  uint32_t drop_seed, drop_layer;
  const uint8_t* drop_mask; /* [N][D][H][W][Cout] when VX_DROP_MASK */
  float* stats_partial; /* nullable: [N][ntiles][Cout][2] (sum, sumsq of out before act) */
  int32_t in_xblk;      /* 0 = plain input; 1, 2 or 4 = x-block size of a concat input */
  int32_t w_family;     /* vx_conv3d_k3_family(Cin, Cout) at the time w_packed was packed */
  /* Optional fused head (only where vx_conv3d_k3_head_fusable(Cin, Cout)): the 1x1x1 conv of
   * vx_conv1x1_ncdhw applied to this layer's output (after act / dropout) in the epilogue, same
   * arguments and the same bits; `out` may then be NULL and the feature map is never stored. */
  float* head_out;      /* nullable: [slots][head_C][D][H][W] */
  const float* head_w;  /* torch (head_C, Cout, 1,1,1) */
  const float* head_b;  /* [head_C] */
  const int32_t* head_dst;  /* nullable: slot of sample n (default n) */
  const int32_t* head_flip; /* nullable: un-flip code of sample n (bit 0 z, 1 y, 2 x) */
  int32_t head_C;       /* 1 .. 8 */
  /* Optional PROLOGUE (only where vx_conv3d_k3_prologue_ok(D, H, W, Cin, Cout)): the input -- or, for a concat input,
   * its skip half -- is the RAW output of a contract block's conv (unet3D_module.py:231-237); InstanceNorm with the
   * given statistics, LeakyReLU and the block's dropout are applied while the tile is staged, so the normalised tensor
   * is never written.  in_repeat > 1: sample n reads input sample / statistics row n / in_repeat (the T MC-dropout
   * samples of a volume share the first block's conv output; the dropout bits are those of sample n). */
  const float* in_mean; const float* in_rstd;   /* nullable together: [N / in_repeat][8] */
  int32_t in_drop_mode; uint32_t in_drop_seed, in_drop_layer;   /* VX_DROP_NONE | VX_DROP_HASH of the producing block */
  int32_t in_repeat;    /* 0 or 1: sample n reads input sample n */
  int32_t out_xblk, out_half; /* out_xblk > 0: `out` is a concat buffer, this conv writes its half out_half (as vx_norm_args) */
  uint32_t* range_flag; /* nullable device word: atomic max of the bit patterns of the |stored values| that reach 32768 (fp16
                           range guard of the split-fp16 consumers: anything >= 65504 must not reach them; smaller
                           magnitudes are not reported -- the word stays 0 for an ordinary tensor) */
  const uint32_t* seed_dev; /* nullable device word ADDED to drop_seed / in_drop_seed at run time (a captured hipGraph
                               replays with the arguments it was captured with; fresh dropout bits per replay = update
                               this word).  Same field in vx_norm_args / vx_convT_args / vx_unet3d_run. */
  /* Optional fused UP-CONVOLUTION (only where vx_conv3d_k3_upfuse_ok(D, H, W, Cin, Cout)): the decoder's
   * upscale -> torch.cat([up, skip], 1) -> expand (unet3D_module.py:332-356) in one kernel.  Channels [0, 8) of the
   * conv's input are ConvTranspose3d(16 -> 8, k = 2, s = 2)(up_in) + up_b, computed while the tiles are staged and never
   * stored; `in` then holds only the skip half: the concat buffer as before (in_xblk > 0, its up half is not read) or a
   * plain [N][D][H][W][in_pitch] tensor whose channels [0, 8) are the skip (in_xblk == 0).  The prologue fields apply to
   * the skip half.  range_flag also covers the up values. */
  const float* up_in;   /* nullable: [N][D/2][H/2][W/2][up_pitch], channels [0, 16) used */
  const float* up_w;    /* vx_pack_convT_k2s2(Cin = 16, Cout = 8) */
  const float* up_b;    /* [8] */
  int32_t up_pitch;
  /* Optional POOLED OUTPUT of a contract block's second conv (only where vx_conv3d_k3_poolfuse_ok(D, H, W, Cin, Cout);
   * needs stats_partial): besides its raw output and statistics the conv leaves what the block's
   * InstanceNorm -> LeakyReLU -> Dropout -> MaxPool3d(2, 2) (unet3D_module.py:231-237, 303-310) needs of every 2 x 2 x 2
   * window: the maximum over the raw values the dropout KEEPS (drop_mode / drop_seed / drop_layer describe that dropout;
   * -inf when none is kept) and an any-dropped bit per channel.  vx_pool_finish turns them into the pooled tensor once the
   * statistics exist -- the full-resolution tensor is not read again. */
  float* pool_out;      /* nullable: [N][D/2][H/2][W/2][8] raw window maxima (layout 2 of vx_conv3d_k3_pool_layout: [N][D][H/2][W/2][16]) */
  uint32_t* pool_flags; /* [N][D/2][H/2][W/2][2]: bit j of word q = a dropped element of channel 4 q + j in the window (layout 2: [..][4]) */
  /* PRE-SPLIT input (only with in_repeat > 1 where vx_conv3d_k3_prologue_ok): `in` is the output of vx_prenorm_split --
   * the shared raw tensor already normalised, activated and split into fp16 (hi, lo) pairs, ONCE per volume; the prologue
   * then only applies sample n's dropout bits (in_drop_*) while the tile is staged.  in_mean / in_rstd are not read. */
  int32_t in_split;
  /* Reduced-storage mode (vx_config.storage16; opt-in, NOT the default: an activation rounded to fp16 cannot meet the 1e-4
   * parity of the maps): out_f16 -- the LeakyReLU + dropout epilogue stores fp16 (out_pitch counts halves); in_f16 -- the
   * dense 8-channel input is such a tensor: it is copied into the hi plane unsplit and the lo-activation product is skipped. */
  int32_t out_f16, in_f16;
  /* PRE-SPLIT hand-over of the coarse tensor of the fused up-convolution: out_split -- the (tile-kernel) epilogue stores
   * every 16-byte piece as [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3] fp16 (the layout of vx_prenorm_split) instead of four floats;
   * up_split -- up_in is such a tensor: the staging waves take the matrix operands as they are (each coarse voxel was split
   * by four waves per step before).  Same values, same bits. */
  int32_t out_split, up_split;
  /* COMPOSED up-convolution (round 4; with up_in, optional): the output of vx_pack_conv3d_upfused for this layer's weights and
   * the transposed conv's.  ConvTranspose3d(k = 2, s = 2) has no activation behind it (unet3D_module.py:157-190, 332-356), so
   * conv(cat([up, skip])) = conv_skip(skip) + (W_up-half o U)(coarse) + bias terms: per output parity class (z & 1, y & 1)
   * the up half of the 3x3x3 conv composed with the transposed conv is a 2 x 2 x 3 (x-pair) tap convolution over the 16
   * COARSE channels -- K = 192 instead of 288 per x-pair row, and the staging waves copy the coarse tensor into LDS instead
   * of evaluating the transposed conv per step.  The up bias enters through a table of the 27 border classes (a 3x3x3 tap
   * outside the volume sees the zero padding of the concatenated tensor, not the bias).  Same function of the inputs;
   * weights composed in float64 at pack time, so results differ from the two-stage evaluation by float32 rounding only.
   * Level 1 (the 16-channel z-column kernel, form 2 of vx_conv3d_k3_upfuse_ok; only together with acc_in): the output of
   * vx_pack_conv3d_upfused_zc16 -- per parity class (z & 1, y & 1, x & 1) a 2 x 2 x 2 tap convolution over the 32 coarse channels,
   * 8 K-steps instead of 14 + the staging waves' products; up_w is not read then.  Same kernel instance, same name. */
  const float* up_fused;
  /* POOL-FINISH on load (round 4; only where vx_conv3d_k3_poolfin_ok(Cin, Cout)): `in` is the pool_out of the previous block's
   * second conv -- window maxima of RAW values [N][D][H][W][8] -- and in_pool_flags its any-dropped words [N][D][H][W][2];
   * in_mean / in_rstd are that block's statistics ([N][8]) and in_drop_mode says whether the dropout's factor 2 applies.  The conv
   * evaluates vx_pool_finish's arithmetic (same expressions, same order) while it stages its tiles: the pooled tensor is never
   * written.  in_repeat / in_split / in_drop_seed are not used.  Only with the plain epilogue of a contract block's first conv
   * (act NONE, no dropout, no head; Cout % 32 != 0): anything else is refused with VX_E_SHAPE. */
  const uint32_t* in_pool_flags;
  /* PARTIAL SUMS (round 5; the 16-channel z-column kernel with an activation epilogue, vx_conv3d_k3_acc_ok): acc_in
   * [N][D][H][W][acc_pitch] (channels [0, Cout)) is added to the conv's result BEFORE the activation / dropout, and `bias` is
   * NOT added (it is part of the partial sums).  A conv over a channel concatenation = the sum of the convs over its parts: the
   * decoder's first conv of level 1 runs as conv(skip half) + bias -> partial, then conv(up half) + partial -> activation
   * (unet3D_module.py:332-356 without the concatenated tensor).  acc_in may alias `out` (every lane reads the pieces it writes). */
  const float* acc_in;
  int32_t acc_pitch;
  /* PLANAR PRE-SPLIT hand-over between two 16-channel layers of the z-column kernel (round 6; only where
   * vx_conv3d_k3_planar_ok(D, H, W, Cin, Cout): the decoder's expand_2_1 -> expand_2_2, unet3D_module.py:263-267, with no
   * normalisation between them).  out_planar: the activation epilogue stores its 16 channels as fp16 (hi, lo) pairs -- the
   * split the consumer's matrix instructions take -- in the consumer's LDS row order:
   *     [N][D][H][octet 2][hi | lo][W][8 halves]          (64 W bytes per row, as the float tensor; out_pitch == 16, out_coff == 0)
   * in_planar: `in` is such a tensor: the staging waves move it into the LDS image by buffer_load ... lds (one instruction per
   * 64 positions, the zero padding as out-of-range lanes) -- no registers, no conversion, no ds_write.  Same values, same
   * products, same bits as the float hand-over.  `out` must not alias acc_in (another layout). */
  int32_t out_planar, in_planar;
  /* Opt-in throughput mode (vx_config.storage16 = 2; never the default, outside the 1e-4 parity bar): products = 1 -- ONE fp16
   * product per fp32 product (activations and weights rounded to fp16, fp32 accumulation) instead of the three of the split
   * scheme.  Exists for the three full-resolution launches of the MC-dropout forward (contr_1_2 on the pre-split tensor,
   * upscale2 composed into expand_1_1, expand_1_2 + head on the fp16 tensor); anything else is refused.  0 = the default. */
  int32_t products;
} vx_conv3d_args;
int64_t vx_conv3d_upfused_packed_floats(void);
/* w1_torch (8, 16, 3,3,3) + b1 (8): the decoder conv whose input channels [0, 8) are the up half; up_w_torch (16, 8, 2,2,2) +
 * up_b (8): the transposed conv (torch layouts, device pointers) -> packed [4 classes][6 K-steps][hi | lo][64 lanes][8 halves]
 * + bias table [27][8] (vx_conv3d_upfused_packed_floats() floats, 16-byte aligned).  The composition runs on the device in
 * float64; a composed weight beyond the fp16 range has its hi part clamped to +-65504 like vx_pack_conv3d_k3's, i.e. the
 * consuming conv then produces inf / NaN loudly.  The B operands of the composed products are the COARSE tensor's values:
 * its producer's range_flag is what guards them (the up values themselves are never formed). */
int vx_pack_conv3d_upfused(const float* w1_torch, const float* b1, const float* up_w_torch, const float* up_b, float* packed,
                           vx_stream_t stream);
int vx_conv3d_k3_prologue_ok(int D, int H, int W, int Cin, int Cout); /* 1 if vx_conv3d_k3 takes in_mean for this layer */
int vx_conv3d_k3_upfuse_ok(int D, int H, int W, int Cin, int Cout);   /* != 0 if vx_conv3d_k3 takes up_in for this layer: 1 the form
   above (16 -> 8 at full resolution); 2 (round 5, the 16-channel z-column kernel): ALL 16 input channels are
   ConvTranspose3d(32 -> 16, k = 2, s = 2)(up_in) + up_b, evaluated while the tiles are staged -- `in` is not read, up_in is
   [N][D/2][H/2][W/2][up_pitch >= 32], up_w the output of vx_pack_convT_zc16, up_split as above; combines with acc_in */
int64_t vx_convT_zc16_packed_floats(void);
/* upscale3 composed into expand_2_1's up half.  w1_torch (16, 32, 3,3,3): the layer's FULL weight (its input channels [0, 16) are
 * the up half); up_w_torch (32, 16, 2,2,2) + up_b (16): the transposed conv (torch layouts, device pointers) -> packed
 * [8 classes (pz, py, px)][8 taps (a, b, c)][hi | lo][64 lanes][8 halves] + the up-bias table [27 border classes][16] fp32
 * (vx_conv3d_upfused_zc16_packed_floats() floats, 16-byte aligned).  Composed on the device in float64 (csrc/upcompose16.h), split
 * and clamped like vx_pack_conv3d_k3's weights.  The layer's bias is not part of it: it rides in the partial sums (acc_in). */
int64_t vx_conv3d_upfused_zc16_packed_floats(void);
int vx_pack_conv3d_upfused_zc16(const float* w1_torch, const float* up_w_torch, const float* up_b, float* packed, vx_stream_t stream);
int vx_pack_convT_zc16(const float* w_torch /* (32, 16, 2,2,2) */, float* packed, vx_stream_t stream);
/* 1 if vx_conv3d_k3 takes in_mean for the SKIP half of an x-blocked concat input (in_xblk = xblk) of this layer: the decoder's
 * first conv of a level normalising the contract block's raw output on load (round 5: also the tile kernel, Cin % 32 == 0) */
int vx_conv3d_k3_skip_prologue_ok(int D, int H, int W, int Cin, int Cout, int xblk);
int vx_conv3d_k3_acc_ok(int D, int H, int W, int Cin, int Cout);      /* 1 if vx_conv3d_k3 takes acc_in for this layer */
int vx_conv3d_k3_planar_ok(int D, int H, int W, int Cin, int Cout);   /* 1 if vx_conv3d_k3 takes in_planar / out_planar for this layer */
int vx_conv3d_k3_poolfuse_ok(int D, int H, int W, int Cin, int Cout); /* 1 if vx_conv3d_k3 takes pool_out for this layer */
int vx_conv3d_k3_presplit_ok(int D, int H, int W, int Cin, int Cout); /* 1 if vx_conv3d_k3 takes in_split (vx_prenorm_split's output) for this layer */
int vx_conv3d_k3_poolfin_ok(int Cin, int Cout);                       /* 1 if vx_conv3d_k3 takes in_pool_flags for this layer */
/* pooled[c] = any_dropped ? max(s f(m), 0) : s f(m) with f(m) = LeakyReLU((m - mean[n][c]) * rstd[n][c]), s = 2 with
 * dropout (drop_scale2 != 0) else 1: the MaxPool3d(2, 2) of Dropout(LeakyReLU(InstanceNorm(x))) from the window maxima and
 * flags vx_conv3d_k3 left in pool_out / pool_flags (bit-identical to pooling the normalised tensor: f is monotone). */
/* In place: x [N][nvox][8] fp32 -> per 16-byte piece (4 channels) [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3] fp16 with
 * y = scale * LeakyReLU((x - mean[n][c]) * rstd[n][c]) = hi + lo * 2^-11 (the split the fp16 matrix kernels consume; scale = 2
 * folds a following p = 0.5 dropout's factor).  For the MC-dropout batch of test_3D.py:462-472: the T samples of a volume
 * share the first block's conv output (InstanceNorm + LeakyReLU of unet3D_module.py:231-237 are the same for all of them,
 * only the dropout bits differ), so this runs once per VOLUME and contr_1_2 (vx_conv3d_args.in_split) masks per sample. */
int vx_prenorm_split(float* x, const float* mean, const float* rstd, int N, int64_t nvox, float scale, vx_stream_t stream);
int vx_pool_finish(const float* pool_raw, const uint32_t* pool_flags, const float* mean, const float* rstd, float* out,
                   int out_pitch, int N, int64_t voxels_per_sample, int drop_scale2, vx_stream_t stream);
/* The same for the 16-channel z-column kernel (round 5; vx_conv3d_k3_pool_layout(...) == 2): its epilogue pools the (y, x) half of
 * every 2 x 2 x 2 window -- pool_raw [N][2 Dp][Hp Wp][16] window maxima of one z-plane each, pool_flags [N][2 Dp][Hp Wp][4] (bit j
 * of word q: a dropped element of channel 4 q + j) -- and this pass takes the maximum / the OR over the z pair before the same
 * arithmetic: out [N][Dp][Hp Wp][out_pitch >= 16].  Bit-identical to pooling the normalised tensor. */
int vx_pool_finish_z(const float* pool_raw, const uint32_t* pool_flags, const float* mean, const float* rstd, float* out,
                     int out_pitch, int N, int Dp, int64_t plane_voxels, int drop_scale2, vx_stream_t stream);
/* layout of pool_out / pool_flags for a layer that takes them (vx_conv3d_k3_poolfuse_ok): 1 = [N][D/2][H/2][W/2][8] + [..][2]
 * (the 8-channel z-column kernel: whole windows), 2 = [N][D][H/2][W/2][16] + [..][4] (the 16-channel one: the z pair is left to
 * vx_pool_finish_z), 0 = no pooled output */
int vx_conv3d_k3_pool_layout(int D, int H, int W, int Cin, int Cout);
/* The decoder's concat buffer (torch.cat([up, skip], 1), unet3D_module.py:332-356) is never materialised as an
 * interleaved tensor: CAT[N][D][H][W/xb][2][xb][C] keeps the up half (s = 0, written by vx_convT_k2s2) and the
 * skip half (s = 1, written by vx_norm_act_drop_pool) as alternating DENSE blocks of xb voxels, so both producers
 * write whole cache lines and the consumer conv reads it through in_xblk.  xb = largest of {4,2,1} dividing W. */
int vx_conv3d_k3_tiles(int D, int H, int W);  /* upper bound of ntiles per sample (stats_partial sizing) */
int vx_conv3d_k3_tiles_for(int D, int H, int W, int Cout); /* exact ntiles for a given Cout (finalize) */
int vx_conv3d_k3(const vx_conv3d_args* a, vx_stream_t stream);
int vx_conv3d_k3_head_fusable(int Cin, int Cout); /* 1 if the layer's kernel can take head_out */
/* Dry run of vx_conv3d_k3: every argument check and the choice of the kernel, no launch and no call into the HIP runtime (works
 * without a GPU; the pointers are only tested for null and alignment).  Returns the VX_E_* code vx_conv3d_k3 would refuse the call
 * with (message in vx_last_error_string), or VX_OK with the instance name vx_last_kernel_name() would report after the launch in
 * kernel_name (nullable; at most cap bytes, always terminated). */
int vx_conv3d_k3_route(const vx_conv3d_args* a, char* kernel_name, int cap);

/* First layer, Cin == 1 (contr_1_1): input is the reference's (V,1,D,H,W) volume batch.
 * Sample n reads volume src[n] (nullable: n / repeat) with flip code flip[n] (nullable: 0;
 * bit0 = flip D, bit1 = flip H, bit2 = flip W -- torch.flip dims 2,3,4 of test_3D.py:430,445). */
int vx_conv3d_k3_c1_tiles(int D, int H, int W); /* ntiles per sample of this kernel's stats_partial */
int vx_conv3d_k3_c1(const float* in, const float* w_torch /* (Cout,1,3,3,3) */, const float* bias, float* out,
                    int out_pitch, int N, int D, int H, int W, int Cout, int repeat, const int32_t* src,
                    const int32_t* flip, float* stats_partial, vx_stream_t stream);

/* in_channels > 1 (unet3D_module.py:8-35): (V, Cin, D, H, W) -> channels-last [N][D][H][W][8] (channels Cin..7 zero) for
 * the general 3x3x3 kernels, with the per-sample source volume / TTA flip of vx_conv3d_k3_c1.  1 <= Cin <= 8. */
int vx_pack_input_cl8(const float* in, float* out, int N, int Cin, int D, int H, int W, int repeat, const int32_t* src,
                      const int32_t* flip, vx_stream_t stream);

/* K2: reduce stats_partial -> mean[N][C], rstd[N][C] (biased variance, eps 1e-5:
 * nn.InstanceNorm3d defaults, unet3D_module.py:234). */
int vx_instnorm_finalize(const float* stats_partial, int N, int ntiles, int C, int64_t nvox, float eps,
                         float* mean, float* rstd, vx_stream_t stream);

/* K2+K3+K4(+K5,K7): y = Dropout(LeakyReLU((x - mean) * rstd)) written to `out` (any pitch /
 * channel offset: the skip half of the decoder's concat buffer, unet3D_module.py:332-356)
 * and, if pool_out != NULL, MaxPool3d(2,2) of y (unet3D_module.py:50, 314-323). */
typedef struct vx_norm_args {
  const float* x; int32_t x_pitch;
  const float* mean; const float* rstd; /* nullable both: no normalisation */
  float* out; int32_t out_pitch, out_coff;
  float* pool_out; int32_t pool_pitch;
  int32_t N, D, H, W, C;
  int32_t act, drop_mode; uint32_t drop_seed, drop_layer; const uint8_t* drop_mask;
  int32_t out_xblk, out_half; /* out_xblk > 0: `out` is a concat buffer (xb = out_xblk), this kernel writes half
                                 out_half (0 = up, 1 = skip); out_pitch / out_coff are then ignored */
  int32_t x_xblk, x_half;     /* x_xblk > 0: `x` is half x_half of a concat buffer (a conv that wrote its raw output
                                 straight into the skip half); x_pitch is then ignored.  With pool_out set, `out` may be
                                 NULL: only the pooled tensor is produced (the consumer conv normalises the skip half
                                 itself, vx_conv3d_args.in_mean) */
  const uint32_t* seed_dev;   /* as in vx_conv3d_args */
  uint32_t* range_flag;       /* nullable, as in vx_conv3d_args: set where this pass does NOT normalise (do_instancenorm=False:
                                 the first layer's activation / dropout pass feeds a split-fp16 conv un-normalised).  The
                                 per-sample kernels report the largest |stored value| (the dropout's 2 included, a dropped
                                 element counts as 0); vx_norm_act_drop_pool_bcast without pooling reports twice the largest
                                 |activation| whatever the masks hold: an upper bound of what its samples store */
} vx_norm_args;
int vx_norm_act_drop_pool(const vx_norm_args* a, vx_stream_t stream);
/* Round 5: a streaming pass that takes its InstanceNorm statistics from the producing conv's PARTIALS instead of from a
 * vx_instnorm_finalize launch in front of it: every workgroup reduces the partials of its sample itself (float64, the formula of
 * vx_instnorm_finalize; the summation order differs, so mean / rstd agree with it to the last bit except on a rounding
 * boundary) and mean_out / rstd_out [N][C] (nullable) receive them for later readers.  stats_partial [N][tiles][C][2] as
 * vx_conv3d_args.stats_partial, count = voxels per sample the sums run over, C <= 512. */
typedef struct vx_stat_src {
  const float* stats_partial; int32_t tiles; float eps; int64_t count;
  float* mean_out; float* rstd_out;
} vx_stat_src;
/* vx_norm_act_drop_pool with a->mean == a->rstd == NULL and the statistics from `st` (x_repeat 1) */
int vx_norm_act_drop_pool_stats(const vx_norm_args* a, const vx_stat_src* st, vx_stream_t stream);
/* vx_prenorm_split / vx_pool_finish_z (above) with the statistics from `st` (C = 8 / 16) */
int vx_prenorm_split_stats(float* x, const vx_stat_src* st, int N, int64_t nvox, float scale, vx_stream_t stream);
/* Zero `bytes` bytes at a device pointer, in stream order (hipMemsetAsync).  The host mirrors allocate with torch.empty and fill
 * through this entry: the persistent zero-padded activation tensors of the 2D walk (channels [C, round4(C)) of a padded layer,
 * hrnet_module.py:37-41 with widths that are no multiple of 4) and the padded BatchNorm scale / shift rows are written ONCE per
 * geometry -- no ATen fill kernel runs on the product's paths (round-5 verdict, weak #13). */
int vx_zero(void* p, int64_t bytes, vx_stream_t stream);
int vx_pool_finish_z_stats(const float* pool_raw, const uint32_t* pool_flags, const vx_stat_src* st, float* out, int out_pitch,
                           int N, int Dp, int64_t plane_voxels, int drop_scale2, vx_stream_t stream);
/* Same, but sample n of the OUTPUT reads sample n / x_repeat of x / mean / rstd: the T MC-dropout samples of a
 * volume share contr_1_1's conv output and statistics (test_3D.py:462-472 feeds the same input T times; dropout
 * is the first thing that differs), so that conv runs once per volume and this kernel fans it out.  At most 65535 samples per
 * launch; without pooling (the fan-out kernel) the limit is on the N / x_repeat SOURCE samples. */
int vx_norm_act_drop_pool_bcast(const vx_norm_args* a, int x_repeat, vx_stream_t stream);
/* Dry run of vx_norm_act_drop_pool (x_repeat 1, st NULL), _bcast (x_repeat) and _stats (st): every argument check, the choice of the
 * kernel instance, its grid and its index decode, no launch and no call into the HIP runtime (works without a GPU; the pointers are only
 * tested for null).  Returns the VX_E_* code the entry point would refuse the call with (message in vx_last_error_string), or VX_OK
 * with the name vx_last_kernel_name() would report after the launch in kernel_name (nullable; at most cap bytes, always terminated) and
 * the geometry in info (nullable). */
typedef struct vx_norm_route_info {
  int32_t grid_x, grid_y;        /* workgroups walking a sample's pieces (grid stride); samples (the fan-out kernel: source samples) */
  uint32_t per_sample;           /* 16-byte pieces (work items) of one sample */
  uint32_t magic_pw, magic_c4, magic_rh; /* multiply-high magics of the piece decode: / pieces per row, / (C / 4), / rows per plane (0: divisor 1) */
} vx_norm_route_info;
int vx_norm_act_drop_pool_route(const vx_norm_args* a, int x_repeat, const vx_stat_src* st, char* kernel_name, int cap,
                                vx_norm_route_info* info);

/* K6: ConvTranspose3d(k=2, s=2) (+ReLU+Dropout for center.4), unet3D_module.py:113-120, 157-190;
 * writes channels [out_coff, out_coff+Cout) of the concat buffer (K7: torch.cat disappears).
 * Cin in {64, 128} (any Cout the entry point takes: a multiple of 8) under vx_config.conv_fp32 == 0 (round 5): the products run on the fp16 matrix
 * cores by operand splitting, like the 3x3x3 convolutions -- same accuracy, and the same contract on the INPUT: |x| < 65504
 * (the producers inside vx_unet3d_forward record it in their range_flag).  A WEIGHT past 65504 is reported through this launch's
 * range_flag (infinity).  conv_fp32 != 0 keeps the native-fp32 instruction. */
typedef struct vx_convT_args {
  const float* in; int32_t in_pitch;
  const float* w_packed; const float* bias;
  float* out; int32_t out_pitch, out_coff;
  int32_t N, D, H, W, Cin, Cout; /* input dims; output is 2D x 2H x 2W */
  int32_t act, drop_mode; uint32_t drop_seed, drop_layer; const uint8_t* drop_mask; /* mask [N][2D][2H][2W][Cout] */
  int32_t out_xblk, out_half; /* as in vx_norm_args: write half out_half of a concat buffer */
  uint32_t* range_flag;       /* nullable: as in vx_conv3d_args.  Recorded by the matrix-core kernels (Cin in {16,32,64,128}) and
                                 by the row-streaming kernel that takes Cin 16 / 32 past their decode bound; a launch that
                                 vx_convT_k2s2_route sends to the generic kernel (any other Cin, or Cin 16 / 32 past the bound
                                 with a Cout outside {8,16,32,64,128}) leaves the word alone */
  const uint32_t* seed_dev;   /* as in vx_conv3d_args */
} vx_convT_args;
int vx_convT_k2s2(const vx_convT_args* a, vx_stream_t stream);
/* Dry run of vx_convT_k2s2: every argument check, the choice of the kernel and its grid, no launch and no call into the HIP runtime
 * (works without a GPU; the pointers are only tested for null).  Returns the VX_E_* code vx_convT_k2s2 would refuse the call with
 * (message in vx_last_error_string), or VX_OK with the name vx_last_kernel_name() would report after the launch in kernel_name
 * (nullable; at most cap bytes, always terminated) and the grid in info (nullable). */
typedef struct vx_convT_route_info {
  int32_t grid_x, grid_y; /* workgroups walking the input (grid stride); groups of output rows */
} vx_convT_route_info;
int vx_convT_k2s2_route(const vx_convT_args* a, char* kernel_name, int cap, vx_convT_route_info* info);

/* K8 (+K13): final 1x1x1 conv (unet3D_module.py:199, 365) -> logits in the reference's NCDHW
 * layout, sample n written to slot dst[n] (nullable: n) of out [slots][C][D][H][W], un-flipped by
 * flip[n] (test_3D.py:445-447). w: torch (C, F, 1,1,1). */
int vx_conv1x1_ncdhw(const float* in, int in_pitch, const float* w, const float* bias, float* out, int N, int D,
                     int H, int W, int F, int C, const int32_t* dst, const int32_t* flip, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Whole-network launch: UNet3D.forward (unet3D_module.py:296-373) for N samples.
 */
typedef struct vx_unet3d_weights {
  /* packed 3x3x3 convs in execution order:
   * contr_1_1(torch layout, Cin==1) contr_1_2 contr_2_1 contr_2_2 contr_3_1 contr_3_2 contr_4_1 contr_4_2
   * center.0 center.2 expand_4_1 expand_4_2 expand_3_1 expand_3_2 expand_2_1 expand_2_2 expand_1_1 expand_1_2 */
  const float* conv_w[18];
  const float* conv_b[18];
  /* packed transposed convs: center.4 upscale4 upscale3 upscale2 */
  const float* up_w[4];
  const float* up_b[4];
  const float* final_w; /* torch (C, F) */
  const float* final_b;
  int32_t F;            /* initial_filter_size */
  int32_t num_classes;
  int32_t conv_family[18]; /* vx_conv3d_k3_family of each packed conv at pack time (entry 0, the Cin == 1 layer: 0) */
  int32_t in_channels;     /* 0 or 1: conv_w[0] is the torch layout of a Cin == 1 layer (vx_conv3d_k3_c1); 2 .. 8: conv_w[0]
                              is PACKED for Cin = 8 (weights zero-padded), the input goes through vx_pack_input_cl8 */
  int32_t no_instancenorm; /* 1: do_instancenorm=False -- contract blocks are conv + LeakyReLU + Dropout (unet3D_module.py:238-243) */
  const float* up_fused;   /* nullable: vx_pack_conv3d_upfused(expand_1_1, upscale2) -- the level-0 up-convolution composed into
                              expand_1_1 (vx_conv3d_args.up_fused); NULL: evaluated per step by the staging waves (round 2) */
  /* (round 5) nullable: expand_2_1's weights as TWO packed 16 -> 16 convs, [0] = input channels [0, 16) (the up half), [1] =
   * channels [16, 32) (the skip half), each vx_pack_conv3d_k3(16, 16) of the contiguous slice: the layer then runs as two
   * launches of the 16-channel z-column kernel (vx_conv3d_args.acc_in) without a concatenated tensor.  F = 8 networks only. */
  const float* split_w[2];
  int32_t split_family;    /* vx_conv3d_k3_family(16, 16) at pack time */
  const float* up3_zc16;   /* nullable: vx_pack_convT_zc16(upscale3): the up half's launch evaluates the transposed conv itself */
  const float* up3_fused;  /* nullable (with up3_zc16): vx_pack_conv3d_upfused_zc16(expand_2_1, upscale3) -- upscale3 composed into the
                              up half's weights (vx_conv3d_args.up_fused); NULL: evaluated per step by the staging waves */
} vx_unet3d_weights;

typedef struct vx_unet3d_run {
  const float* x;        /* (V,1,D,H,W) */
  int32_t N, D, H, W;    /* N samples; D,H,W multiples of 16 */
  int32_t repeat;        /* sample n reads volume n / repeat when src == NULL */
  const int32_t* src;    /* nullable [N] */
  const int32_t* flip;   /* nullable [N] */
  const int32_t* dst;    /* nullable [N]: logits slot */
  int32_t drop_mode;     /* VX_DROP_*; HASH uses seed; MASK uses masks[17] */
  uint32_t seed;
  const uint8_t* masks[17]; /* channels-last keep-masks in DROPOUT order (oracle/unet3d_oracle.py) */
  float* logits;         /* [slots][C][D][H][W] */
  void* workspace; size_t workspace_bytes;
  uint32_t* range_flag;  /* nullable device word (zero it before the launch): ends as the bit pattern of the largest
                            |activation| an un-normalised layer handed to a split-fp16 convolution; >= 65504.0f means
                            the fp16 split overflowed somewhere and the logits must not be used (re-run with
                            vx_config.conv_fp32 = 1, the native-fp32 kernels have no such limit) */
  const uint32_t* seed_dev; /* nullable device word added to `seed` by every kernel (graph replays with fresh dropout) */
} vx_unet3d_run;

size_t vx_unet3d_workspace_bytes(int N, int D, int H, int W, int F);
int vx_unet3d_forward(const vx_unet3d_weights* w, const vx_unet3d_run* r, vx_stream_t stream);
/* Diagnostic (bench.py roofline leg; the one entry point that synchronises): the same forward with a HIP event
 * pair around every launch on `stream`; returns per-launch milliseconds and static label strings. */
int vx_unet3d_forward_profiled(const vx_unet3d_weights* w, const vx_unet3d_run* r, vx_stream_t stream,
                               int max_launches, float* ms, const char** labels, int* n_launches);

/* ---------------------------------------------------------------------------------
 * 2D path (HRNet, uncertainty_modeling/models/hrnet_module.py).  Activations: channels-last [N][H][W][pitch] fp32.
 * K15: 3x3 stride 1 / 3x3 stride 2 / 1x1 convolution, padding k/2 (hrnet_module.py:37-41, 85-93, 349-358, 411-428;
 * bias only on last_layer), raw output + per-tile (sum, sumsq) partials [ntiles_total][Cout][2] for the
 * TRAINING-mode BatchNorm that follows (batch statistics over N,H,W; the reference never calls .eval()) -- or, for a
 * model in eval mode, the running-statistics BatchNorm, residual and ReLU applied in the output epilogue (out_scale).
 * Cin must be a multiple of 16, weights packed by vx_pack_conv2d (real channel count: it pads).  The input of C real
 * channels needs NO padding to Cin: in_pitch may be any multiple of 4 in (Cin - 16, ...); channels at and beyond
 * min(Cin, in_pitch) read as zeros, channels [C, in_pitch) must hold zeros (an 18-channel tensor travels at 20 floats
 * per pixel, the 3-channel image at 4). */
typedef struct vx_conv2d_args {
  const float* in; int32_t in_pitch;
  const float* w_packed; const float* bias; /* bias nullable, [Cout] */
  float* out; int32_t out_pitch, out_coff;
  int32_t N, H, W, Cin, Cout, KS, S;        /* KS in {1,3}; S in {1,2} (1x1: S = 1) */
  float* stats_partial;                     /* nullable */
  int32_t w_family;                         /* vx_conv2d_family(Cin, Cout, KS) at the time w_packed was packed */
  /* Optional PROLOGUE (split-fp16 kernels only): `in` is the RAW output of the previous conv; y = x * in_scale[g][c] +
   * in_shift[g][c] (the training-mode BatchNorm folded by vx_bn_finalize[_groups]), then ReLU if in_relu, are applied
   * while the tile is staged -- conv2(relu(bn1(conv1(x)))) of BasicBlock / Bottleneck (hrnet_module.py:59-77, 99-119)
   * without the pass that would write the activated tensor.  g = n / in_group_images (0: one group), rows in_cpitch
   * floats apart.  Zero padding is that of the ACTIVATED tensor. */
  const float* in_scale; const float* in_shift;   /* nullable together */
  int32_t in_cpitch, in_group_images, in_relu;
  /* Optional output EPILOGUE (split-fp16 kernels only; a zero-initialised struct has none):
   *   out[.., out_coff + c] = act( out_add[.., c] + out_scale[c] * (acc + bias)[c] + out_shift[c] )
   * -- a BatchNorm with FIXED statistics (vx_bn_running_affine), the residual of a block end and the ReLU applied as the
   * conv stores, evaluated with the expressions of vx_affine_gather's identity instance in its order: bit-identical to
   * vx_conv2d without the epilogue followed by vx_affine_gather(scale, shift, add, act).  out_scale / out_shift hold
   * [Cout] floats; out_add is channels-last [N][OH][OW][out_add_pitch] at the OUTPUT geometry (channel c of it meets
   * output channel c; out_coff does not apply to it; it may be `out` itself only at the same pitch and out_coff 0).
   * Refused: out_scale with stats_partial (batch statistics of a tensor that is never written raw), out_add or out_act
   * without out_scale, and any of them under vx_config.conv_fp32 = 1. */
  const float* out_scale; const float* out_shift; /* nullable together */
  const float* out_add; int32_t out_add_pitch;    /* nullable */
  int32_t out_act;                                /* VX_ACT_NONE | VX_ACT_RELU */
} vx_conv2d_args;
int64_t vx_conv2d_packed_floats(int Cin, int Cout, int KS);
int vx_pack_conv2d(const float* w_torch /* (Cout,Cin,KS,KS) */, float* w_packed, int Cin, int Cout, int KS, vx_stream_t stream);
int vx_conv2d_tiles(int H, int W, int KS, int S); /* tiles per image (stats_partial has N * this entries) */
int vx_conv2d(const vx_conv2d_args* a, vx_stream_t stream);
/* Dry run of vx_conv2d: every argument check, the choice of the kernel and its launch geometry, no launch and no call into the HIP
 * runtime (works without a GPU; the pointers are only tested for null and alignment).  Returns the VX_E_* code vx_conv2d would
 * refuse the call with (message in vx_last_error_string), or VX_OK with the instance name vx_last_kernel_name() would report after
 * the launch in kernel_name (nullable; at most cap bytes, always terminated) and the geometry in info (nullable). */
typedef struct vx_conv2d_route_info {
  int32_t nchunks;    /* work items per tile (input chunks) */
  int32_t w_all;      /* 1: all chunks' weights stay in LDS for the kernel's life */
  int32_t lds_bytes;  /* dynamic LDS of the launch */
  int32_t grid_x, grid_y; /* persistent workgroups per output-channel group; output-channel groups */
} vx_conv2d_route_info;
int vx_conv2d_route(const vx_conv2d_args* a, char* kernel_name, int cap, vx_conv2d_route_info* info);

/* K16: BatchNorm2d in training mode: partials -> scale = gamma * rstd, shift = beta - mean * scale
 * (biased variance over count = N*OH*OW, eps 1e-5; hrnet_module.py:30, BN_MOMENTUM side effect not reproduced). */
int vx_bn_finalize(const float* stats_partial, int ntiles, int C, int64_t count, float eps, const float* gamma,
                   const float* beta, float* scale, float* shift, vx_stream_t stream);
/* G independent BatchNorm batches in one tensor (the TTA views of test_2D.py:299-311 are separate forwards, each with
 * its own batch statistics; batched here as G groups of consecutive images): group g owns tiles
 * [g * ntiles_per_group, ...) of the partials and row g of scale / shift [G][cpitch]. */
int vx_bn_finalize_groups(const float* stats_partial, int ntiles_per_group, int G, int C, int cpitch, int64_t count_per_group,
                          float eps, const float* gamma, const float* beta, float* scale, float* shift, vx_stream_t stream);

/* BatchNorm2d with RUNNING statistics (model.eval()) as a per-channel affine, for every BatchNorm layer of a model in one
 * launch: scale[c] = gamma[c] / sqrt(running_var[c] + eps), shift[c] = beta[c] - running_mean[c] * scale[c], evaluated in
 * float64 and rounded once to float32 exactly as vx_bn_finalize does from batch statistics; rows [C, cpitch) of scale and
 * shift are written as zeros (the zero tail of a padded activation stays zero through the affine).  `items` is a DEVICE
 * table of n_items entries (the item-table convention of the batched entry points); gamma / beta nullable (1 / 0).
 * Refused before any launch: a null table (VX_E_NULL), n_items outside [1, 65536] or eps < 0 (VX_E_SHAPE). */
typedef struct vx_bn_affine_item {
  const float* gamma; const float* beta; const float* running_mean; const float* running_var;
  float* scale; float* shift;
  int32_t C, cpitch;
} vx_bn_affine_item;
int vx_bn_running_affine(const vx_bn_affine_item* items, int n_items, float eps, vx_stream_t stream);

/* K16/K17/K18: out[.., out_coff + c] = act( add + scale[c] * G(drop(x))[c] + shift[c] ); G = identity (OH,OW == H,W) or
 * F.interpolate(mode="bilinear", align_corners=False) from (H,W) to (OH,OW); add / scale / drop optional; `add` may
 * alias `out` (term-by-term SUM fusion, hrnet_module.py:316-333). */
typedef struct vx_affine_args {
  const float* x; int32_t x_pitch;
  const float* scale; const float* shift;   /* nullable together */
  const float* add; int32_t add_pitch;      /* nullable; [N][OH][OW][add_pitch] */
  float* out; int32_t out_pitch, out_coff;
  int32_t N, H, W, C, OH, OW;
  int32_t act;                              /* VX_ACT_NONE | VX_ACT_RELU */
  int32_t drop_mode; uint32_t drop_seed, drop_layer; const uint8_t* drop_mask; /* F.dropout(x, 0.5, training=True) on x */
  int32_t group_images;                     /* > 0: scale / shift are [G][C], image n uses row n / group_images */
} vx_affine_args;
int vx_affine_gather(const vx_affine_args* a, vx_stream_t stream);

/* The SUM fusion of a HighResolutionModule output (hrnet_module.py:316-333: y = f_i0(x_0); y = y + f_ij(x_j) for j = 1 ..;
 * relu) as ONE pass: out = act(T_0 + T_1 + ... ) added in that order, T_j = scale_j * G_j(x_j) + shift_j with G_j the
 * identity (H, W == OH, OW) or the bilinear upsampling of vx_affine_gather, scale_j / shift_j nullable together (the
 * identity term x_i).  Bit-identical to nterms chained vx_affine_gather passes (the same expressions in the same order); the
 * chain re-read and re-wrote the full-resolution accumulator once per term. */
typedef struct vx_fuse_term {
  const float* x; int32_t x_pitch, H, W;
  const float* scale; const float* shift;   /* nullable together; [G][C] rows when group_images > 0 */
} vx_fuse_term;
typedef struct vx_fuse_args {
  vx_fuse_term term[4]; int32_t nterms;     /* 1 .. 4 */
  float* out; int32_t out_pitch;
  int32_t N, OH, OW, C;
  int32_t act;                              /* VX_ACT_NONE | VX_ACT_RELU, applied to the sum */
  int32_t group_images;
} vx_fuse_args;
int vx_fuse_sum(const vx_fuse_args* a, vx_stream_t stream);

/* Final upsample of the class logits to the input size (hrnet_module.py:667-669) into the reference's NCHW layout:
 * image n -> slot dst[n] (nullable) of out [slots][C][OH][OW]; flip[n] bit 0 un-flips a HorizontalFlip TTA view
 * (test_2D.py:304-309), bit 1 a VerticalFlip one (8-view extension, BASELINE config 4). */
int vx_bilinear_nchw(const float* x, int x_pitch, int N, int H, int W, int C, int OH, int OW, float* out,
                     const int32_t* dst, const int32_t* flip, vx_stream_t stream);
/* The same upsample followed by F.softmax(dim=1) (test_2D.py:300-303: `output_softmax = F.softmax(output, dim=1)` of every
 * forward), in one pass: out holds PROBABILITIES, the full-resolution logits are never written.  Bit-identical to
 * vx_bilinear_nchw + vx_softmax_planar.
 * Any x_pitch >= C is accepted and no float at or beyond x_pitch of a pixel is read.  The register-resident instances
 * (1, 2, 5 or 8 channel quads per pixel, loaded whole) need x 16-byte aligned, x_pitch a multiple of 4 and x_pitch >=
 * 4 Q for the smallest of those Q >= ceil(C / 4): 19 classes at pitch 20 (Q = 5), up to 8 at pitch 8, 29 .. 32 at pitch
 * 32.  Everything else -- among it 9 .. 16 classes at pitch 12 / 16 and 21 .. 28 at pitch 24 / 28, unless the caller pads
 * the pitch to 20 / 32, as HighResolutionNet does for its logits -- takes the scalar kernel: the same bits at 2.3 - 2.4 x
 * the time (8 x 128x256 -> 512x1024 on an MI355X: 12 classes 235 us against 100 us, 24 classes 437 against 182).
 * Channels [C, x_pitch) may hold anything. */
int vx_bilinear_softmax_nchw(const float* x, int x_pitch, int N, int H, int W, int C, int OH, int OW, float* out,
                             const int32_t* dst, const int32_t* flip, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * K14: sliding-window accumulation of a batch of patches (DataCarrier3D.concat_data,
 * uncertainty_modeling/data_carrier_3D.py:137-179, with the F.softmax of test_3D.py:472 fused):
 *   sum[t][c][crop_b] += softmax_c(logits[b][t]);  count[crop_b] += 1 (once per patch, the reference's pred_idx == 0)
 *   logits [B][T][C][P0][P1][P2] (the pred_idx slots of vx_unet3d_forward), crop [B][3] = (x0, y0, z0) int32 on the
 *   device, sum [T][C][X][Y][Z], count [X][Y][Z] float32, zero-initialised by the caller.
 *   overlap != 0: patches of the batch may overlap (patch_overlap < 1) -> float atomics. 2 <= C <= 8. */
int vx_softmax_accumulate(const float* logits, int B, int T, int C, int P0, int P1, int P2, const int32_t* crop,
                          float* sum, float* count, int X, int Y, int Z, int overlap, vx_stream_t stream);

/* Aleatoric-head sampling (predict_cases, test_3D.py:458-469): mu_s [N][2C][nvox] = final_aleatoric output
 * (mu = first C channels, s = last C, unet3D_module.py:367-369); out [N][T][C][nvox] = mu + exp(s/2) * eps_t with
 * eps [N][T][C][nvox] injected (nullable: generated from `seed`, N(0,1)); sigma [N][C][nvox] nullable output. */
int vx_aleatoric_sample(const float* mu_s, const float* eps, uint32_t seed, int N, int T, int C, int64_t nvox,
                        float* out, float* sigma, vx_stream_t stream);

/* Softmax variance (BASELINE.json north_star; no counterpart in the reference): x [B][T][C][nvox] float32 logits
 * (from_logits != 0) or probabilities -> out [B][nvox] = mean over classes of the population variance over T. */
int vx_softmax_variance(const float* x, int from_logits, int B, int T, int C, int64_t nvox, float* out, vx_stream_t stream);

/* SSN sampling (SsnUNet3D.forward + distribution.sample, ssn_unet3D_module.py:39-70; test_3D.py:361-396):
 * head [N][(2+R)*C][nvox] = the three 1x1x1 heads run as one conv (mean | log_cov_diag | cov_factor, factor channel
 * r*C + c); out [N][S][C][nvox] = mean + sum_r factor_r * eps_w[s][n][r] + sqrt(exp(log_cov_diag) + epsilon) *
 * eps_d[s][n][c][v]  (torch.distributions.LowRankMultivariateNormal.rsample).  eps_w [S][N][R], eps_d [S][N][C][nvox]
 * injected, or NULL: generated from `seed`, N(0,1). */
int vx_ssn_sample(const float* head, const float* eps_w, const float* eps_d, uint32_t seed, int N, int S, int C, int R,
                  int64_t nvox, float epsilon, float* out, vx_stream_t stream);

/* The TTA branch of Cityscapes_dataset.__getitem__ (uncertainty_modeling/data/cityscapes_dataset.py:76-99) as ONE launch:
 * a batch of images -> the G views the 2D driver forwards (test_2D.py:299-311), normalised, channels-last float32 at pitch
 * 4 (channel 3 = 0: the layout the stem convolution stages from), out [G][B][H][W][4], flips as index arithmetic.
 *   src_u8 = 1: src [B][H][W][3] uint8; view = Normalize(mean, std, max_pixel_value)(maybe GaussNoise(maybe Flip(img))) with
 *     the arithmetic of albumentations on uint8 input: noisy = uint8(clip(float(img) + field, 0, 255)), then
 *     (v - mean * max) * (1 / (std * max)) in float32 -- bit-exact with values_amd.data.tta_views_2d.  noise0 / noise1:
 *     additive fields [B][H][W][3] (the generator is third-party: albumentations 1.3.0 GaussNoise, so the fields are INPUTS).
 *   src_u8 = 0: src = clean, noise0 = noisy, both [B][3][H][W] float32 already normalised (values_amd.predict2d.tta_views_8).
 *   view_code [G] (HOST array): bit 0 HorizontalFlip, bit 1 VerticalFlip, bit 2 noisy, bit 3 the noise field is indexed at
 *     the SOURCE pixel (flip of the noisy image) instead of the view's (noise drawn after the flip, as the dataset does),
 *     bit 4 noise slot (u8 source).  The reference's four views: {0, 1, 4, 1 | 4 | 16}.  Codes above 31 are refused (bit 5,
 *     "generated field", belongs to vx_tta_views_2d_gen below). */
int vx_tta_views_2d(const void* src, int src_u8, const float* noise0, const float* noise1, const float* mean, const float* std,
                    float max_pixel_value, int B, int H, int W, int G, const int32_t* view_code, float* out, vx_stream_t stream);

/* vx_tta_views_2d with the noise fields of its noisy views DRAWN on the device (uint8 source only).  One more view-code bit:
 * bit 5 = this view's field is generated (with bit 2; a view without bit 5 behaves as in vx_tta_views_2d, a supplied field
 * included, so supplied and generated fields mix in one call).  The additive term of a generated view at field element
 * e = (y * W + x) * 3 + c -- (x, y) the view's pixel, or the SOURCE pixel with bit 3, exactly as a supplied field is indexed --
 * is sqrt(var[b][k]) * N(0, 1), the normal being element e of stream (image0 + b) * 2 + k of the generator the sampling
 * kernels use (vx_gauss, keyed by (seed + *seed_dev, stream, element); float64 restatement: tests/noise_ref.py), k the noise
 * slot of bit 4, and var[b][k] = var_limit[0] + (var_limit[1] - var_limit[0]) * u with ONE uniform u in [0, 1) per (image,
 * slot) from a stream no element shares.  Then the uint8 path of vx_tta_views_2d: clip to 0..255, truncate, normalise.
 * This is the DISTRIBUTION of albumentations' GaussNoise(var_limit=(10, 50), mean=0, per_channel=True) on the project's own
 * stream -- the library's draws come from its own RNG, bit parity with them is out of scope.  image0: global index of the
 * batch's first image (a view does not depend on how images are batched).  seed_dev: nullable device word added to seed
 * (as vx_conv3d_args.seed_dev).  var_limit: HOST float[2], 0 <= lo <= hi.  sigma_out: nullable device [B][2], the scale
 * sqrt(var) of both slots of every image, written when at least one view is generated.  Codes above 63, bit 5 without bit 2
 * and bit 5 with the f32 source are refused (VX_E_DTYPE). */
int vx_tta_views_2d_gen(const void* src, int src_u8, const float* noise0, const float* noise1, const float* mean,
                        const float* std, float max_pixel_value, int B, int H, int W, int G, const int32_t* view_code,
                        uint32_t seed, const uint32_t* seed_dev, int64_t image0, const float* var_limit, float* sigma_out,
                        float* out, vx_stream_t stream);

/* The noisy input of the 3D TTA (predict_cases, test_3D.py:428: GaussianNoiseTransform, variance ~ U(0, 0.1)) drawn on the
 * device:  out[v][r] = x[v][r] + sigma_g * N(0, 1)  for v in [0, V), r in [0, per), per = C * D * H * W < 2^32, the normal
 * being element r of stream g = index0 + v of vx_gauss under seed + *seed_dev (seed_dev: nullable device word, as
 * vx_conv3d_args.seed_dev -- a captured graph draws fresh noise per replay).  g is the volume's GLOBAL index: with the seed
 * it is all that keys the volume's stream, so chunks, shards and batch sizes do not change a view.
 * var_g = var_lo + (var_hi - var_lo) * u, ONE uniform u in [0, 1) per volume from a stream no element shares;
 * sigma_law 0: sigma_g = sqrt(var_g) (values_amd.predict.gaussian_noise_view; the default everywhere);
 * sigma_law 1: sigma_g = var_g (what batchgenerators' augment_gaussian_noise is believed to do -- it hands the drawn
 * "variance" to numpy's normal() as the scale; UNVERIFIED, the library is not available to this project).
 * The distribution is the reference's, the stream the project's own (float64 restatement: tests/noise_ref.py).
 * sigma_out: nullable device [V].  out may be the second half of an [orig | noisy] buffer whose first half is x; x and out
 * must not overlap partially.  Refused: V <= 0, per >= 2^32, index0 < 0 or index0 + V > 2^32, var_lo < 0, var_hi < var_lo
 * (VX_E_SHAPE); null x / out (VX_E_NULL); another sigma_law (VX_E_DTYPE).  per == 0 is a no-op. */
int vx_noise_view_3d(const float* x, float* out, int V, int64_t per, uint32_t seed, const uint32_t* seed_dev, int64_t index0,
                     float var_lo, float var_hi, int sigma_law, float* sigma_out, vx_stream_t stream);

/* Colour rendering of an arg-max mask (Tester.save_prediction, test_2D.py:124-134): rgb[i] = lut[labels[i]] with
 * labels[i] := unlabeled where ignore[i] != 0 (ignore nullable); lut [256][3] uint8, rgb [n][3]. */
int vx_colorize_u8(const uint8_t* labels, const uint8_t* ignore, int64_t n, const uint8_t* lut, int unlabeled, uint8_t* rgb,
                   vx_stream_t stream);

/* K40: threshold search (evaluation/uncertainty_aggregation/find_threshold.py) for one array, a whole reader batch or a
 * whole split in one call each (select.hip).  np.quantile(x, q) is the lerp of the two order statistics around
 * q * (n - 1), done by the host in float64.
 * vx_count_nonzero_batched (calculate_foreground_quantile_image, find_threshold.py:11-13, for a batch of predicted masks):
 *   counts[i] (device, zeroed here) = np.count_nonzero of item i.  An item is a device pointer, an element count n >= 0
 *   and a kind: VX_COUNT_B1 / B2 / B4 / B8, an integer or bool of 1 / 2 / 4 / 8 bytes (non-zero: any bit set), or
 *   VX_COUNT_F32 / F64 (non-zero: x != 0, so NaN counts and -0.0 does not).  An item with n = 0 yields 0 and its pointer
 *   is not looked at; pointers need only the alignment of their elements.  One memset and ONE launch for all items: the
 *   items are cut into work blocks of 16 KB that the workgroups take in turn, so thousands of small 2D masks and a few
 *   large volumes share one grid.  0 <= n_items <= VX_SELECT_MAX_ITEMS.
 * vx_select_segments (calculate_threshold_image, find_threshold.py:63-68: np.quantile over all validation maps):
 *   out[0] = the k-th smallest (0-based), out[1] = the (k+1)-th smallest of the UNION of the items' elements, where the
 *   maps lie: no concatenation and no cast copy.  k + 1 == n_total: out[1] = out[0].  An item is VX_F32, or VX_F64
 *   narrowed to float32 on load (round to nearest even, as astype(float32)).  MSB-first radix select over the usual
 *   order-preserving map of IEEE float32 bits to unsigned keys (negative: all bits flipped, non-negative: sign bit set)
 *   in passes of 11, 11 and 10 bits (LDS histograms folded into 64-bit bins); the second order statistic
 *   needs no second select: the last pass knows whether another key equal to the k-th remains, and only if none does one
 *   more pass takes the minimum key above it -- decided on the device, the host does not wait between passes.  At most
 *   four reads of the data; a memset, the table upload and eight launches.  status (device) = VX_SELECT_NAN when any element is NaN (the outputs
 *   are then unspecified), else VX_SELECT_OK; +-inf are ordinary values.  Integer arithmetic only: exact, independent of
 *   order and grid size.  1 <= n_items <= VX_SELECT_MAX_ITEMS, element counts are 64-bit.
 * Both refuse before any device call: a null table or a null pointer of a non-empty item (VX_E_NULL), n_items or an n out of
 * range, for the selection n_total = 0 or k outside [0, n_total) (VX_E_SHAPE), an unknown kind / dtype (VX_E_DTYPE), a
 * pointer off its element alignment or a workspace off 16 bytes (VX_E_ALIGN), a short workspace (VX_E_WORKSPACE).
 * workspace: vx_*_workspace_bytes(n_items) bytes, 0 for an n_items the call refuses.  The item table goes up through a
 * pinned staging buffer inside the call: no wait on the stream (only, if it is still in flight, for the previous call's
 * upload), and neither call is capturable into a hipGraph. */
#define VX_SELECT_MAX_ITEMS 65536
enum { VX_COUNT_B1 = 0, VX_COUNT_B2 = 1, VX_COUNT_B4 = 2, VX_COUNT_B8 = 3, VX_COUNT_F32 = 4, VX_COUNT_F64 = 5 };
enum { VX_SELECT_OK = 0, VX_SELECT_NAN = 1 };
typedef struct vx_count_item {
  const void* ptr; /* device, n elements */
  int64_t n;
  int32_t kind; /* VX_COUNT_* */
  int32_t reserved;
} vx_count_item;
typedef struct vx_select_item {
  const void* ptr; /* device, n elements */
  int64_t n;
  int32_t dtype; /* VX_F32 | VX_F64 */
  int32_t reserved;
} vx_select_item;
int64_t vx_count_nonzero_batched_workspace_bytes(int n_items);
int vx_count_nonzero_batched(const vx_count_item* items /* host */, int n_items, uint64_t* counts /* device [n_items] */,
                             void* workspace, int64_t ws_bytes, vx_stream_t stream);
int64_t vx_select_segments_workspace_bytes(int n_items);
int vx_select_segments(const vx_select_item* items /* host */, int n_items, int64_t k, float* out /* device [2] */,
                       int32_t* status /* device */, void* workspace, int64_t ws_bytes, vx_stream_t stream);

/* K41: preprocessing of a 3D data set (datasets/preprocess_datasets_3d.py:135-168) for a whole batch of raw volumes and
 * their raters' labels, where vx_nifti_decode left them (preprocess.hip).
 * vx_volume_stats_batched: stats[i] (device, 4 doubles) = {mean, std, min, n} of item i as numpy computes them on the data
 *   widened to float64: mean = sum(x) / n, std = sqrt(sum((x - mean)^2) / n) (ddof 0, two passes over the data like np.std,
 *   not a one-pass variance), min as np.min; a NaN anywhere makes all three NaN.  An item is a device pointer, a 64-bit
 *   element count 1 <= n <= 2^40 and a kind VX_PREP_*: an integer or bool of 1 / 2 / 4 bytes, float32 or float64.  Float
 *   kinds accumulate in float64.  Integer kinds accumulate sum(x) in 64-bit integers and convert it once: the mean is
 *   numpy's bit for bit whenever numpy's own float64 sum is exact (|sum(x)| < 2^53; the integer sum itself is exact below
 *   2^63, that is for every n < 2^31 of a 4-byte kind).  Each item is cut into work blocks of 32 KB counted from its
 *   first element, the blocks of all items are taken in turn by one grid, every block leaves one partial, and one
 *   workgroup per item adds the item's partials in an order fixed by its block count.  No floating-point atomics.  The cut,
 *   the order inside a block and the order of the partials depend on the item's own n and kind only: AN ITEM'S FOUR
 *   NUMBERS ARE BIT-EQUAL WHETHER IT IS SUBMITTED ALONE OR IN ANY BATCH, AT ANY POSITION (and whatever the grid size).
 *   The mean stays on the device between the passes: four launches, no wait on the host.
 * vx_zscore_pad_batched: per item, the source box dims[3] (C order, z innermost) is placed at pad_below[3] of the output
 *   box out_dims[3].  Mode VX_PREP_ZSCORE: an output voxel inside the source box is (double(x) - mean) / (std + 1e-8), a
 *   voxel outside it the same expression on min, with {mean, std, min} = stats[stats_row] READ ON THE DEVICE (the rows
 *   vx_volume_stats_batched wrote on the same stream: the host does not wait between the two calls); IEEE operations,
 *   correctly rounded -- a true division, no reciprocal, no FMA contraction -- and ONE rounding to out_dtype (VX_F32 |
 *   VX_F64; VX_PREP_OWN: float32 for a float32 source, else float64, as numpy promotes).  Mode VX_PREP_COPY (labels;
 *   out_dtype VX_PREP_OWN): inside x unchanged, outside min, both in the source's kind.  The output is cut into work
 *   blocks of 32 KB that one grid takes in turn, so many small crops and a few large volumes fill the device from one
 *   launch; lanes run along z, a thread writes 16 bytes of output with one store and reads its source run with one load
 *   where the run lies inside one source row; chunks that cross a row end or a padding slab, the last chunk of an item
 *   and a dst off 16 bytes take the per-element path.  What a voxel becomes depends on its item alone.
 * Both refuse before any device call: a null table, pointer, stats or workspace (VX_E_NULL); n_items outside
 *   [0, VX_SELECT_MAX_ITEMS], n < 1, a dimension < 1, more than 2^40 elements, out_dims[a] < dims[a] + pad_below[a], a
 *   negative pad_below, a stats_row outside [0, VX_SELECT_MAX_ITEMS), overlapping src / dst (VX_E_SHAPE); an unknown kind,
 *   mode or out_dtype (VX_E_DTYPE); a pointer off its element alignment or a workspace off 16 bytes (VX_E_ALIGN); a short
 *   workspace (VX_E_WORKSPACE).  workspace: vx_*_workspace_bytes(items, n_items) bytes, 0 for what the call refuses (and
 *   for n_items = 0, which is a no-op).  The item table goes up through a pinned staging buffer inside the call: no wait
 *   on the stream (only, if it is still in flight, for the previous call's upload), and, like K40, neither call is
 *   capturable into a hipGraph. */
enum { VX_PREP_U8 = 0, VX_PREP_I8 = 1, VX_PREP_U16 = 2, VX_PREP_I16 = 3, VX_PREP_U32 = 4, VX_PREP_I32 = 5, VX_PREP_F32 = 6, VX_PREP_F64 = 7 };
enum { VX_PREP_ZSCORE = 0, VX_PREP_COPY = 1 };
#define VX_PREP_OWN (-1)
typedef struct vx_prep_item {
  const void* ptr; /* device, n elements */
  int64_t n;
  int32_t kind; /* VX_PREP_* (bool: VX_PREP_U8) */
  int32_t reserved;
} vx_prep_item;
typedef struct vx_prep_pad_item {
  const void* src;      /* device [dims[0]][dims[1]][dims[2]] of kind */
  void* dst;            /* device [out_dims[0]][out_dims[1]][out_dims[2]] */
  int32_t dims[3];
  int32_t out_dims[3];
  int32_t pad_below[3];
  int32_t kind;         /* VX_PREP_* */
  int32_t out_dtype;    /* VX_F32 | VX_F64 | VX_PREP_OWN */
  int32_t mode;         /* VX_PREP_ZSCORE | VX_PREP_COPY */
  int32_t stats_row;    /* the item's row of stats */
  int32_t reserved;
} vx_prep_pad_item;
int64_t vx_volume_stats_batched_workspace_bytes(const vx_prep_item* items /* host */, int n_items);
int vx_volume_stats_batched(const vx_prep_item* items /* host */, int n_items, double* stats /* device [n_items][4] */,
                            void* workspace, int64_t ws_bytes, vx_stream_t stream);
int64_t vx_zscore_pad_batched_workspace_bytes(const vx_prep_pad_item* items /* host */, int n_items);
int vx_zscore_pad_batched(const vx_prep_pad_item* items /* host */, int n_items, const double* stats /* device */,
                          void* workspace, int64_t ws_bytes, vx_stream_t stream);

/* K42: the generator of the toy 3D data sets (datasets/toy_data_generation/dataset_generation.py:144-254, helpers in
 * stl_to_nifty.py:93-155) on the device, float64 throughout (toydata.hip).  Every entry takes caller-owned memory and an
 * explicit stream; nothing is uploaded (ranks, thresholds and boxes travel as kernel arguments), so the calls are
 * capturable.  An image is a C-order [D0][D1][D2] array, axis 2 contiguous.
 * vx_toy_embed: image = 0 outside the object's box, gray * (double)obj inside it; obj is float32 [obj_dims] placed at
 *   the signed offset[3] and clipped to the image on both sides (both embed functions of stl_to_nifty.py:93-142).
 *   flip0 / flip1 reverse axis 0 / axis 1 of the finished image (np.flipud / np.fliplr).
 * vx_gauss_blur_axis_f64: ONE pass of scipy.ndimage.gaussian_filter's separable filter along `axis` of src into dst,
 *   in scipy's order of operations (its symmetric correlate1d): x[l] * w[r] first, then for i = r .. 1 the pair
 *   (x[l - i] + x[l + i]) * w[r - i] added to the sum, every operation rounded once to float64, no FMA, no
 *   reassociation; mode `reflect` for any extent >= 1 against any radius (index i mod 2n, the second half mirrored).
 *   weights: DEVICE array of 2 radius + 1 doubles, 0 <= radius <= 128.  Passes over axes 0, 1, 2 in turn with
 *   scipy's weights give gaussian_filter's result bit for bit.  A pass never runs in place: src and dst may not overlap.
 *   Lanes run along axis 2 in all three passes; 16-byte loads and stores where the contiguous extent is even and both
 *   pointers are 16-byte aligned, 8-byte ones elsewhere.
 * vx_count_ge_f64: *count (device, int64) = #{i: x[i] >= thr}; integer atomics, exact.  n = 0 gives 0.
 * vx_order_stats_f64: for each 0-based rank ks[i] (HOST array, 1 <= n_k <= 32, 0 <= k < n), out[i] (device, 2 doubles)
 *   = {the k-th smallest, the (k + 1)-th smallest} value of x[0, n); the second repeats the first when k + 1 == n.
 *   MSB-first radix select in eight 8-bit digits on the order-preserving 64-bit keys (negative: all bits flipped,
 *   non-negative: sign bit set; -0.0 sorts directly below +0.0 and compares equal to it): integer arithmetic only, exact
 *   and independent of the grid.  Up to 16 distinct ranks share a sweep of eight passes, each pass one read of the data:
 *   vx_order_stats_f64_reads says how many reads a call makes (8 per 16 distinct ranks among {k, k + 1}; 0 for what the
 *   call refuses).  status (device) = VX_SELECT_NAN when any element is NaN (the outputs are then unspecified), else
 *   VX_SELECT_OK; +-inf are ordinary values.  workspace: vx_order_stats_f64_workspace_bytes(n_k) bytes, 16-byte aligned.
 *   vx_select_segments narrows float64 to float32 and cannot serve where the float64 order statistics are needed.
 * vx_toy_segment: out[r][i] (device int32 [R][n]) = x[i] >= thresholds[r]; thresholds is a HOST array of R doubles,
 *   1 <= R <= 64; one read of the image for all R (create_segmentations' np.where(image >= threshold, 1, 0)).
 * vx_toy_noise: in place, where x[i] < 0.1: x[i] = (u_p <= noise_prob) ? 0 : u_n with u_p = (h1 >> 8) * 2^-24 and
 *   u_n = (h2 >> 8) * 2^-24 from the two hash words of the library's generator for (seed, stream stream_index,
 *   element i); elements >= 0.1 and NaN are left alone.  An element's value depends on (seed, stream_index, i) only.
 *   n < 2^32 (the element index is one hash word), 0 <= noise_prob <= 1.  add_noise (stl_to_nifty.py:145-150) with
 *   this library's generator in place of numpy's stream.
 * All refuse before any device call: a null pointer (VX_E_NULL); a dimension < 1, more than 2^40 voxels, an axis
 *   outside 0..2, a radius outside 0..128, overlapping src / dst, n_k, R, n or a rank out of range, a noise_prob outside
 *   [0, 1] (VX_E_SHAPE); a pointer off its element alignment or a workspace off 16 bytes (VX_E_ALIGN); a short workspace
 *   (VX_E_WORKSPACE). */
int vx_toy_embed(const float* obj /* device */, const int32_t* obj_dims /* host [3] */, const int32_t* offset /* host [3] */,
                 double gray, int flip0, int flip1, double* image /* device */, const int32_t* dims /* host [3] */,
                 vx_stream_t stream);
int vx_gauss_blur_axis_f64(const double* src, double* dst, const int32_t* dims /* host [3] */, int axis,
                           const double* weights /* device [2 radius + 1] */, int radius, vx_stream_t stream);
int vx_count_ge_f64(const double* x, int64_t n, double thr, int64_t* count /* device */, vx_stream_t stream);
int64_t vx_order_stats_f64_workspace_bytes(int n_k);
int vx_order_stats_f64_reads(int64_t n, const int64_t* ks /* host */, int n_k);
int vx_order_stats_f64(const double* x, int64_t n, const int64_t* ks /* host */, int n_k, double* out /* device [n_k][2] */,
                       int32_t* status /* device */, void* workspace, int64_t ws_bytes, vx_stream_t stream);
int vx_toy_segment(const double* x, int64_t n, const double* thresholds /* host [R] */, int R, int32_t* out /* device [R][n] */,
                   vx_stream_t stream);
int vx_toy_noise(double* x, int64_t n, uint32_t seed, uint32_t stream_index, double noise_prob, vx_stream_t stream);

/* K44: triangle meshes to a label volume, the toy generator's first step (the reference's meshes_to_numpy,
 * datasets/toy_data_generation/stl_to_nifty.py:82-90) under this project's own rule (values_amd/stl.py, voxelize.hip,
 * DESIGN 4.54).  Caller-owned memory and an explicit stream; nothing is uploaded (origin, h, dims and the mesh offsets
 * travel as kernel arguments), so the call is capturable.
 * vx_voxelize_meshes: tris holds the float32 triangles [n_tri][vertex 3][xyz 3] of all meshes, mesh m being triangles
 *   [mesh_offsets[m], mesh_offsets[m + 1]).  Voxel (k, j, i) of out [n_z][n_y][n_x] has the sample point
 *   c_a(t) = origin_a + (t + 0.5) * h (float64, in that order) and is inside mesh m when an odd number of m's triangles are
 *   hit by the column (c_x(i), c_y(j)) at a depth z_hit < c_z(k).  out = 0 outside all meshes, m + 1 inside mesh m, later
 *   meshes overwriting earlier ones.  A triangle (float32 widened to float64) is hit when its projected area
 *   E(v0, v1; v2) is not 0, the column lies in its closed xy box, and for each edge (v1,v2), (v2,v0), (v0,v1) the
 *   weight w_e = Ec * m is > 0, or == 0 with m > 0, where Ec = (q.x - p.x) * (s.y - p.y) - (q.y - p.y) * (s.x - p.x) on the
 *   endpoints ordered p < q by (x, then y) and m = sign(area) * (the edge came as (q, p) ? -1 : +1): a point on an edge
 *   belongs to the triangle on the positive side of the ordered edge, so a closed mesh is crossed an even number of
 *   times by every column.  z_hit = ((w0 z0 + w1 z1) + w2 z2) / ((w0 + w1) + w2).  Every operation is rounded once to
 *   float64: no FMA, no reassociation.  *odd_columns (device, zeroed by the call) = the number of (mesh, column) pairs
 *   hit an odd number of times: 0 for closed meshes; integer atomics, exact.
 *   Refused before any device call: a null pointer (VX_E_NULL); n_meshes outside 1..16, a dimension outside 1..1024,
 *   n_tri outside 1..2^20, offsets not increasing from 0 to n_tri, h not finite and positive, a non-finite origin
 *   (VX_E_SHAPE); a pointer off its element alignment (VX_E_ALIGN). */
int vx_voxelize_meshes(const float* tris /* device [n_tri][3][3] */, const int64_t* mesh_offsets /* host [n_meshes + 1] */,
                       int n_meshes, const double* origin /* host [3] xyz */, double h, const int32_t* dims /* host [3]: n_z, n_y, n_x */,
                       float* out /* device [n_z][n_y][n_x] */, int64_t* odd_columns /* device (1,) */, vx_stream_t stream);

/* K43: preprocessing of the GTA / Cityscapes 2D data sets (datasets/gta_cityscapes/preprocess_gta_cityscapes.py:128-174)
 * for a whole batch of decoded images and label files, where vx_png_unfilter left them (preprocess2d.hip).
 * vx_crop_resize_batched: per item, the box [y0, y0 + crop_h) x [x0, x0 + crop_w) of the source [H][W][bpp] (uint8, C
 *   order, any alignment; bpp 3 = RGB, 4 = RGBA with alpha dropped, 1 = grey, or palette indices when `palette`, device
 *   256 x 3 RGB bytes, is given: the pixel is then palette[index], gathered in the kernel -- no expanded image exists)
 *   is shrunk by the even integer `factor` k to out_h x out_w = vx_p2d_out_size(crop_h, k) x vx_p2d_out_size(crop_w, k):
 *   crop / k rounded half to even on the exact quotient, cv2.resize's saturate_cast<int>(size * fx).  Modes:
 *   VX_P2D_IMAGE        cv2.resize(INTER_LINEAR) on uint8 at fx = fy = 1 / k: output (y, x) has the taps k y + k/2 - 1 and
 *                       k y + k/2 on each axis (the second clamped to the crop's last row / column, as OpenCV clamps),
 *                       each with weight 1/2, and OpenCV's 11-bit fixed point gives exactly (p00 + p01 + p10 + p11 + 2) >> 2
 *                       per channel.  Only those two rows of every k are read.  out_rgb [out_h][out_w][3].
 *   VX_P2D_LABEL_IDS    (bpp 1, no palette) INTER_NEAREST: source pixel (k y, k x); out_ids uint8 [out_h][out_w] =
 *                       id2trainid[pixel], out_rgb = trainid2color[that train id].
 *   VX_P2D_LABEL_COLOR  (bpp 3 / 4, or 1 with a palette) INTER_NEAREST in RGB: out_rgb is the pixel, out_ids INT64
 *                       [out_h][out_w] the id of the color2trainid entry whose key is the pixel's 0x00RRGGBB, else
 *                       default_id (vx_rgb_to_trainid's lookup: of two entries with one key the later counts).
 *   status[i] (device, zeroed by the call) = the number of pixels of item i whose id is default_id (LABEL_COLOR; integer
 *   atomics, exact), 0 for the other modes: the reference's `assert 128 not in mask` is the host's to raise.
 *   ONE launch serves the batch, sizes and modes mixed: every item's OUTPUT is cut into work blocks of 2048 pixels counted
 *   from its first pixel and one grid takes the blocks of all items in turn.  A pixel's value depends on its item alone:
 *   AN ITEM'S OUTPUT BYTES ARE EQUAL WHETHER IT IS SUBMITTED ALONE OR IN ANY BATCH, AT ANY POSITION.  Lanes run along
 *   output x, four pixels per lane and step; the taps are fetched with aligned dword loads that cover them whatever the
 *   source's alignment (byte loads only within 12 bytes of the source's two ends); a lane's 12 RGB bytes, 4 ids or 4
 *   int64 ids leave in dword / 16-byte stores where the output address allows it.  No read outside
 *   [src, src + H * W * bpp), no write outside the outputs.  Plain C++ stores.
 *   Refused before any device call: a null item table, status, workspace, src or an output or table the mode needs
 *   (VX_E_NULL); n_items outside [0, VX_SELECT_MAX_ITEMS], H or W < 1, a crop box outside the image or empty, an odd or
 *   non-positive factor, an output dimension of 0, H * W * bpp >= 2^31, n_color outside 0..256 (VX_E_SHAPE); a bpp other
 *   than 1 / 3 / 4, a palette with bpp != 1, bpp 1 without a palette in IMAGE or LABEL_COLOR mode, LABEL_IDS with bpp != 1
 *   or with a palette, an unknown mode, a default_id outside 0..255 (VX_E_DTYPE); an int64 out_ids off 8 bytes or a
 *   workspace off 16 (VX_E_ALIGN); a short workspace (VX_E_WORKSPACE).  workspace:
 *   vx_crop_resize_batched_workspace_bytes(items, n_items, tables) bytes, 0 for what the call refuses and for n_items = 0
 *   (a no-op).  The item table goes up through a pinned staging buffer: no wait on the stream, not capturable. */
enum { VX_P2D_IMAGE = 0, VX_P2D_LABEL_IDS = 1, VX_P2D_LABEL_COLOR = 2 };
typedef struct vx_p2d_item {
  const uint8_t* src;     /* device [H][W][bpp] */
  const uint8_t* palette; /* device [256][3] RGB, or null */
  int32_t H, W, bpp;
  int32_t y0, x0, crop_h, crop_w;
  int32_t factor;
  int32_t mode;           /* VX_P2D_* */
  int32_t reserved;
  uint8_t* out_rgb;       /* device [out_h][out_w][3] */
  void* out_ids;          /* device [out_h][out_w]: uint8 (LABEL_IDS), int64 (LABEL_COLOR); IMAGE: not looked at */
} vx_p2d_item;
typedef struct vx_p2d_tables {
  const uint8_t* id2trainid;     /* device [256] */
  const uint8_t* trainid2color;  /* device [256][3] */
  const uint32_t* color2trainid; /* device [n_color] pairs (0x00RRGGBB key, id) */
  int32_t n_color;
  int32_t default_id;
} vx_p2d_tables;
int vx_p2d_out_size(int size, int factor); /* host only; 0 for size < 1 or an odd or non-positive factor */
int64_t vx_crop_resize_batched_workspace_bytes(const vx_p2d_item* items /* host */, int n_items, const vx_p2d_tables* tables /* host */);
int vx_crop_resize_batched(const vx_p2d_item* items /* host */, int n_items, const vx_p2d_tables* tables /* host */,
                           int32_t* status /* device [n_items] */, void* workspace, int64_t ws_bytes, vx_stream_t stream);

/* K44: the raters of the 2D test split (uncertainty_modeling/augmentations.py:9-50, StochasticLabelSwitches.apply_to_mask)
 * and the label-switch variance map (evaluation/utils/gta.py:15-35) for a whole batch of label maps, where the loader
 * left them (label_switch.hip).
 * vx_label_switch_batched: per item, a label map [H][W] (device; kind VX_COUNT_B1 / B2 / B4 / B8: an integer of 1 / 2 /
 *   4 / 8 bytes; H, W >= 1 and H * W < 2^31; sizes may differ within a batch; pointers need only the alignment of their
 *   elements; VX_COUNT_B1 labels are read as UNSIGNED bytes -- a caller holding signed bytes widens them to 2 bytes first,
 *   as values_amd.dataset2d does, or a negative label passes as 128..255 uncounted) gives
 *     refs     [R][H * W] uint8 (or null): refs[r][i] = rows[k].to where label[i] == rows[k].from and decision(item, r, k),
 *              else (uint8)label[i] -- 255 (ignore) and every class without a row pass through;
 *     variance [W][H] float32 (or null), THE FIRST TWO AXES SWAPPED as gta.py:34 returns it: var_table[label[y][x]] at
 *              [x][y].  var_table (host, 256 floats) is the caller's: built as gta.py builds its values, the map is
 *              bit-equal to the host hook's.
 *   A label outside 0..255 gives 255 in refs, var_table[255] in variance, and is counted in status[i] (device, zeroed by
 *   the call; integer atomics, exact): the host turns a non-zero count into its error.
 *   rows (host, 1 <= n_switch <= VX_LSWITCH_MAX_ROWS): {from, to, thr}, labels in 0..255, thr = (uint32)(p * 2^24) <= 2^24.
 *   All `from` are distinct and no `to` equals a `from` (so the result does not depend on the order of the rows, and
 *   the table is what the reference's sequential in-place moves compute); anything else is VX_E_SHAPE.
 *   Decisions: given -- decisions (host) [n_items][R][n_switch], values 0 / 1 -- or, with decisions == NULL, drawn on the
 *   device: decision(item, r, k) = (h1 >> 8) < rows[k].thr with h1 the first word of the generator of the sampling
 *   kernels (gauss.h: vx_gauss_words) for seed ^ VX_LSWITCH_XOR, element r * n_switch + k, stream item.index.  An
 *   integer compare: values_amd.dataset2d.switch_decisions restates it exactly.  index is the image's position in its
 *   split, so an image's raters do not depend on the batching.
 *   ONE launch serves the batch: every item is cut into tiles of 32 rows x 128 columns and one grid takes the tiles of
 *   all items in turn.  A workgroup builds the R 256-entry remap tables of its item in LDS once, loads the tile in
 *   aligned 16-byte pieces, narrows it to bytes in LDS, stores every rater plane in aligned 16-byte pieces (element
 *   stores only in the pieces that hold a row's two ends) and writes the swapped-axes variance from the LDS tile with
 *   lanes along H.  AN ITEM'S OUTPUT BYTES ARE EQUAL WHETHER IT IS SUBMITTED ALONE OR IN ANY BATCH, AT ANY POSITION.
 *   No read outside [labels, labels + H * W elements), no write outside the outputs.  Plain C++ stores.
 *   Refused before any device call: a null item table, switch table, labels, status or workspace, or a variance map
 *   without var_table (VX_E_NULL); n_items outside [1, VX_SELECT_MAX_ITEMS], R outside [1, VX_LSWITCH_MAX_R], n_switch
 *   out of range, H or W < 1, H * W >= 2^31, a bad switch table, a decision other than 0 / 1 (VX_E_SHAPE); an unknown
 *   kind (VX_E_DTYPE); labels off their element alignment, variance off 4 bytes or a workspace off 16 (VX_E_ALIGN); a
 *   short workspace (VX_E_WORKSPACE).  workspace: vx_label_switch_batched_workspace_bytes(n_items, R) bytes, 0 for what
 *   the call refuses.  The tables go up through a pinned staging buffer: no wait on the stream, not capturable. */
#define VX_LSWITCH_MAX_R 31
#define VX_LSWITCH_MAX_ROWS 8
typedef struct vx_lswitch_item {
  const void* labels; /* device [H][W] */
  uint8_t* refs;      /* device [R][H * W], or null */
  float* variance;    /* device [W][H], or null */
  int32_t H, W;
  int32_t kind;       /* VX_COUNT_B1 | B2 | B4 | B8 */
  uint32_t index;     /* position of the image in its split: keys the item's random streams */
} vx_lswitch_item;
typedef struct vx_lswitch_row {
  int32_t from, to;
  uint32_t thr;
} vx_lswitch_row;
int64_t vx_label_switch_batched_workspace_bytes(int n_items, int R);
int vx_label_switch_batched(const vx_lswitch_item* items /* host */, int n_items, int R, const vx_lswitch_row* rows /* host */,
                            int n_switch, const uint8_t* decisions /* host [n_items][R][n_switch], or null: drawn */, uint32_t seed,
                            const float* var_table /* host [256], or null */, int32_t* status /* device [n_items] */,
                            void* workspace, int64_t ws_bytes, vx_stream_t stream);

/* The 3D test split on the device (patches3d.hip; values_amd.sliding.run_test_3d): three batched streaming
 * passes whose batches mix cases.  Common to all three: lanes run along z, a lane takes four consecutive z positions of a
 * row and moves them in one access of up to 16 bytes where they lie inside the row and the address is aligned to the
 * access, element by element elsewhere; no byte outside a crop, a destination box or an output array is touched; an
 * item's result does not depend on its batch mates; the host item tables go up through a pinned staging buffer inside
 * the call (no wait on the stream, not capturable into a hipGraph); every check below runs before any device call;
 * workspace: the call's *_workspace_bytes(...) bytes (0 for counts the call refuses), 16-byte aligned.
 *
 * vx_gather_patches_3d: out [n_items][P0][P1][P2] float32; out[i] is the crop [origin, origin + P) of item i's volume
 *   src [dims0][dims1][dims2] of kind VX_PREP_*, converted as numpy's astype(float32) converts (round to nearest even from
 *   float64 and the 32-bit integers, exact from the narrower kinds).  Traffic: P0*P1*P2 * (esize + 4) bytes per item.
 *   Refused: a null table, out, workspace or src (VX_E_NULL); n_items outside [1, VX_SELECT_MAX_ITEMS], P or a dimension
 *   below 1, a crop not inside its volume (VX_E_SHAPE); an unknown kind (VX_E_DTYPE); src off its element alignment, out
 *   off 4 bytes, a workspace off 16 (VX_E_ALIGN); a short workspace (VX_E_WORKSPACE).
 *
 * vx_softmax_accumulate_cases: vx_softmax_accumulate with the destination taken per patch.  logits [B][T][C][P0][P1][P2]
 *   float32; patch b adds softmax_c(logits[b][t]) into items[b].sum [T][C][X][Y][Z] at origin and 1 into items[b].count
 *   [X][Y][Z] (t == 0), dims = {X, Y, Z}.  Per voxel the expressions of vx_softmax_accumulate in their order (running
 *   maximum, expf, one reciprocal): with sum_overlap == 0 (plain read-modify-write) the result is bit-equal to that call
 *   made image by image; with sum_overlap != 0 sums and counts go through float atomics (overlapping patches of one
 *   image: the order of the additions is not fixed).  A voxel of a patch outside its image is skipped.  2 <= C <= 8.
 *   Traffic: B*T*C*P^3 * 4 bytes read, twice that read and written in the sums.
 *   Refused: null logits, table, workspace, sum or count (VX_E_NULL); B outside [1, VX_SELECT_MAX_ITEMS], T or P below 1,
 *   C outside [2, 8], a dimension below 1, a negative origin, or -- with sum_overlap == 0 -- two items that name the same
 *   sum with boxes (cut to the image) that share a voxel (VX_E_SHAPE); a pointer off 4 bytes or a workspace off 16
 *   (VX_E_ALIGN); a short workspace (VX_E_WORKSPACE).
 *
 * vx_case_composite: the composites DataCarrier3D keeps beside the predictions (concat_data / save_data,
 *   data_carrier_3D.py:130-153, 173-179, 209-214; calculate_metrics, test_3D.py:555-562), from the case's resident file
 *   payloads and the count map the accumulation left, n = X*Y*Z voxels, in float64 with true divisions:
 *     data   [n] float64      = (0 + x + ... + x, count[v] additions of double(image[v])) / max(count[v], 1)
 *     gt_seg [R][n] float64   = double(intc sum of count[v] additions of the label) / max(count[v], 1)
 *     gt     [R][n] uint8     = (intc) of that, narrowed
 *   A voxel under no patch (count 0) is 0 in all three.  Any of the three outputs may be null (image may be null when
 *   data is).  The R raters of item i are labels[first_label .. first_label + R): device arrays of n integers of 1 / 2 /
 *   4 / 8 bytes (kind VX_COUNT_B1 .. B8) where the reader left them; the value used is the one astype(intc) gives, and a
 *   label outside 0..255 is counted in status[i] (device, zeroed by the call; integer atomics): the host turns a
 *   non-zero count into its error.  A label array is read as UNSIGNED integers unless its flags hold VX_LABEL_SIGNED:
 *   without the flag a signed byte -1 passes as 255, uncounted, and a signed 2-byte -1 is counted but used as 65535; a
 *   caller holding signed elements sets the flag (values_amd.dataset3d.composite_device does) and negative labels are then
 *   counted and used as astype(intc) gives them.  Traffic per voxel: esize + 4 + 8 + R * (label bytes + 9).
 *   Refused: a null item table, label table (n_labels > 0), count, status, workspace, label pointer, or data without an
 *   image (VX_E_NULL); n_items outside [1, VX_SELECT_MAX_ITEMS], n_labels outside [0, VX_COMPOSITE_MAX_LABELS], a
 *   dimension below 1, more than 2^40 voxels, R < 0 or a label range outside the table (VX_E_SHAPE); an unknown image or
 *   label kind (VX_E_DTYPE); a pointer off its element alignment or a workspace off 16 (VX_E_ALIGN); a short workspace
 *   (VX_E_WORKSPACE). */
#define VX_COMPOSITE_MAX_LABELS (1 << 20)
#define VX_LABEL_SIGNED 1
typedef struct vx_gather3d_item {
  const void* src;    /* device [dims[0]][dims[1]][dims[2]] */
  int32_t kind;       /* VX_PREP_* */
  int32_t dims[3];
  int32_t origin[3];  /* first voxel of the crop */
  int32_t reserved;
} vx_gather3d_item;
typedef struct vx_acc3d_item {
  float* sum;         /* device [T][C][X][Y][Z] */
  float* count;       /* device [X][Y][Z] */
  int32_t dims[3];    /* X, Y, Z */
  int32_t origin[3];  /* where the patch lands */
} vx_acc3d_item;
typedef struct vx_composite_label {
  const void* ptr;    /* device, n integers */
  int32_t kind;       /* VX_COUNT_B1 | B2 | B4 | B8 */
  int32_t flags;      /* 0 (unsigned elements) or VX_LABEL_SIGNED; any other bit: VX_E_DTYPE */
} vx_composite_label;
typedef struct vx_composite_item {
  const void* image;  /* device [X][Y][Z] of image_kind (null allowed when data is null) */
  const float* count; /* device [X][Y][Z]: patches per voxel */
  double* data;       /* device [X][Y][Z], or null */
  double* gt_seg;     /* device [R][X][Y][Z], or null */
  uint8_t* gt;        /* device [R][X][Y][Z], or null */
  int32_t image_kind; /* VX_PREP_* */
  int32_t first_label, R; /* labels[first_label .. first_label + R) */
  int32_t dims[3];
} vx_composite_item;
int64_t vx_gather_patches_3d_workspace_bytes(int n_items);
int vx_gather_patches_3d(const vx_gather3d_item* items /* host */, int n_items, float* out, int P0, int P1, int P2, void* workspace,
                         int64_t ws_bytes, vx_stream_t stream);
int64_t vx_softmax_accumulate_cases_workspace_bytes(int B);
int vx_softmax_accumulate_cases(const float* logits, int B, int T, int C, int P0, int P1, int P2, const vx_acc3d_item* items /* host */,
                                int sum_overlap, void* workspace, int64_t ws_bytes, vx_stream_t stream);
int64_t vx_case_composite_workspace_bytes(int n_items, int n_labels);
int vx_case_composite(const vx_composite_item* items /* host */, int n_items, const vx_composite_label* labels /* host */, int n_labels,
                      int32_t* status /* device [n_items] */, void* workspace, int64_t ws_bytes, vx_stream_t stream);

/* A whole training (or validation) batch of the 3D datamodules from resident file payloads, in ONE launch
 * (train_patches3d.hip; values_amd.datamodule3d.DeviceLoader3D): per item the crop of NumpyDataLoader
 * (toy_datamodule_3D.py:479-499), batchgenerators' MirrorTransform and GaussianNoiseTransform and the float cast of
 * NumpyToTensor, for the image and the drawn rater's label in the same pass.  Items mix cases, shapes and stored dtypes.
 *   data[i][x][y][z] = float32(image[o0 + m0(x)][o1 + m1(y)][o2 + m2(z)]),  m_a(t) = P_a - 1 - t when bit a of flags is
 *   set and t otherwise; the conversion is vx_gather_patches_3d's (numpy's astype(float32)).  With bit 3 set the value
 *   becomes fmaf(sigma_i, vx_gauss(seed', r, index), value): r the flat index in the output patch, seed' = seed +
 *   *seed_dev (nullable device word), sigma_i what vx_noise_view_3d derives for volume `index` from (var_lo, var_hi,
 *   sigma_law) -- the same field, bit for bit, as vx_noise_view_3d over the noise-free patch with index0 = index.
 *   THE REFERENCE ADDS ITS NOISE IN FLOAT64 BEFORE THE CAST TO FLOAT32; THIS CALL ADDS IT IN FLOAT32 AFTER THE CAST: at
 *   most one float32 rounding apart.  The distribution is the reference's, the stream this project's.
 *   seg[i] (nullable) = the same crop and mirror of the label as astype(intc) gives it, stored as float32 (seg_u8 == 0:
 *   what NumpyToTensor(cast_to="float") leaves) or as its low byte (seg_u8 != 0); a label outside 0..255 is counted in
 *   status[i] (device, zeroed by the call; integer atomics), read as vx_case_composite reads it (label_flags 0 |
 *   VX_LABEL_SIGNED).  An item without a label (null) gets zeros in seg.  Without seg no label is read.
 *   sigma_out (nullable, device [n_items]): sigma_i of the items with bit 3, 0 for the others.
 *   Lanes run along z, four consecutive z per lane, one access of up to 16 bytes where the four elements lie inside the
 *   row and the address is aligned to the access, element by element elsewhere; a z-mirror loads forward from the
 *   mirrored source address and reverses the four elements in registers.  Plain C++ stores.  No byte outside a crop or
 *   an output array is touched.  AN ITEM'S OUTPUT BYTES ARE EQUAL WHETHER IT IS SUBMITTED ALONE OR IN ANY BATCH, AT ANY
 *   POSITION.  Traffic per item: P0*P1*P2 * (esize + 4) bytes, plus P0*P1*P2 * (label bytes + 4 or 1) with seg.
 *   Refused before any device call: a null table, data, status, workspace or image (VX_E_NULL); n_items outside
 *   [1, VX_SELECT_MAX_ITEMS], P or a dimension below 1, a crop not inside its volume, P0*P1*P2 >= 2^32, var_lo < 0 or
 *   var_hi < var_lo (VX_E_SHAPE); an unknown image or label kind, flag bits above 3, label_flags other than 0 or
 *   VX_LABEL_SIGNED, another sigma_law (VX_E_DTYPE); a pointer off its element alignment or a workspace off 16
 *   (VX_E_ALIGN); a short workspace (VX_E_WORKSPACE).  A refused call writes nothing.  workspace:
 *   vx_train_patches_3d_workspace_bytes(n_items) bytes, 0 for counts the call refuses.  The item table goes up through a
 *   pinned staging buffer: no wait on the stream, not capturable into a hipGraph. */
enum { VX_TRAIN3D_MIRROR0 = 1, VX_TRAIN3D_MIRROR1 = 2, VX_TRAIN3D_MIRROR2 = 4, VX_TRAIN3D_NOISE = 8 };
typedef struct vx_train3d_item {
  const void* image;   /* device [dims[0]][dims[1]][dims[2]] of image_kind VX_PREP_* */
  const void* label;   /* device, same dims, or null */
  int32_t image_kind;
  int32_t label_kind;  /* VX_COUNT_B1 | B2 | B4 | B8 */
  int32_t label_flags; /* 0 | VX_LABEL_SIGNED */
  int32_t dims[3];
  int32_t origin[3];
  int32_t flags;       /* bits 0-2: mirror axis 0 / 1 / 2; bit 3: add noise */
  uint32_t index;      /* global sample index: keys the noise stream */
} vx_train3d_item;
int64_t vx_train_patches_3d_workspace_bytes(int n_items);
int vx_train_patches_3d(const vx_train3d_item* items /* host */, int n_items, int P0, int P1, int P2, float* data,
                        void* seg /* nullable */, int seg_u8, uint32_t seed, const uint32_t* seed_dev, float var_lo, float var_hi,
                        int sigma_law, float* sigma_out /* nullable [n_items] */, int32_t* status /* device [n_items] */,
                        void* workspace, int64_t ws_bytes, vx_stream_t stream);

/* Metric reductions behind calculate_test_metrics / calculate_ged (test_3D.py:250-358): see metrics.hip.
 * vx_mask_agreement: masks [M][nvox] uint8 labels < C; counts [M][M][C] uint64 (zeroed here),
 *   counts[i][j][c] = #{v: mask_i(v) == c and mask_j(v) == c}.  M <= 32, C <= 8.
 * vx_mask_agreement_batched (the metrics half of process_output, test_2D.py:205-244): the same counts for the B images of
 *   a 2D inference step at once.  masks [B][M][nvox] uint8, counts [B][M][M][C] uint64 (zeroed here, the full array, not a
 *   triangle).  1 <= M <= 32, 1 <= C <= 32, B >= 1, 0 <= nvox <= 2^39; anything else is VX_E_SHAPE before any launch.
 *   A label equal to remap_from counts as class C - 1 (the reference's gt[gt == 255] = C - 1 for the appended "ignore"
 *   class, done on load; remap_from outside 0..255: none); any other label >= C counts for no class.  One memset + one
 *   launch on the stream, no synchronisation, no descriptor upload: capturable into a hipGraph.
 * vx_soft_metric_sums: prob [C][nvox] float32 (mean softmax), gt [R][nvox] uint8; sums [R][3*C+1] float64:
 *   for each class (sum p_c [gt==c], sum [gt==c], sum p_c), then sum_v log p_{gt(v)}(v);
 *   workspace of vx_soft_metric_workspace_bytes(C, R).
 * vx_soft_metric_sums_batched (the SoftDice + NLL half of calculate_metrics, test_3D.py:537-575, for a whole step): the sums of
 *   vx_soft_metric_sums for B images in one pass over the data.  prob [B][C][nvox] float32, gt [B][R][nvox] uint8,
 *   sums [B][R][3*C+1] float64 in the one-image layout.  1 <= C <= 32, 1 <= R <= 31, B >= 1, 1 <= nvox <= 2^39; anything
 *   else is VX_E_SHAPE, a null pointer VX_E_NULL, both before any device call.  A label >= C counts for no class and takes no
 *   log term.  Deterministic: fixed summation order, no atomics, and an image's sums do not depend on B or on its batch
 *   mates (bit-equal to the same image submitted alone).  workspace of vx_soft_metric_batched_workspace_bytes(B, C, R, nvox)
 *   (0 for arguments the call refuses; B times the value for one image).  Two launches on the stream, no synchronisation:
 *   capturable into a hipGraph. */
int vx_mask_agreement(const uint8_t* masks, int M, int C, int64_t nvox, uint64_t* counts, vx_stream_t stream);
int vx_mask_agreement_batched(const uint8_t* masks, int B, int M, int C, int64_t nvox, int remap_from, uint64_t* counts,
                              vx_stream_t stream);
int64_t vx_soft_metric_workspace_bytes(int C, int R);
int vx_soft_metric_sums(const float* prob, const uint8_t* gt, int C, int R, int64_t nvox, double* sums, void* workspace,
                        vx_stream_t stream);
int64_t vx_soft_metric_batched_workspace_bytes(int B, int C, int R, int64_t nvox);
int vx_soft_metric_sums_batched(const float* prob, const uint8_t* gt, int B, int C, int R, int64_t nvox, double* sums,
                                void* workspace, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * The validation step's reductions (LightningExperiment.validation_step and forward_ssn(val=True),
 * lightning_experiment.py:175-219, 278-377), see valstep.hip: what turns a model's output and a label volume into
 * validation/val_loss and validation/val_dice.  The head is read once, no sample is written.
 *
 * labels [B][nvox] uint8.  ignore_label is -1 (none) or 0..255: a voxel whose label equals it takes no log term; a label
 *   >= C other than ignore_label belongs to no class, takes no log term and is counted as INVALID (torch raises there, and
 *   so does values_amd.validation).  Arg-max ties go to the lowest class index.
 * Arithmetic: the sample logits are float32, formed with vx_aleatoric_sample's y = fmaf(exp(s / 2), eps, mu) and
 *   vx_ssn_sample's y = (mean + sum_r factor_r eps_w) + sqrt(exp(logd) + epsilon) eps_d; everything after them -- the
 *   maximum, exp, log and every sum -- is float64 (the exact order is in valstep.hip's header and restated by
 *   tests/valstep_ref.py).  Span partials, a fixed shuffle tree, a finalize launch in span order, no atomics: an item's
 *   numbers are bit-equal whether it is submitted alone or with batch mates.  Two launches on the stream, no
 *   synchronisation: capturable into a hipGraph.
 *
 * vx_val_sums_batched (the deterministic branch; any layout [B][C][nvox], 3D or NCHW): logits float32, 1 <= C <= 32,
 *   1 <= nvox <= 2^39.  sums [B][5C + 3] float64: per class c  sum softmax_c [t = c],  sum [t = c],  sum softmax_c,
 *   tp_c = #{argmax = c and t = c},  pred_c = #{argmax = c};  then  sum log_softmax_t  over the voxels that take a log
 *   term, the count of those voxels, and the invalid count.
 * vx_val_aleatoric_sums_batched: mu_s [B][2C][nvox] (mu | s), eps [B][T][C][nvox] injected or NULL (generated from
 *   `seed`), 2 <= C <= 8, 1 <= T <= 32, C * nvox < 2^32.  Per voxel and sample the log-softmax over classes of y_t, then
 *   lavg_c = logsumexp_t - log T; sums as above with p = exp(lavg), the log term lavg_t and the arg-max of lavg.
 * vx_val_ssn_sums_batched: head [B][(2 + R)C][nvox] in vx_ssn_sample's layout (R = 0: the mean_only pretraining branch),
 *   eps_w [S][B][R] and eps_d [S][B][C * nvox] injected or NULL (generated), 2 <= C <= 8, 1 <= S <= 32, 0 <= R <= 32,
 *   C * nvox < 2^32.  sample_sums [B][S][1 + 2C]: sum_v log_softmax(y_s)[t], tp_c, pred_c of sample s;
 *   target_sums [B][C + 2]: sum [t = c], the count of voxels that take a log term, the invalid count.
 * Generated normals are keyed by the GLOBAL item index item0 + b: with item0 = 0 they are the streams vx_aleatoric_sample /
 *   vx_ssn_sample draw for the same seed (slot (item0 + b) * T + t, resp. * S + s), and for any item0 an item's result does
 *   not depend on how a set of items is cut into calls.  Injected normals are indexed by the call's own b.
 * Refused before any launch: B outside [1, 65535], C, T, S, R, nvox or ignore_label out of range (VX_E_SHAPE); a null
 *   logits / head / labels / output / workspace (VX_E_NULL); workspace_bytes below *_workspace_bytes(...) (VX_E_WORKSPACE;
 *   the companions return 0 for shapes the call refuses). */
int64_t vx_val_sums_workspace_bytes(int B, int C, int64_t nvox);
int vx_val_sums_batched(const float* logits, const uint8_t* labels, int B, int C, int64_t nvox, int ignore_label, double* sums,
                        void* workspace, int64_t workspace_bytes, vx_stream_t stream);
int64_t vx_val_aleatoric_sums_workspace_bytes(int B, int C, int64_t nvox);
int vx_val_aleatoric_sums_batched(const float* mu_s, const float* eps, uint32_t seed, uint32_t item0, const uint8_t* labels, int B,
                                  int T, int C, int64_t nvox, int ignore_label, double* sums, void* workspace,
                                  int64_t workspace_bytes, vx_stream_t stream);
int64_t vx_val_ssn_sums_workspace_bytes(int B, int S, int C, int64_t nvox);
int vx_val_ssn_sums_batched(const float* head, const float* eps_w, const float* eps_d, uint32_t seed, uint32_t item0,
                            const uint8_t* labels, int B, int S, int C, int R, int64_t nvox, float epsilon, int ignore_label,
                            double* sample_sums, double* target_sums, void* workspace, int64_t workspace_bytes,
                            vx_stream_t stream);

/* vx_val_ssn2d_sums_batched: the same sums for the 2D SSN head (HighResolutionNet.hrnet_ssn), whose mean and factor live
 *   at the head's resolution h0 x w0, channels-last, exactly as vx_ssn2d_lowres takes them (mean_lo [B*h0*w0][mean_pitch],
 *   factor_lo [B*h0*w0][factor_pitch], channel r*C + c; R = 0 is mean_only and factor_lo may be NULL).  The samples of the
 *   H x W image are the ones vx_ssn2d_lowres -> vx_bilinear_nchw -> vx_ssn2d_add_diag write, bit for bit:
 *       y_s,c = interp(mean + sum_r factor_r eps_w)_c + sqrtf(interp(expf(mean))_c + epsilon) * eps_d
 *   with interp the bilinear upsample of F.interpolate(align_corners=False) -- but no full-resolution value is written.
 *   eps_w [S][B][R], eps_d [S][B][C*H*W] injected or NULL: generated, eps_d = vx_gauss(seed, c*H*W + pixel, (item0 + b)*S + s),
 *   eps_w = vx_gauss(seed ^ 0x5bd1e995, r, (item0 + b)*S + s) -- with item0 = 0 the streams of the three calls above.
 *   labels [B][H*W]; sample_sums [B][S][1 + 2C], target_sums [B][C + 2] and the float64 arithmetic as vx_val_ssn_sums_batched.
 *   2 <= C <= 32, 1 <= S <= 32, 0 <= R <= 32, 1 <= B <= 65535, every side in 1..65536, C*H*W < 2^32, B*h0*w0 < 2^32,
 *   mean_pitch >= C, factor_pitch >= R*C (R > 0), ignore_label in -1..255: anything else VX_E_SHAPE; a null mean_lo, labels,
 *   output or workspace (or factor_lo with R > 0) VX_E_NULL; a short workspace VX_E_WORKSPACE -- all before any launch.
 *   The workspace holds the low-resolution combination ([S + 1][B*h0*w0][C] float32) and the span partials.  Three launches
 *   on the stream, no synchronisation; counts are integer sums, the float64 sums go through the fixed tree: an item's rows
 *   are bit-equal alone (item0 = k) and as row k of a batch. */
int64_t vx_val_ssn2d_sums_workspace_bytes(int B, int S, int C, int h0, int w0, int H, int W);
int vx_val_ssn2d_sums_batched(const float* mean_lo, int mean_pitch, const float* factor_lo, int factor_pitch, const float* eps_w,
                              const float* eps_d, uint32_t seed, uint32_t item0, const uint8_t* labels, int B, int S, int C, int R,
                              int h0, int w0, int H, int W, float epsilon, int ignore_label, double* sample_sums,
                              double* target_sums, void* workspace, int64_t workspace_bytes, vx_stream_t stream);

/* 2D SSN head (HighResolutionNet.hrnet_ssn, hrnet_module.py:559-595), see accumulate.hip:
 * vx_ssn2d_lowres: channels-last head outputs at the head's resolution -- mean [B*pix][mean_pitch] (C used),
 *   factor [B*pix][factor_pitch] (channel r*C + c) -- and eps_w [S][B][R] (nullable: generated) ->
 *   comb [S][B*pix][C] = mean + sum_r factor_r * eps_w,  expm [B*pix][C] = exp(mean) (nullable).
 *   mean_pitch >= C, factor_pitch >= R*C, B * pix < 2^32, B * S < 2^31; anything else is VX_E_SHAPE, a null mean or comb
 *   (or factor with R > 0) VX_E_NULL, both before any launch.
 * vx_ssn2d_add_diag: out [B][S][per] += sqrt(diag [B][per] + epsilon) * eps_d [S][B][per] (nullable: generated).
 *   0 < per < 2^32. */
int vx_ssn2d_lowres(const float* mean, int mean_pitch, const float* factor, int factor_pitch, const float* eps_w,
                    uint32_t seed, int B, int64_t pix_per_image, int S, int C, int R, float* comb, float* expm,
                    vx_stream_t stream);
int vx_ssn2d_add_diag(float* out, const float* diag, const float* eps_d, uint32_t seed, int S, int B, int64_t per,
                      float epsilon, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Downstream scalars of the evaluation stage (evaluation/metrics/{ncc,ace}.py): the per-voxel float64 reductions for a
 * batch of images in one call each (evalmetrics.hip); one image is a batch of one.  All sums are deterministic and formed
 * with ONE association, which is the contract of these calls: thread t of block b adds elements
 * b * 256 + t + k * 131072 in ascending k, a 64-lane shuffle tree, four waves in order, 512 block rows in index order; no
 * multiply-add is fused.  An item's numbers do not depend on its batch mates or on n_items: they are bit-equal to the
 * same item submitted alone.  Items of a call may differ in size, R and dtype.
 *   items      HOST array of descriptors of DEVICE buffers.  1 <= n_items <= VX_EM_MAX_ITEMS, R >= 1, nvox >= 1.
 *   vx_ncc_batched         (ncc.py:9-25: numpy's two-pass mean / std(ddof=1) / product)  sums [n_items][5] (device) =
 *                          sum gt, sum pred, sum (gt-mg)^2, sum (pred-mp)^2, sum (gt-mg)(pred-mp) with
 *                          mg = sums[0] / (double)n, mp = sums[1] / (double)n, one IEEE division each, formed on the
 *                          device between the passes.  Four launches, no synchronisation.
 *                          The ground-truth side is a map (gt_R = 0, gt_dtype VX_F32 | VX_F64) or
 *                          gt_R >= 1 int32 label volumes [gt_R][n]: then every voxel's value is np.var(labels, axis=0),
 *                          evaluated on the fly in float64 in numpy's order (sum over raters in index order, / R, sum
 *                          of (x - mean)^2 in index order, / R); the variance map is never written.  n_gt != n_pred is
 *                          refused.
 *   vx_rater_variance      that variance as a float64 map [nvox] of its own (one launch).
 *   vx_platt_sums_batched  (ace.py:13-41, sklearn.calibration._sigmoid_calibration on (-unc, reference == prediction))
 *                          per item: ref [R][nvox] int32 reference segmentations, pred [nvox] int32 mean prediction,
 *                          unc [nvox] f32/f64; voxels with ref == ignore_value dropped (ignore_value < 0: none; one
 *                          ignore_value for the call).  params: HOST [n_items][4] = the sigmoid parameters and Platt's
 *                          targets (A, B, t_pos, t_neg) per item.  sums [n_items][8] (device): [0] = valid count,
 *                          [1] = correct count, [2] = loss, [3..4] = gradient (dA, dB), [5..7] = Hessian (AA, AB, BB).
 *                          The host iterates (Newton).  Two launches.
 *   vx_calib_bins_batched  (ace.py:44-90) platt_scale_confid + calib_stats' 20-bin statistics: bins63 [n_items][63]
 *                          (device) = bin_sums[21], bin_true[21], bin_total[21] per item for the bin edges edges21 (a
 *                          HOST array: np.linspace(0, 1 + 1e-8, 21)); ab: HOST [n_items][2] = (A, B) per item.  A voxel
 *                          lies in bin np.digitize(prob, edges21) - 1: the last edge <= prob.  A NaN prob (a NaN in
 *                          the map) counts in bin 20 as np.digitize puts it: its correctness goes to bin_true[20], 1
 *                          to bin_total[20], and bin_sums[20] becomes NaN, so the ACE of such an image is NaN as the
 *                          reference's.  Two launches.
 * Every argument check (VX_E_NULL / VX_E_SHAPE / VX_E_DTYPE, the message names the item; VX_E_WORKSPACE / VX_E_ALIGN)
 * returns before any device call.  workspace: caller-owned, of vx_*_batched_workspace_bytes(the same items) bytes --
 * the descriptor table and 512 partial rows per item -- 0 for arguments the call refuses.  The descriptor table goes up
 * through a pinned staging buffer: a call does not wait for the stream (only, if it is still in flight, for the previous
 * call's upload), and it is not capturable into a hipGraph. */
#define VX_EM_MAX_ITEMS 4096
typedef struct vx_em_item {
  const void* unc;     /* device [nvox], VX_F32 | VX_F64 */
  const int32_t* ref;  /* device [R][nvox] reference segmentations */
  const int32_t* pred; /* device [nvox] mean prediction */
  int64_t nvox;
  int32_t dtype, R;
} vx_em_item;
typedef struct vx_ncc_item {
  const void* gt;       /* gt_R == 0: device map [n_gt] of gt_dtype;  gt_R >= 1: device int32 labels [gt_R][n_gt] */
  const void* pred;     /* device map [n_pred] of pred_dtype */
  int64_t n_gt, n_pred; /* must be equal */
  int32_t gt_dtype, pred_dtype, gt_R, reserved;
} vx_ncc_item;
size_t vx_ncc_batched_workspace_bytes(const vx_ncc_item* items, int n_items);
int vx_ncc_batched(const vx_ncc_item* items /* host */, int n_items, double* sums /* device */, void* workspace,
                   size_t workspace_bytes, vx_stream_t stream);
int vx_rater_variance(const int32_t* labels, int R, int64_t nvox, double* variance, vx_stream_t stream);
size_t vx_platt_batched_workspace_bytes(const vx_em_item* items, int n_items);
int vx_platt_sums_batched(const vx_em_item* items /* host */, int n_items, const double* params /* host */, int ignore_value,
                          double* sums /* device */, void* workspace, size_t workspace_bytes, vx_stream_t stream);
size_t vx_calib_batched_workspace_bytes(const vx_em_item* items, int n_items);
int vx_calib_bins_batched(const vx_em_item* items /* host */, int n_items, const double* ab /* host */,
                          const double* edges21 /* host */, int ignore_value, double* bins63 /* device */, void* workspace,
                          size_t workspace_bytes, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * K38: map -> scalar aggregations (evaluation/uncertainty_aggregation/aggregate_uncertainties.py:13-67) for a batch of
 * maps in one call; one map is a batch of one.
 *   items  host array: a device map [D][H][W] (a 2D map: D = 1) of VX_F32 or VX_F64 each; shapes and dtypes may differ.
 *   specs  host array, shared by all items.  kind IMAGE: image_level_aggregation (:34-37), the sum of the map.
 *          THRESHOLD: threshold_aggregation (:61-67), sum and count of the elements with x >= thr.  PATCH:
 *          patch_level_aggregation (:13-31), maximum of the 'valid' (pd, ph, pw) box sums and the first C-order index
 *          close to it.
 *   out    device [n_items][n_specs][4] float64:  IMAGE {sum, 0, 0, 0};  THRESHOLD {sum, count, 0, 0};
 *          PATCH {maximum, d, h, w} (the index as exact integers).
 * The order of every float64 operation is part of the contract (tests/agg_restated.py restates it on the host, and the
 * results are compared with ==); a map's results do not depend on its batch mates, the tiling or the workspace:
 *   sums   element i of the flattened map belongs to lane i % 1024; a lane adds its elements, widened to float64, in
 *          ascending i from 0.0.  It keeps three accumulators: the sum, the sum of the elements with x >= thr and their
 *          count, the comparison in float64 on both sides (a map read back from NIfTI is float64, and so is the
 *          reference's threshold).  In every wave of 64 lanes the xor butterfly v = v + v[lane ^ off] runs for off = 1, 2,
 *          4, 8, 16, 32; the 16 wave results are added in wave order from 0.0.
 *   box    a float64 map is narrowed to float32 first; every element is then widened to float64.  Box sums along W, then
 *          along H, then along D: each starts from 0.0 and adds its p terms in ascending k (an axis with p = 1 keeps its
 *          0.0 + x).  The maximum over all box sums, then the first C-order index with |v - max| <= 1e-8 + 1e-5 |max|
 *          (np.isclose with b = max), unravelled over (D - pd + 1, H - ph + 1, W - pw + 1).
 * 1 <= n_items <= 4096, 1 <= n_specs <= 8, every map has at least one element, a patch must fit every item's map (the
 * message names the item), and a patch so large that no LDS tile holds its halo is refused: VX_E_SHAPE, before any
 * device call.  All IMAGE / THRESHOLD specs of an item come from one read of its map (one workgroup per item); the box
 * sums run on LDS tiles and keep two 8-byte words per tile in the workspace, never the box sums themselves.  At most
 * four launches, whatever n_items and n_specs are.  The descriptor tables go up through a pinned staging buffer: the
 * call does not wait for the stream (only, if it is still in flight, for the previous call's upload), and it is not
 * capturable into a hipGraph.
 * workspace of vx_aggregate_workspace_bytes(the same arguments), 0 for arguments the call refuses. */
#define VX_AGG_IMAGE 0
#define VX_AGG_THRESHOLD 1
#define VX_AGG_PATCH 2
typedef struct vx_agg_item {
  const void* map;
  int32_t dtype; /* VX_F32 | VX_F64 */
  int32_t D, H, W;
} vx_agg_item;
typedef struct vx_agg_spec {
  int32_t kind; /* VX_AGG_* */
  int32_t pd, ph, pw;
  double thr;
} vx_agg_spec;
size_t vx_aggregate_workspace_bytes(const vx_agg_item* items, int n_items, const vx_agg_spec* specs, int n_specs);
int vx_aggregate_batched(const vx_agg_item* items /* host */, int n_items, const vx_agg_spec* specs /* host */, int n_specs,
                         double* out /* device */, void* workspace, size_t workspace_bytes, vx_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Device results writer (data_carrier_3D.py:208-371, DataCarrier3D.save_data; host mirror: values_amd/results.py
 * save_case).  The NIfTI payloads of a case are assembled on the device (vx_nifti_payload), compressed to gzip members
 * on the device (vx_gzip_encode), and the host only copies the members back and writes the files.
 * These two entry points upload a small descriptor table from their own host copy and wait for that copy on the stream
 * (hipStreamSynchronize) before they launch: they are not capturable into a hipGraph.
 *
 * vx_nifti_payload: one launch writes every item's payload at dst + dst_off: the 352-byte header (348 bytes + 4 zero
 *   extension bytes, built by the caller: values_amd.nifti.header_bytes) and the voxels in Fortran order -- element
 *   src[x][y][z] of a C-order (X, Y, Z) volume at index (z * Y + y) * X + x.  kind:
 *     COPY        src (X, Y, Z) of esize (1/2/4/8) bytes per element, copied as it is
 *     PROB        src (T, C, X, Y, Z) VX_F32 / VX_F64 probabilities -> float64 src[t][c] / float64(clip(count, 1))
 *                 (count: optional (X, Y, Z) float64 divisor; null = none)
 *     MEAN_PROB   float64 sum of PROB over t = 0..T-1 added in that order, divided by T
 *     ARGMAX      uint8 first index of the maximum over c of PROB[t] (a NaN is the maximum: np.argmax)
 *     ARGMAX_MEAN the same over MEAN_PROB
 *   dst 16-byte aligned, dst_off a multiple of 16, every payload within dst_bytes; workspace: vx_nifti_workspace_bytes.
 *   vx_nifti_payload_bytes: 352 + voxels * output element size (host only).
 * vx_gzip_encode: one complete gzip member (RFC 1952: 10-byte header with MTIME 0, DEFLATE stream, CRC-32, ISIZE) of
 *   each item's n bytes at dst + dst_off (the slot needs vx_gzip_bound(n) bytes within dst_bytes); the member's size goes
 *   to out_sizes[i] (device).  stride_hint: distances (element, row, slice bytes; 0 = none, each <= 32768) the match
 *   finder tries besides its hash table.  The output is deterministic.  workspace: vx_gzip_workspace_bytes(sizes, n).
 * vx_gzip_bound: worst-case member size of n input bytes (n + 5 per 32 KiB chunk + 18; <= n + n/1000 + 64 from
 *   n >= 1 MiB); host only.
 * vx_crc32: out[0] = CRC-32 (ISO-HDLC, zlib.crc32) of n bytes at x (any alignment). */
enum { VX_NIFTI_COPY = 0, VX_NIFTI_PROB = 1, VX_NIFTI_MEAN_PROB = 2, VX_NIFTI_ARGMAX = 3, VX_NIFTI_ARGMAX_MEAN = 4 };
typedef struct vx_nifti_item {
  const void* src;
  const double* count;   /* PROB kinds: optional (X, Y, Z) float64 divisor */
  int64_t dst_off;
  int32_t kind;
  int32_t src_dtype;     /* PROB kinds: VX_F32 / VX_F64 */
  int32_t esize;         /* COPY: bytes per element */
  int32_t T, C, t, c;
  int32_t X, Y, Z;
  uint8_t header[352];
} vx_nifti_item;
size_t vx_nifti_workspace_bytes(int n_items);
int64_t vx_nifti_payload_bytes(const vx_nifti_item* item);
int vx_nifti_payload(const vx_nifti_item* items /* host array */, int n_items, uint8_t* dst, int64_t dst_bytes, void* workspace,
                     size_t ws_bytes, vx_stream_t stream);

typedef struct vx_gz_item {
  const void* src;
  int64_t n;
  int64_t dst_off;
  int32_t stride_hint[3];
  int32_t pad;
} vx_gz_item;
int64_t vx_gzip_bound(int64_t n);
size_t vx_gzip_workspace_bytes(const int64_t* sizes /* host array */, int n_items);
int vx_gzip_encode(const vx_gz_item* items /* host array */, int n_items, uint8_t* dst, int64_t dst_bytes,
                   int64_t* out_sizes /* device */, void* workspace, size_t ws_bytes, vx_stream_t stream);
int vx_crc32(const void* x, int64_t n, uint32_t* out /* device */, vx_stream_t stream);

/* The 2D results tree (Tester.save_prediction, test_2D.py:116-141; host mirror: values_amd/results2d.py save_prediction).
 * vx_png_encode: one complete 8-bit RGB PNG file (signature, IHDR, one IDAT holding a zlib stream -- header 78 01, raw
 *   DEFLATE, Adler-32 -- and IEND) per item, colouring each label through lut (device, 256 x 3 RGB bytes); pixels
 *   whose ignore byte is non-zero take lut[unlabeled].  Every scanline has filter 0: the inflated IDAT is exactly the
 *   raw stream image_io.write_png compresses.  labels / ignore: device (H, W) uint8, C order; ignore may be null.  The
 *   files are written back to back in item order from dst + 0; out_offsets[i] / out_sizes[i] (device) receive file i's
 *   place.  dst_bytes must cover the sum of vx_png_bound over the items, the workspace (16-byte aligned) at least
 *   vx_png_workspace_bytes(items, n) bytes.  H * (3 W + 1) < 2^31.  The output is deterministic.  Like vx_gzip_encode it
 *   uploads its descriptor table and synchronises the stream before it launches: not capturable into a hipGraph.
 * vx_png_bound: worst-case file size of an H x W item: n = H * (3 W + 1) scanline bytes as stored blocks
 *   (n + 5 per 32 KiB chunk) plus 63 bytes of PNG and zlib framing; host only, -1 for H or W < 1.
 * vx_png_workspace_bytes: 0 for a null table, n < 1 or an item with H or W < 1.
 * vx_png_encode_rgb: the same files from pixels that are RGB bytes already (rgb: device [H][W][3], any alignment)
 *   instead of labels through a table -- the vis/ images of the 2D preprocessing (K43).  Layout, filter-0 scanlines, zlib
 *   framing, limits, refusals and the DEFLATE chunk launch are vx_png_encode's (one host routine serves both); the only
 *   difference is where a scanline byte comes from.  vx_png_bound serves both; workspace:
 *   vx_png_encode_rgb_workspace_bytes(items, n). */
typedef struct vx_png_item {
  const uint8_t* labels;
  const uint8_t* ignore;
  int32_t H, W;
} vx_png_item;
typedef struct vx_png_rgb_item {
  const uint8_t* rgb;
  int32_t H, W;
} vx_png_rgb_item;
int64_t vx_png_bound(int H, int W);
size_t vx_png_workspace_bytes(const vx_png_item* items /* host array */, int n);
int vx_png_encode(const vx_png_item* items /* host array */, int n, const uint8_t* lut, int unlabeled, uint8_t* dst,
                  int64_t dst_bytes, int64_t* out_offsets /* device */, int64_t* out_sizes /* device */, void* workspace,
                  size_t ws_bytes, vx_stream_t stream);
size_t vx_png_encode_rgb_workspace_bytes(const vx_png_rgb_item* items /* host array */, int n);
int vx_png_encode_rgb(const vx_png_rgb_item* items /* host array */, int n, uint8_t* dst, int64_t dst_bytes,
                      int64_t* out_offsets /* device */, int64_t* out_sizes /* device */, void* workspace, size_t ws_bytes,
                      vx_stream_t stream);

/* Reading the results tree back (ExperimentDataloader, aggregate_uncertainties, find_threshold: every consumer of
 * nifti.load; Python: values_amd.gz.gunzip, values_amd.nifti.load_device).
 *
 * vx_inflate: decodes each item's compressed bytes (src, src_n: device) into dst[dst_off, dst_off + dst_cap).  format:
 *   GZIP  RFC 1952, every header flag (FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT); several members decode to their
 *         concatenation, zero padding between or after members is skipped (gzip.decompress); each member's CRC-32 and
 *         ISIZE are checked;
 *   ZLIB  RFC 1950 with the Adler-32 checked; a preset dictionary is VX_INFLATE_DICT;
 *   RAW   a bare RFC 1951 stream.
 *   Statuses are per item: out_status[i] (device) is VX_INFLATE_OK or one of the codes below, out_sizes[i] (device) the
 *   bytes written into the item's window, also on error.  The return value is reserved for argument errors (refused
 *   before any launch) and hipError_t.  No input reads outside [src, src + src_n) or writes outside the item's window,
 *   and every loop of the decoder makes progress on input or output.  The windows must not overlap each other or any
 *   source.  workspace: vx_inflate_workspace_bytes(n_items) bytes, 16-byte aligned.  Like vx_gzip_encode it uploads its
 *   descriptor table and synchronises the stream before it launches: not capturable into a hipGraph.
 * vx_nifti_decode: the inverse of vx_nifti_payload.  Per item, the voxels of a decoded NIfTI-1 payload (src: header +
 *   voxels in Fortran order at vox_offset, src_n bytes) go to dst as the C-order array nifti.load returns, indexed
 *   [x, y, z, ...] (ndim 1..7, dims[0..ndim)): byte-swapped when big_endian, and when scaled, v * slope + inter computed
 *   in the output type (out_dtype VX_F32: float32 operands; VX_F64: float64) as numpy promotes a * slope + inter;
 *   unscaled, out_dtype is -1 and the elements keep the file's type.  code: the NIfTI datatype (2, 4, 8, 16, 64, 256, 512,
 *   768, 1024, 1280).  src_n must cover vox_offset + voxels * element size, dst_n the output.  workspace:
 *   vx_nifti_decode_workspace_bytes(n_items).  Uploads its table and synchronises the stream, as vx_inflate. */
enum { VX_INFLATE_GZIP = 0, VX_INFLATE_ZLIB = 1, VX_INFLATE_RAW = 2 };
enum {
  VX_INFLATE_OK = 0,
  VX_INFLATE_TRUNCATED = 1,     /* the input ends inside the stream, its header or its trailer */
  VX_INFLATE_BAD_HEADER = 2,    /* gzip magic / method / reserved flags, zlib method / window / check bits */
  VX_INFLATE_BAD_BLOCK = 3,     /* block type 3 */
  VX_INFLATE_BAD_LENGTHS = 4,   /* invalid, over-subscribed or incomplete code lengths; HLIT > 286, HDIST > 30 */
  VX_INFLATE_BAD_SYMBOL = 5,    /* bits that are no code, literal/length 286 / 287, distance 30 / 31 */
  VX_INFLATE_BAD_DISTANCE = 6,  /* a distance reaching before the start of the member's output */
  VX_INFLATE_CAPACITY = 7,      /* the output window is full and the stream has more */
  VX_INFLATE_BAD_CHECK = 8,     /* CRC-32 (gzip) or Adler-32 (zlib) mismatch */
  VX_INFLATE_BAD_ISIZE = 9,     /* gzip ISIZE mismatch */
  VX_INFLATE_TRAILING = 10,     /* bytes after the stream (after zero padding for gzip) */
  VX_INFLATE_BAD_STORED = 11,   /* stored block whose NLEN is not the complement of LEN */
  VX_INFLATE_DICT = 12          /* zlib preset dictionary */
};
typedef struct vx_inflate_item {
  const uint8_t* src;
  int64_t src_n;
  int64_t dst_off;
  int64_t dst_cap;
  int32_t format;
  int32_t pad;
} vx_inflate_item;
int64_t vx_inflate_workspace_bytes(int n_items);
int vx_inflate(const vx_inflate_item* items /* host array */, int n_items, uint8_t* dst, int64_t dst_n,
               int64_t* out_sizes /* device */, int32_t* out_status /* device */, void* workspace,
               int64_t workspace_bytes, vx_stream_t stream);

typedef struct vx_nifti_dec_item {
  const uint8_t* src;
  int64_t src_n;
  int64_t vox_offset;
  void* dst;
  int64_t dst_n;
  int32_t ndim;
  int32_t dims[7];
  int32_t code;
  int32_t big_endian;
  int32_t out_dtype;   /* -1: the file's type; VX_F32 / VX_F64: scaled */
  int32_t pad;
  double slope, inter;
} vx_nifti_dec_item;
int64_t vx_nifti_decode_workspace_bytes(int n_items);
int vx_nifti_decode(const vx_nifti_dec_item* items /* host array */, int n_items, void* workspace,
                    int64_t workspace_bytes, vx_stream_t stream);

/* Reading the 2D results tree back (values_amd/images.py: load_png_device; values_amd/gta.py: pred_seg_loading_device) --
 * what follows vx_inflate(format = ZLIB) of a PNG's joined IDAT chunks.
 *
 * vx_png_unfilter: per item, the inflated scanline stream of an 8-bit non-interlaced PNG (src, src_n bytes: device; H rows
 *   of one filter byte and W * bpp pixel bytes; bpp 1 / 3 / 4 = grey / RGB / RGBA) is reconstructed into dst (device,
 *   H * W * bpp bytes, C order).  All five filters as RFC 2083 section 6: Paeth ties resolve a, then b, then c; Average
 *   is (a + b) >> 1 on the unclamped 9-bit sum; the row above the first and the pixel left of the first are zero.
 *   Statuses are per item: out_status[i] (device) is VX_PNG_OK, VX_PNG_BAD_FILTER (a filter byte above 4) or
 *   VX_PNG_BAD_SIZE (src_n != H * (1 + W * bpp)); such an item's dst is left as it was, the others decode.  The return
 *   value is reserved for argument errors (refused before any launch: a null table or pointer, bpp other than 1 / 3 / 4,
 *   H or W < 1, a row of more than 65536 pixel bytes, H * (1 + W * bpp) >= 2^31) and hipError_t.  No read outside
 *   [src, src + src_n), no write outside dst; src and dst may have any alignment.  workspace:
 *   vx_png_unfilter_workspace_bytes(n_items) bytes, 16-byte aligned.  Like vx_inflate it uploads its table and
 *   synchronises the stream before it launches: not capturable into a hipGraph.
 * vx_rgb_to_trainid: out[i] = the id of the table entry whose key is pixel i's 0x00RRGGBB (rgb: n pixels at pitch 3), else
 *   default_id -- color2trainId.get(tuple(x), 128) of evaluation/utils/gta.py:9-11.  table: device, n_table <= 256 pairs
 *   (key, id) of uint32; of two entries with one key the later one counts.  Plain launch: capturable. */
enum { VX_PNG_OK = 0, VX_PNG_BAD_FILTER = 1, VX_PNG_BAD_SIZE = 2 };
typedef struct vx_png_unfilter_item {
  const uint8_t* src;
  int64_t src_n;
  uint8_t* dst;
  int32_t H, W;
  int32_t bpp;
  int32_t pad;
} vx_png_unfilter_item;
int64_t vx_png_unfilter_workspace_bytes(int n_items);
int vx_png_unfilter(const vx_png_unfilter_item* items /* host array */, int n_items, int32_t* out_status /* device */,
                    void* workspace, int64_t workspace_bytes, vx_stream_t stream);
int vx_rgb_to_trainid(const uint8_t* rgb, int64_t n, const uint32_t* table /* device */, int n_table, int default_id,
                      uint8_t* out, vx_stream_t stream);

/* LZW-compressed float32 TIFF maps (Compression 5; values_amd/images.py: load_tiff_device) -- what libtiff writes for a
 * float32 image: cv2.imwrite, PIL, GDAL, ImageJ.
 *
 * vx_tiff_lzw: decodes each item's LZW strip (src, src_n: device; TIFF 6.0 section 13: codes MSB first, 9 to 12 bits,
 *   ClearCode 256, EndOfInformation 257, early change; with a full table and no ClearCode the decode goes on at 12 bits
 *   without new entries) into dst[dst_off, dst_off + dst_cap).  A strip's first code must be ClearCode.  An item ends
 *   with VX_LZW_OK when its window is full, whatever follows (a string reaching beyond the window is cut there), and at
 *   EndOfInformation, where a window not yet full shows in out_sizes[i].  Statuses are per item: out_status[i] (device)
 *   is VX_LZW_OK or one of the codes below, out_sizes[i] (device) the bytes written into the item's window, also on
 *   error.  The return value is reserved for argument errors (refused before any launch) and hipError_t.  No input reads
 *   outside [src, src + src_n) or writes outside the item's window, and every loop of the decoder makes progress on input
 *   or output.  The windows must not overlap each other or any source.  workspace: vx_tiff_lzw_workspace_bytes(n_items)
 *   bytes, 16-byte aligned.  Like vx_inflate it uploads its table and synchronises the stream before it launches: not
 *   capturable into a hipGraph.
 * vx_tiff_unpredict: undoes the predictor of tag 317 on float32 rows of a little-endian file.  Per item, `rows` rows of W
 *   samples at src (device, 4 * rows * W bytes) go to dst (the same size); rows are independent.
 *   predictor 2  horizontal differencing on 32-bit words: within a row word[i] += word[i - 1] mod 2^32;
 *   predictor 3  floating point (libtiff's fpAcc): within a row byte[i] += byte[i - 1] mod 256 over all 4 W bytes, then
 *                sample x is put together from the row's four byte planes, the most significant bytes first (plane 0
 *                holds W most significant bytes, plane 3 the least significant).
 *   Any W >= 1 and any alignment of src and dst.  src == dst is allowed for predictor 2 only; src and dst may not overlap
 *   otherwise.  out_status[i] (device) is set to VX_LZW_OK: no input makes an item fail.  Argument errors (a null table or
 *   pointer, rows or W < 1, a predictor other than 2 / 3, a workspace below vx_tiff_unpredict_workspace_bytes(n_items)) are
 *   refused before any launch.  Uploads its table and synchronises the stream, as vx_tiff_lzw. */
enum {
  VX_LZW_OK = 0,
  VX_LZW_TRUNCATED = 1,   /* the input ends before EndOfInformation or a full window */
  VX_LZW_BAD_CODE = 2,    /* a code above the next free entry, or a first code that is not ClearCode (the LSB-first variant) */
  VX_LZW_NO_ROOM = 3      /* vx_tiff_lzw_encode: the item's window is smaller than its strip */
};
typedef struct vx_tiff_lzw_item {
  const uint8_t* src;
  int64_t src_n;
  int64_t dst_off;
  int64_t dst_cap;
} vx_tiff_lzw_item;
int64_t vx_tiff_lzw_workspace_bytes(int n_items);
int vx_tiff_lzw(const vx_tiff_lzw_item* items /* host array */, int n_items, uint8_t* dst, int64_t dst_n,
                int64_t* out_sizes /* device */, int32_t* out_status /* device */, void* workspace,
                int64_t workspace_bytes, vx_stream_t stream);
typedef struct vx_tiff_unpredict_item {
  const uint8_t* src;
  uint8_t* dst;
  int32_t rows, W;
  int32_t predictor;
  int32_t pad;
} vx_tiff_unpredict_item;
int64_t vx_tiff_unpredict_workspace_bytes(int n_items);
int vx_tiff_unpredict(const vx_tiff_unpredict_item* items /* host array */, int n_items, int32_t* out_status /* device */,
                      void* workspace, int64_t workspace_bytes, vx_stream_t stream);

/* Writing LZW-compressed float32 TIFF maps (values_amd/results2d.py: save_images_device(tiff="lzw")) -- the strips of
 * a Compression 5 file with Predictor 1, 2 or 3, byte for byte what image_io.write_tiff_f32(compression="lzw") writes.
 * All three calls upload a table and synchronise the stream before they launch, as vx_tiff_lzw: not capturable into a
 * hipGraph.  The return value is reserved for argument errors (refused before any launch) and hipError_t.
 *
 * vx_tiff_predict: the forward of vx_tiff_unpredict, with its item.  Per item, `rows` rows of W float32 samples at src
 *   (device, 4 * rows * W bytes) go to dst (the same size) as the bytes the strips hold; rows are independent.
 *   predictor 2  within a row word[i] -= word[i - 1] mod 2^32 on the little-endian 32-bit words;
 *   predictor 3  libtiff's fpDiff: the row's four byte planes, the most significant bytes first, then
 *                byte[i] -= byte[i - 1] mod 256 over all 4 W bytes.
 *   Any W >= 1 and any alignment of src and dst; src and dst may not overlap (not in place either).  out_status[i]
 *   (device) is set to VX_LZW_OK: no input makes an item fail.  Refused: a null table or pointer, rows or W < 1, a
 *   predictor other than 2 / 3, overlapping src and dst, a workspace below vx_tiff_predict_workspace_bytes(n_items).
 * vx_tiff_lzw_bound: the largest strip n >= 0 input bytes can produce: at most n data codes, one ClearCode at the start
 *   and one more per 3836 table insertions (of which there are fewer than n), one EndOfInformation, each at most 12 bits:
 *   (12 * (n + n / 3836 + 2) + 7) / 8.  -1 for n < 0.
 * vx_tiff_lzw_encode: encodes each item's bytes src[0, src_n) (device) as one LZW strip (TIFF 6.0 section 13 with
 *   libtiff's policy: ClearCode first, greedy longest match, codes MSB first, 9 to 12 bits, early change, a ClearCode
 *   when the next free entry would be 4094, EndOfInformation, the last byte zero-padded; an empty input is ClearCode +
 *   EndOfInformation, 3 bytes) into dst[dst_off, dst_off + dst_cap); the item table is vx_tiff_lzw's, read the other
 *   way round.  out_sizes[i] (device) is the strip's length and out_status[i] (device) VX_LZW_OK; a window smaller than
 *   the strip (dst_cap < vx_tiff_lzw_bound(src_n) may be one) ends the item with VX_LZW_NO_ROOM, out_sizes[i] = dst_cap
 *   and the strip's first dst_cap bytes in the window.  No read outside [src, src + src_n); no write
 *   outside the item's window and none at or beyond its out_sizes[i] bytes: the packer's last partial word is stored
 *   byte by byte.  Items are independent: an item's bytes do not depend on what else the call holds.  The windows must
 *   not overlap each other or any source.  workspace: vx_tiff_lzw_encode_workspace_bytes(n_items) bytes, 16-byte aligned.
 * vx_tiff_lzw_pack: makes the strips contiguous.  The items name the strips' windows src[dst_off, dst_off + dst_cap)
 *   in the order the blob holds them (a file's strips in row order, file after file), sizes[i] (device: the encoder's
 *   out_sizes) their lengths, read as clamped to [0, dst_cap].  out_offsets (device, n_items + 1) receives the exclusive
 *   scan of the sizes, out_offsets[n_items] the blob's size; strip i is copied to out[out_offsets[i], + sizes[i]) unless
 *   it would end beyond out_n (out_n >= the sum of the dst_cap always suffices).  src and out may not overlap.
 *   workspace: vx_tiff_lzw_pack_workspace_bytes(n_items) bytes, 16-byte aligned. */
int64_t vx_tiff_predict_workspace_bytes(int n_items);
int vx_tiff_predict(const vx_tiff_unpredict_item* items /* host array */, int n_items, int32_t* out_status /* device */,
                    void* workspace, int64_t workspace_bytes, vx_stream_t stream);
int64_t vx_tiff_lzw_bound(int64_t n);
int64_t vx_tiff_lzw_encode_workspace_bytes(int n_items);
int vx_tiff_lzw_encode(const vx_tiff_lzw_item* items /* host array */, int n_items, uint8_t* dst, int64_t dst_n,
                       int64_t* out_sizes /* device */, int32_t* out_status /* device */, void* workspace,
                       int64_t workspace_bytes, vx_stream_t stream);
int64_t vx_tiff_lzw_pack_workspace_bytes(int n_items);
int vx_tiff_lzw_pack(const vx_tiff_lzw_item* items /* host array */, int n_items, const uint8_t* src, int64_t src_n,
                     const int64_t* sizes /* device */, uint8_t* out, int64_t out_n, int64_t* out_offsets /* device */,
                     void* workspace, int64_t workspace_bytes, vx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VALUES_AMD_H */
