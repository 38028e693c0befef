// Whole-network launch: UNet3D.forward (uncertainty_modeling/models/unet3D_module.py:296-373) for a batch
// of N samples (MC-dropout samples x TTA views x volumes), as ~45 kernel launches on the caller's
// stream -- no allocation, no synchronisation, capturable into one hipGraph.
//
// Data flow (channels-last fp32, level l has spatial (D,H,W) >> l and C_l = F << l channels):
//   encoder l:  conv -> A_l (raw + stats) -> finalize -> IN/LReLU/drop in place
//               conv -> B_l (raw + stats) -> finalize -> IN/LReLU/drop -> skip half of CAT_l + pool -> P_{l+1}
//   center:     conv+ReLU, conv+ReLU, convT+ReLU+drop -> up half of CAT_3
//   decoder l:  conv(CAT_l)+LReLU+drop -> A_l, conv+LReLU+drop -> B_l, convT -> up half of CAT_{l-1}
//   final:      1x1x1 conv(B_0) -> logits NCDHW, slot dst[n], un-flipped
// torch.cat never happens (K7): CAT_l is the x-blocked buffer [N][D][H][W/xb][2][xb][C_l] (values_amd.h) whose two
// halves are written as dense blocks by their producers and read by the decoder conv through in_xblk.
// First layer in MC-dropout mode: computed once per volume (the T samples share input and statistics).
#include "conv3d_internal.h"

namespace {
struct Level { int D, H, W, C; int64_t nvox; };

struct Plan {
  Level lv[5];
  float *A[4], *B[4], *CAT[4], *P[5], *C0, *C1;
  float *stats, *mean, *rstd;
  float *mean0, *rstd0;   // level-0 skip statistics: kept until the decoder normalises the skip half itself
  float *meanS[4], *rstdS[4];   // (round 5) the same for the levels whose second contract conv leaves its RAW output in the skip half
  size_t bytes;
};

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

static void make_plan(Plan& p, int N, int D, int H, int W, int F, char* base) {
  size_t off = 0;
  auto carve = [&](size_t floats) {
    float* q = base ? (float*)(base + off) : nullptr;
    off += align_up(floats * sizeof(float));
    return q;
  };
  for (int l = 0; l < 5; ++l) {
    p.lv[l].D = D >> l; p.lv[l].H = H >> l; p.lv[l].W = W >> l; p.lv[l].C = F << l;
    p.lv[l].nvox = (int64_t)p.lv[l].D * p.lv[l].H * p.lv[l].W;
  }
  for (int l = 0; l < 4; ++l) {
    const size_t e = (size_t)N * p.lv[l].nvox * p.lv[l].C;
    p.A[l] = carve(e);
    p.B[l] = carve(e);
    p.CAT[l] = carve(2 * e);
  }
  p.P[0] = nullptr;
  for (int l = 1; l < 5; ++l) p.P[l] = carve((size_t)N * p.lv[l].nvox * p.lv[l - 1].C);
  p.C0 = carve((size_t)N * p.lv[4].nvox * p.lv[4].C);
  p.C1 = carve((size_t)N * p.lv[4].nvox * p.lv[4].C);
  // statistics: the largest partial buffer is level 0
  size_t smax = 0;
  for (int l = 0; l < 4; ++l) {
    size_t t = (size_t)vx_conv3d_k3_tiles(p.lv[l].D, p.lv[l].H, p.lv[l].W);
    if (l == 0) {
      size_t t1 = (size_t)vx_conv3d_k3_c1_tiles(p.lv[0].D, p.lv[0].H, p.lv[0].W);
      if (t1 > t) t = t1;
    }
    const size_t e = (size_t)N * t * p.lv[l].C * 2;
    if (e > smax) smax = e;
  }
  p.stats = carve(smax);
  p.mean = carve((size_t)N * p.lv[3].C);
  p.rstd = carve((size_t)N * p.lv[3].C);
  p.mean0 = carve((size_t)N * p.lv[0].C);
  p.rstd0 = carve((size_t)N * p.lv[0].C);
  for (int l = 0; l < 4; ++l) {
    p.meanS[l] = l == 0 ? p.mean0 : carve((size_t)N * p.lv[l].C);
    p.rstdS[l] = l == 0 ? p.rstd0 : carve((size_t)N * p.lv[l].C);
  }
  p.bytes = off;
}
}  // namespace

extern "C" size_t vx_unet3d_workspace_bytes(int N, int D, int H, int W, int F) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || F <= 0) return 0;
  Plan p;
  make_plan(p, N, D, H, W, F, nullptr);
  return p.bytes;
}

// Optional per-launch timing (vx_unet3d_forward_profiled): a HIP event pair around every launch, on the
// caller's stream.  Off (g_prof == nullptr) in normal and captured runs.
namespace {
struct Prof {
  static constexpr int MAXL = 96;
  hipEvent_t ev[2 * MAXL];
  const char* name[MAXL];
  const char* kernel[MAXL];
  int n = 0;
  hipStream_t s;
};
thread_local Prof* g_prof = nullptr;
thread_local char g_prof_labels[Prof::MAXL][192];   // "label|kernel instance", valid until the thread's next profiled forward
}  // namespace

#define VX_TRY(expr)            \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != VX_OK) return rc_; \
  } while (0)

#define VX_STEP(label, expr)                                                       \
  do {                                                                             \
    Prof* pf_ = g_prof;                                                            \
    if (pf_ && pf_->n < Prof::MAXL) { vx_note_kernel(nullptr); (void)hipEventRecord(pf_->ev[2 * pf_->n], pf_->s); }  \
    int rc_ = (expr);                                                              \
    if (rc_ != VX_OK) return rc_;                                                  \
    if (pf_ && pf_->n < Prof::MAXL) {                                              \
      (void)hipEventRecord(pf_->ev[2 * pf_->n + 1], pf_->s);                             \
      pf_->kernel[pf_->n] = vx_last_kernel();                                      \
      pf_->name[pf_->n++] = (label);                                               \
    }                                                                              \
  } while (0)

namespace {
int xblk_of(int W) { return W % 4 == 0 ? 4 : (W % 2 == 0 ? 2 : 1); }

// Every data-flow decision of one forward, taken by decide_flow before the first launch; the launch code only reads it.
struct Flow {
  bool inorm;          // do_instancenorm (unet3D_module.py:231-243)
  int ich;             // input channels (1: the first conv on its own VALU kernel)
  int rep;             // MC-dropout samples per volume
  bool shared;         // the first conv (+ statistics) once per volume, its samples fanned out by the consumer
  bool fuse_head;      // the final 1x1x1 conv in expand_1_2's epilogue, B_0 never stored
  bool pre[4];         // contr_l_2 normalises its raw input on load (no separate pass over A_l)
  bool presplit;       // ... and at level 0 reads the once-per-volume output of vx_prenorm_split
  bool skip_raw[4];    // the skip half of CAT_l holds contr_l_2's RAW output; expand_l_1 normalises it on load
  bool pooled[4];      // contr_l_2's epilogue leaves its block's MaxPool window maxima + any-dropped flags in B_l
  bool poolfin1;       // contr_2_1 finishes level 0's window maxima on load (vx_conv3d_args.in_pool_flags)
  bool halves[4];      // expand_l_1 as two launches over the two DENSE halves of CAT_l (vx_conv3d_args.acc_in)
  bool fuse_up;        // upscale2 inside expand_1_1 (B_1 in, the up half of CAT_0 never exists)
  bool fuse_up1;       // upscale3 inside expand_2_1's up-half launch (B_2 in)
  bool split_out[4];   // expand_l_2 hands B_l to such a fused up-convolution as fp16 (hi, lo) pairs
  bool planar1;        // expand_2_1 -> expand_2_2 as the planar pre-split tensor, staged by LDS-DMA
  bool st16;           // storage16: expand_1_1 -> expand_1_2 as fp16
  int products_c12, products_e11, products_e12;   // vx_conv3d_args.products of contr_1_2, expand_1_1, expand_1_2
};

Flow decide_flow(const vx_unet3d_weights* w, const vx_unet3d_run* r, const Plan& p) {
  const vx_config& cfg = vx_cfg();
  const int F = w->F, dm = r->drop_mode;
  const Level* lv = p.lv;
  // every fusion needs the hash generator or no dropout: injected masks take the general kernels with their separate passes
  const bool hashed = dm != VX_DROP_MASK;
  Flow f = {};
  f.inorm = !w->no_instancenorm;
  f.ich = w->in_channels > 1 ? w->in_channels : 1;
  f.rep = r->repeat > 0 ? r->repeat : 1;
  // MC-dropout: the T samples of a volume share the first conv and its statistics -> once per volume into a scratch;
  // contr_1_2 reads that scratch with T dropout patterns, or (general kernels) the norm kernel fans it out
  f.shared = !r->src && !r->flip && f.rep > 1 && r->N % f.rep == 0;
  // head fusion: where the last 3x3x3 conv runs on the kernel that holds a voxel's channels in one lane
  f.fuse_head = w->num_classes <= 4 && vx_conv3d_k3_head_fusable(F, F) && !cfg.no_head_fusion;
  // level 0 on the z-column kernel: contr_1_2 and expand_1_1 normalise their inputs themselves (no normalised
  // full-resolution tensor is ever written)
  f.pre[0] = hashed && !cfg.s16_no_prenorm && F == 8 && f.inorm && vx_conv3d_k3_prologue_ok(lv[0].D, lv[0].H, lv[0].W, F, F);
  for (int l = 1; l < 4; ++l)
    f.pre[l] = f.inorm && hashed && !cfg.s16_no_prenorm && vx_conv3d_k3_prologue_ok(lv[l].D, lv[l].H, lv[l].W, lv[l].C, lv[l].C);
  // InstanceNorm + LeakyReLU + the fp16 split of the shared tensor ONCE per volume (in place); contr_1_2's staging waves then
  // only AND sample n's dropout bits in -- a third of their vector work (they are that layer's critical path: tools/stamp_s16.py)
  // (only where contr_1_2 runs on the z-column kernel: the tile kernel's prologue reads the RAW tensor through in_repeat --
  // s16_no_xp = 1 with n_pred > 1 failed with VX_E_SHAPE after the scratch had been rewritten)
  f.presplit = f.shared && f.pre[0] && vx_conv3d_k3_presplit_ok(lv[0].D, lv[0].H, lv[0].W, F, F);
  // contr_1_2's raw output straight into the skip half + a pooling-only pass + expand_1_1 normalising its skip half
  // (vx_config.s16_skip_raw, default 1): the pass shrinks 1.10 -> 0.58 ms per 320 samples, expand_1_1 grows 2.38 -> 2.69
  // now that its staging runs in producer waves (on the kernel where every wave staged AND multiplied it grew 2.33 -> 2.95
  // and the fusion was neutral).  The full-resolution tensor is written once and read twice instead of written twice and
  // read twice; the statistics wait in mean0 / rstd0 for expand_1_1.
  f.skip_raw[0] = f.pre[0] && cfg.s16_skip_raw && vx_conv3d_k3_prologue_ok(lv[0].D, lv[0].H, lv[0].W, 2 * F, F);
  // MaxPool of the first block out of contr_1_2's epilogue (window maxima of the kept raw values + any-dropped bits, then
  // vx_pool_finish on 1/8 of the voxels) instead of a pass that re-reads the full-resolution tensor
  f.pooled[0] = f.skip_raw[0] && vx_conv3d_k3_poolfuse_ok(lv[0].D, lv[0].H, lv[0].W, F, F);
  // Round 4: contr_2_1 finishes the window maxima itself while it stages its tiles: the pass over the pooled tensor, its
  // launch and the tensor are gone
  f.poolfin1 = f.pooled[0] && vx_conv3d_k3_poolfin_ok(F, 2 * F);
  // Round 5 (levels below full resolution on the 16-channel z-column kernel, conv3d_zc16.hip): the level-0 data flow -- the
  // second conv writes its RAW output straight into the skip half, leaves the (y, x) half of the block's MaxPool next to it,
  // vx_pool_finish_z produces P_{l+1} from a quarter of the voxels once the statistics exist, and the decoder's first conv of
  // the level normalises the skip half on load.  The normalise + pool pass over the whole tensor (0.25 ms per 320 samples at
  // level 1) is gone.
  for (int l = 1; l < 4; ++l) {
    const Level& L = lv[l];
    f.skip_raw[l] = f.pooled[l] = f.inorm && hashed && !cfg.s16_no_prenorm && cfg.s16_skip_raw &&
                                  vx_conv3d_k3_pool_layout(L.D, L.H, L.W, L.C, L.C) == 2 &&
                                  vx_conv3d_k3_skip_prologue_ok(L.D, L.H, L.W, 2 * L.C, L.C, xblk_of(L.W));
  }
  // level 1 of the F = 8 networks: CAT_1 is used as TWO DENSE tensors (up = first half of the buffer, skip = second)
  f.halves[1] = f.skip_raw[1] && lv[1].C == 16 && w->split_w[0] && w->split_w[1] && !cfg.s16_no_halves &&
                w->split_family == vx_conv3d_k3_family(16, 16) && vx_conv3d_k3_acc_ok(lv[1].D, lv[1].H, lv[1].W, 16, 16);
  // upscale2 inside expand_1_1: the up half of CAT_0 is computed from B_1 while expand_1_1 stages its tiles and never exists
  // in memory (conv3d_xp8w.hip: UP = 2 with the composed weights w->up_fused, 1 without)
  f.fuse_up = hashed && F == 8 && vx_conv3d_k3_upfuse_ok(lv[0].D, lv[0].H, lv[0].W, 2 * F, F);
  // upscale3 evaluated by the staging waves of expand_2_1's up-half launch from B_2 (round 5)
  f.fuse_up1 = f.halves[1] && w->up3_zc16 && hashed && vx_conv3d_k3_upfuse_ok(lv[1].D, lv[1].H, lv[1].W, 16, 16) == 2;
  // the coarse tensor of a fused up-convolution has ONE reader: its producer hands it over pre-split
  f.split_out[1] = f.fuse_up;
  f.split_out[2] = f.fuse_up1;
  // Round 6: expand_2_2 has no normalisation in front of it (unet3D_module.py:263-267), so expand_2_1's up-half launch hands
  // the tensor over as the fp16 (hi, lo) planes expand_2_2's matrix instructions take, in its LDS row order
  f.planar1 = f.fuse_up1 && !cfg.s16_no_l1dma && vx_conv3d_k3_planar_ok(lv[1].D, lv[1].H, lv[1].W, 16, 16);
  // opt-in reduced-storage mode (vx_config.storage16, never the default): expand_1_1 -> expand_1_2 hand their tensor over as
  // fp16; needs the z-column kernels on both and the fused head
  f.st16 = cfg.storage16 && dm == VX_DROP_HASH && F == 8 && f.fuse_head && cfg.conv_fp32 == 0 &&
           vx_conv3d_k3_prologue_ok(lv[0].D, lv[0].H, lv[0].W, F, F);
  // storage16 = 2: one fp16 product per fp32 product on the three full-resolution launches, each in its fused form
  const bool one = f.st16 && cfg.storage16 == 2;
  f.products_c12 = one && f.presplit && f.pooled[0];
  f.products_e11 = one && f.skip_raw[0] && f.fuse_up && w->up_fused;
  f.products_e12 = one;
  return f;
}
}  // namespace

extern "C" int vx_unet3d_forward(const vx_unet3d_weights* w, const vx_unet3d_run* r, vx_stream_t stream) {
  if (!w || !r) VX_FAIL(VX_E_NULL, "vx_unet3d_forward: null argument");
  if (!r->x || !r->logits || !r->workspace) VX_FAIL(VX_E_NULL, "vx_unet3d_forward: null tensor/workspace");
  const int N = r->N, D = r->D, H = r->H, W = r->W, F = w->F, NC = w->num_classes;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) VX_FAIL(VX_E_SHAPE, "vx_unet3d_forward: empty batch");
  if (D % 16 || H % 16 || W % 16)
    VX_FAIL(VX_E_SHAPE, "vx_unet3d_forward: spatial size (%d,%d,%d) must be divisible by 16 (4 poolings; InstanceNorm "
            "needs > 1 voxel at the 8x level)", D, H, W);
  if (F != 8 && F != 16 && F != 32) VX_FAIL(VX_E_SHAPE, "vx_unet3d_forward: initial_filter_size %d unsupported (8,16,32)", F);
  if (NC <= 0) VX_FAIL(VX_E_SHAPE, "vx_unet3d_forward: num_classes %d", NC);
  if (r->drop_mode < 0 || r->drop_mode > 2) VX_FAIL(VX_E_DTYPE, "vx_unet3d_forward: drop_mode %d", r->drop_mode);
  if ((((uintptr_t)r->workspace) & 255u) != 0) VX_FAIL(VX_E_ALIGN, "vx_unet3d_forward: workspace must be 256-byte aligned");
  for (int i = 0; i < 18; ++i)
    if (!w->conv_w[i] || !w->conv_b[i]) VX_FAIL(VX_E_NULL, "vx_unet3d_forward: conv weight %d missing", i);
  if (w->in_channels < 0 || w->in_channels > 8) VX_FAIL(VX_E_SHAPE, "vx_unet3d_forward: in_channels %d (1 .. 8)", w->in_channels);
  for (int i = 0; i < 4; ++i)
    if (!w->up_w[i] || !w->up_b[i]) VX_FAIL(VX_E_NULL, "vx_unet3d_forward: transposed-conv weight %d missing", i);
  if (!w->final_w || !w->final_b) VX_FAIL(VX_E_NULL, "vx_unet3d_forward: final weights missing");
  if (r->drop_mode == VX_DROP_MASK)
    for (int i = 0; i < 17; ++i)
      if (!r->masks[i]) VX_FAIL(VX_E_NULL, "vx_unet3d_forward: mask %d missing", i);

  Plan p;
  make_plan(p, N, D, H, W, F, (char*)r->workspace);
  if (p.bytes > r->workspace_bytes)
    VX_FAIL(VX_E_WORKSPACE, "vx_unet3d_forward: workspace %zu B < required %zu B", r->workspace_bytes, p.bytes);
  const Flow f = decide_flow(w, r, p);

  const int dm = r->drop_mode;
  auto mask = [&](int i) { return dm == VX_DROP_MASK ? r->masks[i] : (const uint8_t*)nullptr; };
  // the arguments every 3x3x3 launch shares: layer wi's weights, level L's shape, the batch, the seed; the fp16 range guard
  // watches the outputs without statistics (decoder / center outputs feed split-fp16 consumers un-normalised)
  auto conv_args = [&](int wi, const Level& L, int Cin, int Cout, float* stats) {
    vx_conv3d_args a = {};
    a.w_packed = w->conv_w[wi]; a.bias = w->conv_b[wi]; a.w_family = w->conv_family[wi];
    a.N = N; a.D = L.D; a.H = L.H; a.W = L.W; a.Cin = Cin; a.Cout = Cout;
    a.drop_seed = r->seed; a.seed_dev = r->seed_dev;
    a.stats_partial = stats; a.range_flag = stats ? nullptr : r->range_flag;
    a.out_half = 1;
    return a;
  };
  // epilogue: activation, then dropout layer `layer`
  auto set_drop = [&](vx_conv3d_args& a, int act, int layer) {
    a.act = act; a.drop_mode = dm; a.drop_layer = (uint32_t)layer; a.drop_mask = mask(layer);
  };
  // prologue: the input is a contract block's RAW conv output; its InstanceNorm (mean / rstd), LeakyReLU and dropout layer
  // `layer` are applied while the conv stages its tiles (rep samples share one input sample and statistics row)
  auto set_pre = [&](vx_conv3d_args& a, int layer, int rep, const float* mean, const float* rstd) {
    a.in_mean = mean; a.in_rstd = rstd; a.in_repeat = rep;
    a.in_drop_mode = dm; a.in_drop_seed = r->seed; a.in_drop_layer = (uint32_t)layer;
  };
  // a streaming InstanceNorm (p.mean / p.rstd unless `normalise` is false) + LeakyReLU + dropout pass over x (C channels)
  auto norm_args = [&](const float* x, int C, const Level& L, int drop_layer, bool normalise) {
    vx_norm_args a = {};
    a.x = x; a.x_pitch = C; a.x_half = 1; a.out_half = 1; a.pool_pitch = C;
    a.mean = normalise ? p.mean : nullptr; a.rstd = normalise ? p.rstd : nullptr;
    a.range_flag = normalise ? nullptr : r->range_flag;   // an un-normalised tensor on its way to a split-fp16 conv
    a.N = N; a.D = L.D; a.H = L.H; a.W = L.W; a.C = C;
    a.act = VX_ACT_LRELU;
    a.drop_mode = drop_layer >= 0 ? dm : VX_DROP_NONE; a.drop_seed = r->seed; a.drop_layer = (uint32_t)(drop_layer >= 0 ? drop_layer : 0);
    a.drop_mask = drop_layer >= 0 ? mask(drop_layer) : nullptr;
    a.seed_dev = r->seed_dev;
    return a;
  };
  auto convT = [&](const float* in, int ui, float* out, int out_pitch, const Level& Lin, int Cin, int Cout, int act,
                   int drop_layer, bool dense) {
    vx_convT_args a = {};
    a.range_flag = r->range_flag;
    a.seed_dev = r->seed_dev;
    a.out_xblk = dense ? 0 : xblk_of(2 * Lin.W); a.out_half = 0;
    a.in = in; a.in_pitch = Cin; a.w_packed = w->up_w[ui]; a.bias = w->up_b[ui];
    a.out = out; a.out_pitch = out_pitch; a.out_coff = 0;
    a.N = N; a.D = Lin.D; a.H = Lin.H; a.W = Lin.W; a.Cin = Cin; a.Cout = Cout;
    a.act = act;
    a.drop_mode = drop_layer >= 0 ? dm : VX_DROP_NONE;
    a.drop_seed = r->seed; a.drop_layer = (uint32_t)(drop_layer >= 0 ? drop_layer : 0);
    a.drop_mask = drop_layer >= 0 ? mask(drop_layer) : nullptr;
    return vx_convT_k2s2(&a, stream);
  };
  // B_l is free until the decoder: a pooled epilogue leaves its window maxima there and the flag words behind them --
  // level 0 [N][nvox / 8][8] + [..][2], below [N][D][H/2][W/2][C] + [..][C/4]
  auto pool_flags = [&](int l) {
    const size_t maxima = l == 0 ? (size_t)N * p.lv[1].nvox * 8 : (size_t)N * (p.lv[l].nvox / 4) * p.lv[l].C;
    return reinterpret_cast<uint32_t*>(p.B[l] + maxima);
  };
  // the first conv over n_out samples (raw output + bias; statistics if asked): Cin == 1 on its own VALU kernel, more
  // input channels zero-padded to 8 on the general kernels (input laid out channels-last in B_0, free until contr_1_2)
  auto first_conv = [&](float* out, int n_out, int rep, float* stats) -> int {
    const Level& L = p.lv[0];
    if (f.ich == 1)
      return vx_conv3d_k3_c1(r->x, w->conv_w[0], w->conv_b[0], out, L.C, n_out, L.D, L.H, L.W, L.C, rep, r->src, r->flip, stats, stream);
    VX_TRY(vx_pack_input_cl8(r->x, p.B[0], n_out, f.ich, L.D, L.H, L.W, rep, r->src, r->flip, stream));
    vx_conv3d_args a = conv_args(0, L, 8, L.C, stats);
    a.N = n_out; a.in = p.B[0]; a.in_pitch = 8; a.out = out; a.out_pitch = L.C;
    return vx_conv3d_k3(&a, stream);
  };

  static const char* kConv[18] = {"contr_1_1", "contr_1_2", "contr_2_1", "contr_2_2", "contr_3_1", "contr_3_2",
                                  "contr_4_1", "contr_4_2", "center.0", "center.2", "expand_4_1", "expand_4_2",
                                  "expand_3_1", "expand_3_2", "expand_2_1", "expand_2_2", "expand_1_1", "expand_1_2"};
  static const char* kNorm[8] = {"norm:contr_1_1", "norm:contr_1_2", "norm:contr_2_1", "norm:contr_2_2",
                                 "norm:contr_3_1", "norm:contr_3_2", "norm:contr_4_1", "norm:contr_4_2"};
  static const char* kFin[8] = {"finalize:contr_1_1", "finalize:contr_1_2", "finalize:contr_2_1", "finalize:contr_2_2",
                                "finalize:contr_3_1", "finalize:contr_3_2", "finalize:contr_4_1", "finalize:contr_4_2"};
  static const char* kPoolFin[4] = {"poolfin:contr_1_2", "poolfin:contr_2_2", "poolfin:contr_3_2", "poolfin:contr_4_2"};
  static const char* kUp[4] = {"center.4", "upscale4", "upscale3", "upscale2"};
  // the first conv's output: with f.shared a once-per-volume scratch that `fan` samples read -- A_0 when CAT_0 takes contr_1_2's
  // raw output; else CAT_0, free until contr_1_2's norm
  float* const out1 = f.shared && !f.skip_raw[0] ? p.CAT[0] : p.A[0];
  const int fan = f.shared ? f.rep : 1;
  // ---------------- encoder ----------------
  for (int l = 0; l < 4; ++l) {
    const Level& L = p.lv[l];
    const int C = L.C;
    const int ntiles = vx_conv3d_k3_tiles_for(L.D, L.H, L.W, C);
    if (l == 0) {
      const int n1 = N / fan;
      const int ntiles1 = f.ich == 1 ? vx_conv3d_k3_c1_tiles(L.D, L.H, L.W) : ntiles;
      VX_STEP(kConv[0], first_conv(out1, n1, f.shared ? 1 : f.rep, f.inorm ? p.stats : nullptr));
      // (vx_prenorm_split_stats -- the pre-split pass reducing the 256 partial tiles of a 64^3 volume itself -- measured 0.095 ms
      // against 0.079 + 0.007 for the finalize launch and the plain pass: the launch stays here)
      if (f.inorm) VX_STEP(kFin[0], vx_instnorm_finalize(p.stats, n1, ntiles1, C, L.nvox, 1e-5f, p.mean, p.rstd, stream));
      if (f.presplit)
        VX_STEP("presplit:contr_1_1", vx_prenorm_split(out1, p.mean, p.rstd, n1, L.nvox, dm == VX_DROP_HASH ? 2.f : 1.f, stream));
      if (!f.pre[0]) {
        vx_norm_args n = norm_args(out1, C, L, 0, f.inorm);
        n.out = p.A[0]; n.out_pitch = C;
        VX_STEP(kNorm[0], vx_norm_act_drop_pool_bcast(&n, fan, stream));
      }
    } else {
      vx_conv3d_args a = conv_args(2 * l, L, C / 2, C, f.inorm ? p.stats : nullptr);
      a.in = p.P[l]; a.in_pitch = C / 2; a.out = p.A[l]; a.out_pitch = C;
      // do_instancenorm=False (unet3D_module.py:238-243): conv + LeakyReLU + Dropout, all in the conv's epilogue
      if (!f.inorm) set_drop(a, VX_ACT_LRELU, 2 * l);
      if (l == 1 && f.poolfin1) {
        a.in = p.B[0]; a.in_pool_flags = pool_flags(0);
        set_pre(a, 1, 1, p.mean0, p.rstd0);
      }
      VX_STEP(l == 1 && f.poolfin1 ? "poolfin+contr_2_1" : kConv[2 * l], vx_conv3d_k3(&a, stream));
      if (f.inorm) {
        VX_STEP(kFin[2 * l], vx_instnorm_finalize(p.stats, N, ntiles, C, L.nvox, 1e-5f, p.mean, p.rstd, stream));
        if (!f.pre[l]) {
          vx_norm_args n = norm_args(p.A[l], C, L, 2 * l, true);
          n.out = p.A[l]; n.out_pitch = C;
          VX_STEP(kNorm[2 * l], vx_norm_act_drop_pool_bcast(&n, 1, stream));
        }
      }
    }
    if (!f.inorm) {
      // second conv of the block with its activation / dropout fused; one streaming pass copies it into the skip half of
      // the concat buffer and pools it (no normalisation, no activation)
      vx_conv3d_args a = conv_args(2 * l + 1, L, C, C, nullptr);
      a.in = p.A[l]; a.in_pitch = C; a.out = p.B[l]; a.out_pitch = C;
      set_drop(a, VX_ACT_LRELU, 2 * l + 1);
      VX_STEP(kConv[2 * l + 1], vx_conv3d_k3(&a, stream));
      vx_norm_args n = norm_args(p.B[l], C, L, -1, false);
      n.act = VX_ACT_NONE;
      n.out = p.CAT[l]; n.out_pitch = 2 * C; n.out_coff = C; n.out_xblk = xblk_of(L.W); n.pool_out = p.P[l + 1];
      VX_STEP(kNorm[2 * l + 1], vx_norm_act_drop_pool_bcast(&n, 1, stream));
      continue;
    }
    vx_conv3d_args a = conv_args(2 * l + 1, L, C, C, p.stats);
    a.in = p.A[l]; a.in_pitch = C; a.out = p.B[l]; a.out_pitch = C;
    if (f.pre[l]) {   // the raw A_l -- at level 0 the first conv's output as it stands
      if (l == 0) a.in = out1;
      set_pre(a, 2 * l, l == 0 ? fan : 1, p.mean, p.rstd);
    }
    a.in_split = l == 0 && f.presplit;
    if (l == 0) a.products = f.products_c12;
    if (f.skip_raw[l]) {
      if (f.halves[l]) a.out = p.CAT[l] + (size_t)N * L.nvox * C;   // the dense skip half
      else { a.out = p.CAT[l]; a.out_xblk = xblk_of(L.W); }
    }
    if (f.pooled[l]) {   // the window maxima are over the raw values the block's dropout keeps
      a.pool_out = p.B[l]; a.pool_flags = pool_flags(l);
      set_drop(a, VX_ACT_NONE, 2 * l + 1);
    }
    VX_STEP(kConv[2 * l + 1], vx_conv3d_k3(&a, stream));
    if (l == 0 && f.skip_raw[0]) {
      VX_STEP(kFin[1], vx_instnorm_finalize(p.stats, N, ntiles, C, L.nvox, 1e-5f, p.mean0, p.rstd0, stream));
      if (!f.pooled[0]) {
        vx_norm_args n = norm_args(p.CAT[0], C, L, 1, true);
        n.mean = p.mean0; n.rstd = p.rstd0; n.x_xblk = xblk_of(L.W); n.pool_out = p.P[1];
        VX_STEP("pool:contr_1_2", vx_norm_act_drop_pool_bcast(&n, 1, stream));
      } else if (!f.poolfin1) {
        VX_STEP(kPoolFin[0], vx_pool_finish(p.B[0], pool_flags(0), p.mean0, p.rstd0, p.P[1], C, N, p.lv[1].nvox, dm == VX_DROP_HASH, stream));
      }
    } else if (f.skip_raw[l]) {   // (round 5: the pass reduces the partials itself and leaves meanS / rstdS for the decoder's prologue)
      const vx_stat_src st = {p.stats, ntiles, 1e-5f, (int64_t)L.nvox, p.meanS[l], p.rstdS[l]};
      VX_STEP(kPoolFin[l], vx_pool_finish_z_stats(p.B[l], pool_flags(l), &st, p.P[l + 1], C, N, L.D / 2, (int64_t)(L.H / 2) * (L.W / 2),
                                                  dm == VX_DROP_HASH, stream));
    } else {   // the normalise + pool pass writes the skip half of CAT_l and P_{l+1}
      vx_norm_args n = norm_args(p.B[l], C, L, 2 * l + 1, true);
      n.out = p.CAT[l]; n.out_pitch = 2 * C; n.out_coff = C; n.out_xblk = xblk_of(L.W); n.pool_out = p.P[l + 1];
      if (C <= 512) {   // (round 5: the pass reduces the partials itself; no finalize launch)
        n.mean = nullptr; n.rstd = nullptr;
        const vx_stat_src st = {p.stats, ntiles, 1e-5f, (int64_t)L.nvox, p.mean, p.rstd};
        VX_STEP(kNorm[2 * l + 1], vx_norm_act_drop_pool_stats(&n, &st, stream));
      } else {
        VX_STEP(kFin[2 * l + 1], vx_instnorm_finalize(p.stats, N, ntiles, C, L.nvox, 1e-5f, p.mean, p.rstd, stream));
        VX_STEP(kNorm[2 * l + 1], vx_norm_act_drop_pool_bcast(&n, 1, stream));
      }
    }
  }
  // ---------------- center ----------------
  {
    const Level& L4 = p.lv[4];
    const int C3 = p.lv[3].C, C4 = L4.C;
    vx_conv3d_args a = conv_args(8, L4, C3, C4, nullptr);
    a.in = p.P[4]; a.in_pitch = C3; a.out = p.C0; a.out_pitch = C4; a.act = VX_ACT_RELU;
    VX_STEP(kConv[8], vx_conv3d_k3(&a, stream));
    vx_conv3d_args b = conv_args(9, L4, C4, C4, nullptr);
    b.in = p.C0; b.in_pitch = C4; b.out = p.C1; b.out_pitch = C4; b.act = VX_ACT_RELU;
    VX_STEP(kConv[9], vx_conv3d_k3(&b, stream));
    VX_STEP(kUp[0], convT(p.C1, 0, p.CAT[3], 2 * C3, L4, C4, C3, VX_ACT_RELU, 8, false));
  }
  // ---------------- decoder ----------------
  for (int l = 3; l >= 0; --l) {
    const Level& L = p.lv[l];
    const int C = L.C;
    const int wi = 10 + 2 * (3 - l);   // expand_{l+1}_1 / _2 are layers wi / wi + 1 with dropout layers dl / dl + 1
    const int dl = 9 + 2 * (3 - l);
    if (f.halves[l]) {
      // conv(cat([up, skip])) = conv_up(up) + conv_skip(skip) + bias, as two launches of the 16-channel z-column kernel over the two
      // DENSE halves: (1) the skip half, normalised on load (InstanceNorm + LeakyReLU + dropout layer 2 l + 1), + bias -> partial
      // sums in A_l; (2) the up half + the partial sums -> LeakyReLU -> dropout -> A_l in place.  The tile kernel's launch over the
      // x-blocked buffer paid 0.17 ms for the prologue in waves that also multiply (1.02 ms; the two launches: see DESIGN 5e).
      vx_conv3d_args a = conv_args(wi, L, C, C, nullptr);
      a.w_packed = w->split_w[1]; a.w_family = w->split_family;
      a.in = p.CAT[l] + (size_t)N * L.nvox * C; a.in_pitch = C; a.out = p.A[l]; a.out_pitch = C;
      set_pre(a, 2 * l + 1, 1, p.meanS[l], p.rstdS[l]);
      a.range_flag = nullptr;   // partial sums: the second launch's output is what a split-fp16 conv reads
      VX_STEP("expand_2_1(skip half)", vx_conv3d_k3(&a, stream));
      vx_conv3d_args b = conv_args(wi, L, C, C, nullptr);
      b.w_packed = w->split_w[0]; b.w_family = w->split_family;
      b.in = p.CAT[l]; b.in_pitch = C; b.out = p.A[l]; b.out_pitch = C; b.acc_in = p.A[l]; b.acc_pitch = C;
      set_drop(b, VX_ACT_LRELU, dl);
      if (f.fuse_up1) {
        b.in = p.B[l + 1]; b.up_in = p.B[l + 1]; b.up_pitch = 2 * C; b.up_w = w->up3_zc16; b.up_b = w->up_b[2];
        b.up_split = 1;
        b.up_fused = w->up3_fused;   // (nullable) upscale3 composed into the up half's weights: same instance, composed bodies
      }
      // the planar tensor goes into the up half of CAT_l, free since upscale3 lives inside this launch (it cannot overwrite A_l
      // in place: the partial sums there have the float layout)
      if (f.planar1) { b.out = p.CAT[l]; b.out_planar = 1; }
      VX_STEP(f.fuse_up1 ? "upscale3+expand_2_1(up half)" : "expand_2_1(up half)", vx_conv3d_k3(&b, stream));
    } else {
      vx_conv3d_args a = conv_args(wi, L, 2 * C, C, nullptr);
      a.in = p.CAT[l]; a.in_pitch = 2 * C; a.in_xblk = xblk_of(L.W); a.out = p.A[l]; a.out_pitch = C;
      set_drop(a, VX_ACT_LRELU, dl);
      if (f.skip_raw[l]) set_pre(a, 2 * l + 1, 1, p.meanS[l], p.rstdS[l]);
      if (l == 0 && f.fuse_up) {
        a.up_in = p.B[1]; a.up_w = w->up_w[3]; a.up_b = w->up_b[3]; a.up_pitch = 2 * C;
        a.up_fused = w->up_fused;   // (nullable) the up-convolution composed into expand_1_1's weights
        a.up_split = 1;
      }
      if (l == 0) { a.out_f16 = f.st16; a.products = f.products_e11; }
      VX_STEP(l == 0 && f.fuse_up ? "upscale2+expand_1_1" : kConv[wi], vx_conv3d_k3(&a, stream));
    }
    vx_conv3d_args a = conv_args(wi + 1, L, C, C, nullptr);
    a.in = p.A[l]; a.in_pitch = C; a.out = p.B[l]; a.out_pitch = C;
    set_drop(a, VX_ACT_LRELU, dl + 1);
    if (l == 1 && f.planar1) { a.in = p.CAT[l]; a.in_planar = 1; }
    a.out_split = f.split_out[l];
    if (l == 0) { a.in_f16 = f.st16; a.products = f.products_e12; }
    if (l == 0 && f.fuse_head) {
      a.out = nullptr;
      a.head_out = r->logits; a.head_w = w->final_w; a.head_b = w->final_b; a.head_C = NC; a.head_dst = r->dst; a.head_flip = r->flip;
    }
    // a fused launch is labelled with every layer it computes
    VX_STEP(l == 0 && f.fuse_head ? "expand_1_2+final" : kConv[wi + 1], vx_conv3d_k3(&a, stream));
    if (l > 0 && !(l == 1 && f.fuse_up) && !(l == 2 && f.fuse_up1))
      VX_STEP(kUp[4 - l], convT(p.B[l], 4 - l, p.CAT[l - 1], f.halves[l - 1] ? C / 2 : C, L, C, C / 2, VX_ACT_NONE, -1, f.halves[l - 1]));
  }
  // ---------------- head ----------------
  if (!f.fuse_head)
    VX_STEP("final", vx_conv1x1_ncdhw(p.B[0], F, w->final_w, w->final_b, r->logits, N, D, H, W, F, NC, r->dst, r->flip, stream));
  return VX_OK;
}

// Diagnostic entry for bench.py's roofline leg: runs the forward eagerly with a HIP event pair around every
// launch on `stream`, synchronises the stream, and returns per-launch milliseconds and labels.
extern "C" int vx_unet3d_forward_profiled(const vx_unet3d_weights* w, const vx_unet3d_run* r, vx_stream_t stream,
                                          int max_launches, float* ms, const char** labels, int* n_launches) {
  if (!ms || !labels || !n_launches) VX_FAIL(VX_E_NULL, "vx_unet3d_forward_profiled: null output");
  Prof pf;
  pf.s = (hipStream_t)stream;
  for (int i = 0; i < 2 * Prof::MAXL; ++i) {
    hipError_t e = hipEventCreate(&pf.ev[i]);
    if (e != hipSuccess) VX_FAIL((int)e, "hipEventCreate: %s", hipGetErrorString(e));
  }
  g_prof = &pf;
  int rc = vx_unet3d_forward(w, r, stream);
  g_prof = nullptr;
  if (rc == VX_OK) {
    hipError_t e = hipStreamSynchronize(pf.s);
    if (e != hipSuccess) { vx_set_error("hipStreamSynchronize: %s", hipGetErrorString(e)); rc = (int)e; }
  }
  int n = 0;
  if (rc == VX_OK) {
    for (; n < pf.n && n < max_launches; ++n) {
      float t = 0.f;
      (void)hipEventElapsedTime(&t, pf.ev[2 * n], pf.ev[2 * n + 1]);
      ms[n] = t;
      snprintf(g_prof_labels[n], sizeof(g_prof_labels[n]), "%s|%s", pf.name[n], pf.kernel[n] ? pf.kernel[n] : "?");
      labels[n] = g_prof_labels[n];
    }
  }
  *n_launches = n;
  for (int i = 0; i < 2 * Prof::MAXL; ++i) (void)hipEventDestroy(pf.ev[i]);
  return rc;
}
