// Routing of the 3D streaming passes between the convolutions (norm_apply.hip): every argument check, the kernel instance and the
// launch geometry of vx_instnorm_finalize, vx_norm_act_drop_pool (+ _bcast, _stats), vx_prenorm_split (+ _stats), vx_pool_finish,
// vx_pool_finish_z (+ _stats) and vx_drop_hash_mask.  Host only: pure functions of their arguments -- nothing from HIP, compiles
// with plain g++ (tests/stream3d_route_host.cpp walks it under ASan / UBSan).  An entry point is: its route, then the kernel
// family's launcher with the descriptor.
//
//   instance list         STREAM3D_NORM_INSTANCES: the route asks "does this instance exist?", norm_apply.hip generates its launch
//                         switch from the same line, stream3d_route_name() the name
//   rules                 the pooling lane rule, the bound of the multiply-high decode, the grid's y limit, the grid caps and the
//                         quarter grid of the _stats form -- each stated once, here
//   stream3d_*_route()    one per pass; the plain and the _stats form of a pass are one function that takes a nullable statistics
//                         source and the entry point's name for its messages
//
// Size guards are 128-bit products (vx_wide): no argument can overflow them.
#pragma once
#include "../../include/values_amd.h"
#include "host_checks.h"

enum Stream3dKernel { S3_FINALIZE = 0, S3_NORM, S3_FANOUT, S3_SPLIT, S3_FINISH, S3_FINISH_Z, S3_HASH_MASK, S3_NKERNELS };

// ---- instance list: norm_act_drop_pool_kernel<POOL, WIDE, FOLD>.  The fan-out kernel and the <FOLD> pairs of prenorm_split_kernel and
// pool_finish_z_kernel are kernels of their own ----
#define STREAM3D_NORM_INSTANCES(X) X(1, 1, 1) X(1, 0, 1) X(0, 0, 1) X(1, 1, 0) X(1, 0, 0) X(0, 0, 0)

constexpr int stream3d_key(int pool, int wide, int fold) { return pool * 4 + wide * 2 + fold; }
static inline bool stream3d_norm_instance_exists(int pool, int wide, int fold) {
  if ((pool | wide | fold) & ~1) return false;
#define STREAM3D_EXISTS_CASE(P, W, F) case stream3d_key(P, W, F):
  switch (stream3d_key(pool, wide, fold)) { STREAM3D_NORM_INSTANCES(STREAM3D_EXISTS_CASE) return true; default: return false; }
#undef STREAM3D_EXISTS_CASE
}

// ---- rules ------------------------------------------------------------------------------------------------------------------------
constexpr int VX_STAT_MAXC = 512;        // channels a workgroup's own reduction of the statistics partials keeps in LDS
constexpr int S3_GRID_Y_MAX = 65535;     // blockIdx.y = sample
// Grid caps (x; every kernel walks its pieces with a grid stride).  The normalise pass without pooling and the fan-out kernel: workgroups
// over ALL samples; the small passes: per sample.  The _stats forms run longer-lived workgroups, each reduces the partials once
constexpr int S3_NORM_WGS = 16384, S3_FANOUT_WGS = 32768, S3_HASH_MASK_WGS = 16384;
constexpr int S3_SPLIT_WGS = 512, S3_SPLIT_FOLD_WGS = 128, S3_FINISH_WGS = 64, S3_FINISH_Z_FOLD_WGS = 16;
// workgroups of 256 threads for `pieces` 16-byte pieces, at most cap
static inline int stream3d_blocks(vx_wide pieces, int64_t cap) {
  const vx_wide bx = (pieces + 255) / 256;
  return (int)(bx > cap ? cap : bx);
}
// the workgroups of `samples` samples share `wgs`: each sample's cap (at least 1)
static inline int64_t stream3d_cap_per_sample(int wgs, int samples) { return ((int64_t)wgs + samples - 1) / samples; }
// The _stats form of the normalise pass: four pieces per thread -- the workgroup's reduction of the partials is paid once per 1 024
// pieces instead of 256
static inline int stream3d_quarter(int bx) { return (bx + 3) / 4; }
// Pooling: the x-pair exchange is a shuffle over C/4 lanes.  Both voxels of a pair must sit in one wave: the pieces of a row never
// straddle a 64-lane boundary mid-pair ((W C/4) % (2 C/4) == 0 with W even) and a wave starts at a multiple of 64 pieces, which is a
// multiple of 2 C/4 when C/4 divides 32.  More than 128 channels: a thread takes both voxels (WIDE), no shuffle.  -1: neither
static inline int stream3d_pool_wide(int C) { return C / 4 > 32 ? 1 : 32 % (C / 4) == 0 ? 0 : -1; }
// The piece index within a sample is 32-bit and is split with multiply-high divisions by PW, C/4 <= PW and RH: exact while
// index * divisor < 2^32
static inline bool stream3d_decode_ok(vx_wide per, int PW, int RH) { return per * (PW > RH ? PW : RH) < ((vx_wide)1 << 32); }

// ---- the descriptor a route fills -----------------------------------------------------------------------------------------------
struct Stream3dRoute {
  int kernel;              // Stream3dKernel
  int pool, wide, fold;    // S3_NORM: the instance; S3_SPLIT / S3_FINISH_Z: fold
  int grid_x, grid_y;
  unsigned pieces;         // 16-byte pieces (work items) per sample: the normalise kernels' per_sample
  unsigned mPW, mC4, mH;   // S3_NORM / S3_FANOUT: multiply-high magics of the decode (0: the divisor is 1)
  char err[240];           // the refusal's message (vx_last_error_string) when a route returns < 0
};
static inline void stream3d_clear(Stream3dRoute* r, int kernel) {
  r->kernel = kernel;
  r->pool = r->wide = r->fold = r->grid_x = r->grid_y = 0;
  r->pieces = r->mPW = r->mC4 = r->mH = 0;
  r->err[0] = 0;
}

// a pass that reduces the producing conv's statistics partials itself (vx_stat_src)
static inline int stream3d_stat_check(const vx_stat_src* st, int C, const char* who, Stream3dRoute* r) {
  if (!st || !st->stats_partial) VX_REFUSE(r, VX_E_NULL, "%s: null statistics source", who);
  if (st->tiles <= 0 || st->count <= 0 || C > VX_STAT_MAXC)
    VX_REFUSE(r, VX_E_SHAPE, "%s: %d tiles, %lld values per channel, C = %d (<= %d)", who, st->tiles, (long long)st->count, C, VX_STAT_MAXC);
  return VX_OK;
}

// ---- vx_instnorm_finalize: one workgroup per (sample, channel) ----
static inline int stream3d_finalize_route(const void* stats_partial, int N, int ntiles, int C, int64_t nvox, const void* mean, const void* rstd,
                                          Stream3dRoute* r) {
  stream3d_clear(r, S3_FINALIZE);
  if (!stats_partial || !mean || !rstd) VX_REFUSE(r, VX_E_NULL, "vx_instnorm_finalize: null pointer");
  if (N <= 0 || ntiles <= 0 || C <= 0 || nvox <= 0) VX_REFUSE(r, VX_E_SHAPE, "vx_instnorm_finalize: empty");
  if ((vx_wide)N * C >= ((vx_wide)1 << 31)) VX_REFUSE(r, VX_E_SHAPE, "vx_instnorm_finalize: N * C must stay below 2^31 (N = %d, C = %d)", N, C);
  r->grid_x = N * C;
  r->grid_y = 1;
  return VX_OK;
}

// ---- vx_norm_act_drop_pool, _bcast (x_repeat) and _stats (st): every check in one order, then the instance, the grid and the decode ----
static inline int stream3d_norm_route(const vx_norm_args& a, int x_repeat, const vx_stat_src* st, Stream3dRoute* r) {
  stream3d_clear(r, S3_NORM);
  if (st) {
    const int rc = stream3d_stat_check(st, a.C, "vx_norm_act_drop_pool_stats", r);
    if (rc != VX_OK) return rc;
    if (a.mean || a.rstd) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool_stats: the statistics come from the source, mean / rstd must be NULL");
  }
  if (x_repeat < 1) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: x_repeat must be >= 1");
  // (no entry point pairs the two; the fan-out kernel takes no source)
  if (st && x_repeat != 1) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool_stats: a statistics source goes with x_repeat 1");
  if (!a.x || (!a.out && !a.pool_out)) VX_REFUSE(r, VX_E_NULL, "vx_norm_act_drop_pool: null tensor");
  if (a.x_xblk && ((a.x_xblk != 1 && a.x_xblk != 2 && a.x_xblk != 4) || a.W % a.x_xblk || (a.x_half != 0 && a.x_half != 1)))
    VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: bad concat input (xblk=%d, half=%d, W=%d)", a.x_xblk, a.x_half, a.W);
  if (a.x_xblk && (x_repeat > 1 || !a.pool_out)) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: a concat input goes with pooling, x_repeat 1");
  if ((a.mean == nullptr) != (a.rstd == nullptr)) VX_REFUSE(r, VX_E_NULL, "vx_norm_act_drop_pool: mean/rstd must come together");
  if (a.N <= 0 || a.D <= 0 || a.H <= 0 || a.W <= 0 || a.C <= 0 || a.C % 4)
    VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: bad shape (C must be a multiple of 4)");
  if (!a.x_xblk && (a.x_pitch % 4 || a.x_pitch < a.C)) VX_REFUSE(r, VX_E_ALIGN, "vx_norm_act_drop_pool: input pitch");
  if (!a.out) {
    // pooled tensor only
  } else if (a.out_xblk) {
    if ((a.out_xblk != 1 && a.out_xblk != 2 && a.out_xblk != 4) || a.W % a.out_xblk || (a.out_half != 0 && a.out_half != 1))
      VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: bad concat layout (xblk=%d, half=%d, W=%d)", a.out_xblk, a.out_half, a.W);
  } else if (a.out_pitch % 4 || a.out_coff % 4 || a.out_pitch < (int64_t)a.out_coff + a.C) {
    VX_REFUSE(r, VX_E_ALIGN, "vx_norm_act_drop_pool: pitches/offsets must be multiples of 4 floats");
  }
  if (a.drop_mode == VX_DROP_MASK && !a.drop_mask) VX_REFUSE(r, VX_E_NULL, "vx_norm_act_drop_pool: mask mode without mask");
  // the dropout element index ((z H + y) W + x) C + c of one sample is a 32-bit word
  if ((vx_wide)a.D * a.H * a.W * a.C >= ((vx_wide)1 << 32)) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: sample too large");
  const int pool = a.pool_out ? 1 : 0;
  int wide = 0;
  if (pool) {
    if (a.D % 2 || a.H % 2 || a.W % 2) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: pooling needs even dims");
    if (a.pool_pitch % 4 || a.pool_pitch < a.C) VX_REFUSE(r, VX_E_ALIGN, "vx_norm_act_drop_pool: pool pitch");
    wide = stream3d_pool_wide(a.C);
    if (wide < 0) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: pooling needs C/4 to divide 32, or C > 128 (C = %d)", a.C);
  }
  // work items per row, rows (row bundles) per z, planes: ints by the sample guard
  const int C4 = a.C / 4, PW = (wide ? a.W / 2 : a.W) * C4, RH = pool ? a.H / 2 : a.H, RD = pool ? a.D / 2 : a.D;
  const vx_wide per = (vx_wide)RD * RH * PW;
  const bool fanout = !pool && x_repeat > 1;
  // grid y = samples: N, or the N / x_repeat source samples of the fan-out kernel
  r->grid_y = fanout ? a.N / x_repeat : a.N;
  if (!stream3d_decode_ok(per, PW, RH) || r->grid_y > S3_GRID_Y_MAX)
    VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: sample too large for the 32-bit index decode (%lld pieces) or more than 65535 samples in the grid (%d)",
              (long long)per, r->grid_y);
  if (fanout && a.N % x_repeat) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: N=%d is not a multiple of x_repeat=%d", a.N, x_repeat);
  // the kernels form the plane index n D + z in an int before they widen it.  (A concat row's offset < 2 W C is an int by the decode
  // bound: PW^2 <= per PW < 2^32 leaves W C < 2^19)
  if ((vx_wide)r->grid_y * a.D >= ((vx_wide)1 << 31) || (!fanout && (vx_wide)a.N * a.D >= ((vx_wide)1 << 31)))
    VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: the plane index n D + z must stay below 2^31 (N = %d, D = %d)", a.N, a.D);
  r->pieces = (unsigned)per;
  r->mPW = vx_magic_or0(PW); r->mC4 = vx_magic_or0(C4); r->mH = vx_magic_or0(RH);
  if (fanout) {
    r->kernel = S3_FANOUT;
    r->grid_x = stream3d_blocks(per, stream3d_cap_per_sample(S3_FANOUT_WGS, r->grid_y));
    return VX_OK;
  }
  r->pool = pool; r->wide = wide; r->fold = st ? 1 : 0;
  if (!stream3d_norm_instance_exists(r->pool, r->wide, r->fold)) VX_REFUSE(r, VX_E_SHAPE, "vx_norm_act_drop_pool: no such instance");   // (not reached)
  r->grid_x = stream3d_blocks(per, pool ? INT32_MAX : stream3d_cap_per_sample(S3_NORM_WGS, a.N));
  if (st) r->grid_x = stream3d_quarter(r->grid_x);
  return VX_OK;
}

// ---- vx_prenorm_split (mean / rstd) and vx_prenorm_split_stats (fold: st): C = 8, in place ----
static inline int stream3d_split_route(const char* who, const void* x, const void* mean, const void* rstd, bool fold, const vx_stat_src* st,
                                       int N, int64_t nvox, Stream3dRoute* r) {
  stream3d_clear(r, S3_SPLIT);
  if (!x || (!fold && (!mean || !rstd))) VX_REFUSE(r, VX_E_NULL, "%s: null pointer", who);
  if (N <= 0 || N > S3_GRID_Y_MAX || nvox <= 0 || nvox >= (1ll << 30)) VX_REFUSE(r, VX_E_SHAPE, "%s: empty / too large", who);
  if (!vx_aligned16(x) || (!fold && (!vx_aligned16(mean) || !vx_aligned16(rstd)))) VX_REFUSE(r, VX_E_ALIGN, "%s: alignment", who);
  if (fold) {
    const int rc = stream3d_stat_check(st, 8, who, r);
    if (rc != VX_OK) return rc;
  }
  r->fold = fold;
  r->pieces = (unsigned)(nvox * 2);
  r->grid_x = stream3d_blocks(r->pieces, fold ? S3_SPLIT_FOLD_WGS : S3_SPLIT_WGS);
  r->grid_y = N;
  return VX_OK;
}

// ---- vx_pool_finish: C = 8 ----
static inline int stream3d_finish_route(const void* pool_raw, const void* pool_flags, const void* mean, const void* rstd, const void* out,
                                        int out_pitch, int N, int64_t voxels_per_sample, Stream3dRoute* r) {
  stream3d_clear(r, S3_FINISH);
  if (!pool_raw || !pool_flags || !mean || !rstd || !out) VX_REFUSE(r, VX_E_NULL, "vx_pool_finish: null pointer");
  if (N <= 0 || voxels_per_sample <= 0 || voxels_per_sample >= (1ll << 30)) VX_REFUSE(r, VX_E_SHAPE, "vx_pool_finish: empty / too large");
  if (out_pitch < 8 || out_pitch % 4 || !vx_aligned16(pool_raw) || !vx_aligned16(out))
    VX_REFUSE(r, VX_E_ALIGN, "vx_pool_finish: pitch %d / alignment", out_pitch);
  if (N > S3_GRID_Y_MAX) VX_REFUSE(r, VX_E_SHAPE, "vx_pool_finish: N");
  r->pieces = (unsigned)(voxels_per_sample * 2);
  r->grid_x = stream3d_blocks(r->pieces, S3_FINISH_WGS);
  r->grid_y = N;
  return VX_OK;
}

// ---- vx_pool_finish_z (mean / rstd) and vx_pool_finish_z_stats (fold: st): C = 16, Dp pooled planes of plane_voxels voxels ----
static inline int stream3d_finish_z_route(const char* who, const void* pool_raw, const void* pool_flags, const void* mean, const void* rstd,
                                          bool fold, const vx_stat_src* st, const void* out, int out_pitch, int N, int Dp, int64_t plane_voxels,
                                          Stream3dRoute* r) {
  stream3d_clear(r, S3_FINISH_Z);
  if (!pool_raw || !pool_flags || !out || (!fold && (!mean || !rstd))) VX_REFUSE(r, VX_E_NULL, "%s: null pointer", who);
  if (N <= 0 || Dp <= 0 || plane_voxels <= 0 || (vx_wide)Dp * plane_voxels >= (1ll << 28)) VX_REFUSE(r, VX_E_SHAPE, "%s: empty / too large", who);
  if (out_pitch < 16 || out_pitch % 4 || !vx_aligned16(pool_raw) || !vx_aligned16(out)) VX_REFUSE(r, VX_E_ALIGN, "%s: pitch %d / alignment", who, out_pitch);
  if (N > S3_GRID_Y_MAX) VX_REFUSE(r, VX_E_SHAPE, "%s: N", who);
  if (fold) {
    const int rc = stream3d_stat_check(st, 16, who, r);
    if (rc != VX_OK) return rc;
  }
  r->fold = fold;
  r->pieces = (unsigned)(Dp * plane_voxels * 4);
  r->grid_x = stream3d_blocks(r->pieces, fold ? S3_FINISH_Z_FOLD_WGS : S3_FINISH_WGS);
  r->grid_y = N;
  return VX_OK;
}

// ---- vx_drop_hash_mask: one thread per four elements, over all samples ----
static inline int stream3d_hash_mask_route(int N, int64_t elems_per_sample, const void* mask, Stream3dRoute* r) {
  stream3d_clear(r, S3_HASH_MASK);
  if (N <= 0 || elems_per_sample <= 0 || elems_per_sample % 4 || elems_per_sample >= (1ll << 32))
    VX_REFUSE(r, VX_E_SHAPE, "vx_drop_hash_mask: N=%d, %lld elements per sample (a positive multiple of 4 below 2^32)", N, (long long)elems_per_sample);
  if (!mask || (((uintptr_t)mask) & 3u)) VX_REFUSE(r, VX_E_ALIGN, "vx_drop_hash_mask: mask must be a 4-byte aligned device pointer");
  r->grid_x = stream3d_blocks((vx_wide)N * (elems_per_sample / 4), S3_HASH_MASK_WGS);
  r->grid_y = 1;
  return VX_OK;
}

// the name vx_last_kernel_name() reports after the launch (the passes that note one).  Returns the length snprintf reports
static inline int stream3d_route_name(const Stream3dRoute& r, char* buf, int cap) {
  if (cap < 0) cap = 0;
  const char* b[2] = {"false", "true"};
  switch (r.kernel) {
    case S3_FINALIZE: return snprintf(buf, cap, "instnorm_finalize_kernel");
    case S3_NORM: return snprintf(buf, cap, "norm_act_drop_pool_kernel<%s,%s%s>", b[r.pool != 0], b[r.wide != 0], r.fold ? ",true" : "");
    case S3_FANOUT: return snprintf(buf, cap, "norm_act_drop_fanout_kernel");
    case S3_SPLIT: return snprintf(buf, cap, "prenorm_split_kernel<%s>", b[r.fold != 0]);
    case S3_FINISH: return snprintf(buf, cap, "pool_finish_kernel");
    case S3_FINISH_Z: return snprintf(buf, cap, "pool_finish_z_kernel<%s>", b[r.fold != 0]);
  }
  return snprintf(buf, cap, "drop_hash_mask_kernel");
}
