// Routing of vx_conv3d_k3: which kernel family and which instance runs a 3x3x3 layer, and with what launch geometry.
// Host only: a pure function of (vx_conv3d_args, vx_config) -- nothing from HIP, compiles with plain g++ (tests/conv3d_route_host.cpp
// walks it under ASan / UBSan).  vx_conv3d_k3 is: conv3d_route(), then the family's launcher with the descriptor.
//
//   shape / channel rules   conv_config, s16_config, tile_config, vx_conv3d_s16_tile, conv3d_*_applies / _packs, deep_geo / deep_pick,
//                           deep_tail (how the deep kernel's last round is shared; tests/deep_tail_host.cpp), the family numbering,
//                           the packed sizes and the tile counts -- each stated once, here
//   instance lists          one X-macro per family (MFMA_ / C8_ / S16_ / XP8W_ / ZC16_ / DEEP_INSTANCES): the route asks "does this
//                           instance exist?", the family's .hip file instantiates launch_X<...> from the same list
//   conv3d_route()          every argument check of vx_conv3d_k3 in one order; the families are tried xp8w -> zc16 -> deep -> tile
//                           kernels, and a family that does not take a launch is an ordinary step of this function
//   conv3d_route_name()     the instance name vx_last_kernel_name() reports (as rocprofv3 prints it)
//   conv3d_*_ok rules       the public vx_conv3d_k3_*_ok predicates, built from the rules the route itself applies
//
// Adding an instance: one X(...) line in the family's list, plus the rule in that family's route_*() step that selects it.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/values_amd.h"
#include "host_checks.h"

// ---- constants shared with the kernel files ---------------------------------------------------------------------------------
constexpr int DEEP_NPOS = 1080;                    // conv3d_deep: positions of one LDS image (18 x 10 x 6), the R = 4 tile's cap
constexpr int DEEP_NPOS_R2 = 896;                  //   the R = 2 tile's cap (2 npos pieces in IN_IT x 256)
constexpr int DEEP_W_B = 7 * 2 * 2 * 1024;         //   bytes of one 8-channel chunk's weights
constexpr int DEEP_MAXC = 512;                     //   output channels the bias vector in LDS holds
constexpr int DEEP_MAXDIM = 32;                    //   the larger layers keep the tile kernel's XCD-ordered small tiles
constexpr int S16_HEAD_MAXC = 4;                   // classes the split-fp16 kernels' fused head takes

enum Conv3dKernel { CONV3D_MFMA = 0, CONV3D_C8, CONV3D_S16, CONV3D_XP8W, CONV3D_ZC16, CONV3D_DEEP, CONV3D_NKERNELS };

// ---- instance lists: the template parameters of every instantiated kernel, in the kernel template's order --------------------
// conv3d_k3_mfma_kernel<CB, NT, TX, TY, TZ, NW, XP>
#define MFMA_TILES(X, CB, NT, XP) X(CB, NT, 16, 4, 4, 8, XP) X(CB, NT, 8, 8, 4, 8, XP) X(CB, NT, 4, 4, 4, 4, XP)
#define MFMA_INSTANCES(X) MFMA_TILES(X, 8, 1, 1) MFMA_TILES(X, 16, 1, 0) MFMA_TILES(X, 16, 2, 0) MFMA_TILES(X, 8, 1, 0) MFMA_TILES(X, 8, 2, 0)
// conv3d_k3_c8_kernel<NCH, TXV, TY, TZ>
#define C8_INSTANCES(X) X(1, 32, 4, 4) X(2, 32, 4, 4) X(1, 16, 8, 4) X(2, 16, 8, 4) X(1, 8, 4, 4) X(2, 8, 4, 4)
// conv3d_k3_s16_kernel<CB, NT, TX, TY, TZ, NW, XP, DB, EPI>, one list per translation unit (conv3d_s16.hip, S16_PART)
#define S16_SMALL(X, CB, NT, XP)                                                                                       \
  X(CB, NT, 16, 4, 4, 8, XP, 0, 0) X(CB, NT, 16, 4, 4, 8, XP, 0, 1) X(CB, NT, 16, 4, 4, 8, XP, 0, 3)                     \
  X(CB, NT, 8, 8, 4, 8, XP, 0, 0) X(CB, NT, 8, 8, 4, 8, XP, 0, 1) X(CB, NT, 8, 8, 4, 8, XP, 0, 3) X(CB, NT, 4, 4, 4, 4, XP, 0, 3)
#define S16_LARGE(X, CB, XP) X(CB, 1, 16, 8, 4, 8, XP, 0, 0) X(CB, 1, 16, 8, 4, 8, XP, 0, 1) X(CB, 1, 16, 8, 4, 8, XP, 0, 3)
#define S16_DB_PLAIN(X, CB, NT) X(CB, NT, 16, 4, 4, 8, 0, 2, 0) X(CB, NT, 16, 4, 4, 8, 0, 2, 1) X(CB, NT, 16, 4, 4, 8, 0, 2, 3)
#define S16_DB_XP(X)                                                                                                   \
  X(8, 1, 16, 8, 4, 8, 1, 2, 0) X(8, 1, 16, 8, 4, 8, 1, 2, 1) X(8, 1, 16, 8, 4, 8, 1, 2, 2) X(8, 1, 16, 8, 4, 8, 1, 2, 3) \
  X(8, 1, 16, 8, 4, 8, 1, 3, 1) X(8, 1, 16, 8, 4, 8, 1, 3, 3)
#define S16_INSTANCES_PART0(X) S16_SMALL(X, 16, 1, 0) S16_LARGE(X, 16, 0) S16_DB_PLAIN(X, 16, 1)
#define S16_INSTANCES_PART1(X)                                                                                         \
  S16_SMALL(X, 8, 1, 1) S16_LARGE(X, 8, 1) S16_DB_XP(X) S16_SMALL(X, 8, 1, 0) S16_LARGE(X, 8, 0) S16_DB_PLAIN(X, 8, 1) \
  S16_SMALL(X, 8, 2, 0) S16_DB_PLAIN(X, 8, 2)
#define S16_INSTANCES_PART2(X) S16_SMALL(X, 16, 2, 0) S16_DB_PLAIN(X, 16, 2)
#define S16_INSTANCES(X) S16_INSTANCES_PART0(X) S16_INSTANCES_PART1(X) S16_INSTANCES_PART2(X)
// conv3d_xp8w_kernel<NCH, EPI, PRE, UP, NPW, IN16>: producer waves NPW = 8 (two per SIMD) for the two-chunk layers, whose staging is
// the heavy side; 4 for the one-chunk layers (their consumers hold R = 4 image rows + accumulators: at 16 waves per workgroup every
// one-chunk instance spilled).  IN16 = 1 / 3: the fp16 input of the head layer; IN16 = 2 / 3: products = 1.
#define XP8W_INSTANCES(X)                                                                                              \
  X(1, 4, 0, 0, 4, 0) X(1, 4, 1, 0, 4, 0) X(1, 4, 2, 0, 4, 0) X(1, 0, 2, 0, 4, 0) X(1, 0, 0, 0, 4, 0) X(1, 0, 1, 0, 4, 0)  \
  X(1, 1, 0, 0, 4, 0) X(1, 2, 0, 0, 4, 0) X(1, 3, 0, 0, 4, 0) X(1, 3, 1, 0, 4, 0) X(1, 5, 0, 0, 4, 0)                      \
  X(2, 1, 0, 0, 8, 0) X(2, 1, 1, 0, 8, 0) X(2, 3, 0, 0, 8, 0) X(2, 3, 1, 0, 8, 0)                                          \
  X(2, 1, 0, 1, 8, 0) X(2, 1, 1, 1, 8, 0) X(2, 3, 0, 1, 8, 0) X(2, 3, 1, 1, 8, 0)                                          \
  X(2, 1, 0, 2, 8, 0) X(2, 1, 1, 2, 8, 0) X(2, 3, 0, 2, 8, 0) X(2, 3, 1, 2, 8, 0)                                          \
  X(1, 2, 0, 0, 4, 1) X(1, 2, 0, 0, 4, 3) X(1, 4, 2, 0, 4, 2) X(2, 1, 1, 2, 8, 2)
// conv3d_zc16_kernel<CIN, EPI, PRE, ACC, UP>
#define ZC16_INSTANCES(X)                                                                                              \
  X(16, 0, 0, 0, 0) X(16, 0, 1, 0, 0) X(16, 4, 0, 0, 0) X(16, 4, 1, 0, 0) X(16, 1, 0, 0, 0) X(16, 1, 1, 0, 0)              \
  X(16, 3, 0, 0, 0) X(16, 3, 1, 0, 0) X(16, 1, 4, 0, 0) X(16, 3, 4, 0, 0) X(16, 5, 0, 0, 0) X(16, 6, 0, 0, 0)              \
  X(8, 0, 0, 0, 0) X(8, 0, 3, 0, 0) X(8, 3, 0, 0, 0) X(8, 1, 0, 0, 0)                                                      \
  X(16, 1, 0, 1, 0) X(16, 3, 0, 1, 0) X(16, 1, 0, 0, 1) X(16, 3, 0, 0, 1)                                                  \
  X(16, 1, 0, 1, 1) X(16, 3, 0, 1, 1) X(16, 5, 0, 1, 1) X(16, 6, 0, 1, 1)
// conv3d_deep_kernel<R, EPI, PRE>
#define DEEP_INSTANCES(X) X(4, 0, 0) X(4, 0, 1) X(4, 1, 0) X(4, 3, 0) X(2, 0, 0) X(2, 0, 1) X(2, 1, 0) X(2, 3, 0)

// one integer per instance: the `case` label of the launchers' switches and of conv3d_instance_exists (every parameter < 64)
constexpr uint64_t conv3d_key(int a, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0, int g = 0, int h = 0, int i = 0) {
  return ((((((((uint64_t)a * 64 + b) * 64 + c) * 64 + d) * 64 + e) * 64 + f) * 64 + g) * 64 + h) * 64 + i;
}
static inline uint64_t conv3d_key_of(const int* p, int np) {
  int q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < np; ++i) q[i] = p[i];
  return conv3d_key(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
}
#define CONV3D_EXISTS_CASE(...) case conv3d_key(__VA_ARGS__):
static inline bool conv3d_instance_exists(int kernel, const int* p, int np) {
  const uint64_t key = conv3d_key_of(p, np);
  switch (kernel) {
    case CONV3D_MFMA: switch (key) { MFMA_INSTANCES(CONV3D_EXISTS_CASE) return true; default: return false; }
    case CONV3D_C8:   switch (key) { C8_INSTANCES(CONV3D_EXISTS_CASE) return true; default: return false; }
    case CONV3D_S16:  switch (key) { S16_INSTANCES(CONV3D_EXISTS_CASE) return true; default: return false; }
    case CONV3D_XP8W: switch (key) { XP8W_INSTANCES(CONV3D_EXISTS_CASE) return true; default: return false; }
    case CONV3D_ZC16: switch (key) { ZC16_INSTANCES(CONV3D_EXISTS_CASE) return true; default: return false; }
    case CONV3D_DEEP: switch (key) { DEEP_INSTANCES(CONV3D_EXISTS_CASE) return true; default: return false; }
  }
  return false;
}

// ---- the descriptor conv3d_route() fills ----------------------------------------------------------------------------------------
struct Conv3dRoute {
  int kernel;                      // Conv3dKernel
  int np, p[9];                    // the instance's template parameters (lists above)
  int64_t w_off;                   // floats from w_packed to this kernel's block of the packed weights (families 6 / 7)
  int tiles_x, tiles_y, tiles_z;   // tiles per sample along each axis (z-column kernels: columns along x, y)
  unsigned mx, my, mz;             // multiply-high magics floor(2^32 / tiles_*) + 1: exact t / tiles_* for t * tiles_* < 2^32
  int nchunks;                     // input chunks of the kernel's chunk size
  int ty8;                         // s16: 16 x 8 x 4 tiles
  int kz;                          // z-column kernels: items per column
  int nitems;                      // z-column kernels: columns in the launch; deep: (tile, output group) pairs
  unsigned mcps;                   // z-column kernels: magic of columns per sample
  int rep; unsigned mrep;          // xp8w: in_repeat as the column order's inner factor, and its magic
  int stat_epc;                    // statistics entries per column / tile in stats_partial (entry 0 real, the rest zero; deep: the
                                   //   first stat_parts)
  int stat_parts, tail_cap;        // deep: wave groups a tile's statistics are written by; largest split of a last-round pair
  int tx, ty, tz, ts, npos, ncg;   // deep: tile voxels along x, y, z; samples per tile; halo positions; 32-row output groups
  unsigned m_cg;                   // deep: magic of ncg
  char err[400];                   // the refusal's message (vx_last_error_string) when conv3d_route returns < 0
};

static inline bool conv3d_pow2(int64_t v) { return (v & (v - 1)) == 0; }
// the 32-bit offset guards: bytes of a sample, as a product no argument can overflow (four int factors and a small constant)
constexpr int64_t CONV3D_2GIB = 1ll << 31;

// ---- channel rules ------------------------------------------------------------------------------------------------------------
// Packing of the 16-row tile: NT row tiles per wave, XP = x-pair packing (Cout == 8), CB channels per chunk (x-pair layers always go
// in chunks of 8).  The same for the fp32 tile kernel and the split-fp16 one.
struct S16Cfg { int CB, NT, XP; };
static inline S16Cfg s16_config(int Cin, int Cout) {
  S16Cfg c;
  c.NT = (Cout % 32 == 0) ? 2 : 1;
  c.XP = Cout == 8 ? 1 : 0;
  c.CB = c.XP ? 8 : ((Cin % 16 == 0) ? 16 : 8);
  return c;
}
static inline bool conv3d_c8_applies(int Cin, int Cout) { return Cout == 8 && (Cin == 8 || Cin == 16); }
// Default: the split-fp16 schedule (S16) for every layer -- faster AND closer to float64 than the native fp32 matrix instruction
// (DESIGN.md section 5).  conv_fp32 = 1 selects the native-fp32 kernels (conv3d_mfma.hip / conv3d_c8.hip: an exact fmaf chain; the A/B
// baseline), conv_fp32 = 2 keeps fp32 only for Cout = 8.  A launch checks its weights' w_family against what this gives NOW.
struct ConvCfg { int CB, NT, XP, C8, S16; };
static inline ConvCfg conv_config(int Cin, int Cout, const vx_config& cfg) {
  const S16Cfg s = s16_config(Cin, Cout);
  ConvCfg c;
  c.CB = s.CB; c.NT = s.NT; c.XP = s.XP;
  c.S16 = (cfg.conv_fp32 == 0 || (cfg.conv_fp32 == 2 && Cout != 8)) ? 1 : 0;
  c.C8 = (!c.S16 && conv3d_c8_applies(Cin, Cout)) ? 1 : 0;
  return c;
}
static inline bool conv3d_channels_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0; }
static inline int64_t conv_rows_padded(int Cout, int NT) { return (((int64_t)Cout + 16 * NT - 1) / (16 * NT)) * (16 * NT); }
// the split-fp16 tile kernel: the x-pair layers carry the fused head, the plain ones the normalise-on-load prologue
static inline bool conv3d_s16_head_fusable(int Cin, int Cout) { return s16_config(Cin, Cout).XP != 0; }
static inline bool conv3d_s16_prologue_ok(int Cin, int Cout) { return s16_config(Cin, Cout).XP == 0; }

static inline bool conv3d_zc16_packs(int Cin, int Cout) { return Cout == 16 && (Cin == 8 || Cin == 16); }
static inline bool conv3d_deep_packs(int Cin, int Cout) { return Cout % 32 == 0 && Cin % 8 == 0 && Cin >= 16 && Cout <= DEEP_MAXC; }

// ---- shape rules --------------------------------------------------------------------------------------------------------------
// xp8w: the full-resolution Cout = 8 layers.  D >= 8: a column has at least two items (the statistics hand-off between the wave
// halves needs the spacing)
static inline bool conv3d_xp8_applies(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  if (cfg.conv_fp32 != 0 || cfg.s16_no_xp8) return false;
  return Cout == 8 && (Cin == 8 || Cin == 16) && W % 32 == 0 && H % 8 == 0 && D % 4 == 0 && W >= 32 && H >= 8 && D >= 8;
}
// zc16: the Cout = 16 layers below full resolution.  D >= 4: at least two items per column, as above
static inline bool conv3d_zc16_applies(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  if (cfg.conv_fp32 != 0 || cfg.s16_no_zc16) return false;
  return conv3d_zc16_packs(Cin, Cout) && W % 32 == 0 && H % 8 == 0 && D % 2 == 0 && W >= 32 && H >= 8 && D >= 4;
}
// deep: tile of a layer = 128 R voxels, x first (the whole row up to 16), then y (up to 8), then z; a tile that is a whole sample
// takes further samples (the last tile of a batch may hold fewer: the kernel masks them).  false = no tile of this size.
// The geometry is a function of the VOLUME's shape only, never of the batch size: a sample's bits must not depend on its batch
// mates (tests/test_gpu_kernels.py::test_conv3d_deep_is_batch_independent).
struct DeepGeo { int tx, ty, tz, ts, tiles_x, tiles_y, tiles_z, npos; };
static inline bool deep_geo(int D, int H, int W, int R, DeepGeo* o) {
  const int vox = 128 * R;
  const int tx = W < 16 ? W : 16;
  if (tx < 4 || !conv3d_pow2(tx) || W % tx) return false;
  int ty = H < 8 ? H : 8;
  while (tx * ty > vox) ty >>= 1;
  if (ty < 1 || H % ty) return false;
  int tz = vox / (tx * ty);
  if (tz > D) tz = D;
  if (tz < 1 || D % tz) return false;
  const int ts = vox / (tx * ty * tz);
  if (ts * tx * ty * tz != vox) return false;
  if (!conv3d_pow2(ty) || !conv3d_pow2(tz)) return false;      // (the kernel decodes a tile's voxels with shifts)
  if (ts > 1 && (tx != W || ty != H || tz != D || ts > 4 || R != 2)) return false;   // (the kernel masks a partial last tile for R = 2 only)
  const int npos = ts * (tx + 2) * (ty + 2) * (tz + 2);
  if (npos > (R == 4 ? DEEP_NPOS : DEEP_NPOS_R2)) return false;
  o->tx = tx; o->ty = ty; o->tz = tz; o->ts = ts;
  o->tiles_x = W / tx; o->tiles_y = H / ty; o->tiles_z = D / tz; o->npos = npos;
  return true;
}
// the layer's tile: R = 4 wherever it fits, else R = 2 (0: neither).  (At 8^3 x 64 channels and 320 samples the large tile is 2 %
// faster; at 16^3 the small tile costs 20 %.)
static inline int deep_pick(int D, int H, int W, DeepGeo* o) {
  if (deep_geo(D, H, W, 4, o)) return 4;
  return deep_geo(D, H, W, 2, o) ? 2 : 0;
}
// The last, partly filled round of the deep kernel's persistent grid: P (tile, output group) pairs on G workgroups are `full` whole
// rounds (workgroup vb runs pairs vb + i G) and `rest` pairs from `tail0` on.  Where split * rest <= G, each of those goes to `split`
// workgroups (4, else 2), which all stage the whole pair and multiply 8 / split of its eight multiplying waves' column tiles each --
// the tile and every stored value's accumulation chain stay what they are, so a sample's bits do not depend on where it stands in
// the batch.  cap: the largest split the launch admits (statistics: deep_stat_parts).  grid: workgroups to launch.
struct DeepTail { int full, rest, split, tail0, grid; };
static inline DeepTail deep_tail(int P, int G, int cap) {
  DeepTail t;
  if (G < 1) G = 1;
  t.full = P / G;
  t.tail0 = t.full * G;
  t.rest = P - t.tail0;
  t.split = 1;
  for (int s = 4; s >= 2; s >>= 1)
    if (t.split == 1 && s <= cap && t.rest > 0 && (int64_t)t.rest * s <= G) t.split = s;
  t.grid = t.full > 0 ? G : t.rest * t.split;
  return t;
}
// Statistics of a tile are written as per-wave-group entries -- by every tile, shared or not, so that the sums InstanceNorm reads are
// the same bits either way: as many groups (4, 2) as the tile's block of the partials buffer holds entries, a function of the
// layer's shape only.  One entry: one group, and statistics launches share no pair.
static inline int deep_stat_parts(int stat_epc) { return stat_epc >= 4 ? 4 : (stat_epc >= 2 ? 2 : 1); }
static inline bool conv3d_deep_applies(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  if (cfg.conv_fp32 != 0 || cfg.s16_no_deep) return false;
  if (!conv3d_deep_packs(Cin, Cout)) return false;
  if (W > DEEP_MAXDIM || H > DEEP_MAXDIM || D > DEEP_MAXDIM) return false;
  DeepGeo g;
  return deep_pick(D, H, W, &g) != 0;
}

// ---- tiles of the tile kernels ------------------------------------------------------------------------------------------------
// fp32 tile kernel and conv3d_c8: TX = columns per column tile row (the x extent in voxels, TXV, is 2 TX for x-pair)
struct TileCfg { int TX, TY, TZ, TXV; };
static inline TileCfg tile_config(int W, int XP) {
  if (XP) {
    if (W >= 32) return {16, 4, 4, 32};
    if (W >= 16) return {8, 8, 4, 16};
    return {4, 4, 4, 8};
  }
  if (W >= 16) return {16, 4, 4, 16};
  if (W >= 8) return {8, 8, 4, 8};
  return {4, 4, 4, 4};
}
// split-fp16 tile kernel: tx columns per row as above; large layers (H >= 32) take 16 x 8 x 4 tiles = 4 column tiles per wave: the
// halo read per output voxel drops from 2.5x to 2.1x and the per-item costs (barriers, decode, masks) halve -- +14..20 % on the 64^3
// layers; small layers keep 16 x 4 x 4 so that the 256 CUs still get enough work items.
static inline void vx_conv3d_s16_tile(int H, int W, int Cout, int* txv, int* ty, int* tz) {
  const int xp = s16_config(8, Cout).XP;
  const int wcols = xp ? W / 2 : W;
  const int tx = wcols >= 16 ? 16 : (wcols >= 8 ? 8 : 4);
  // two row tiles per wave (Cout % 32 == 0) on the large tile would need > 256 registers (75 spilled): small tile there
  // (measured 32->32 @64^3: 321 TFLOP/s on 16x4x4 tiles against 204 on the spilling 16x8x4 instance)
  const bool nt2 = !xp && Cout % 32 == 0;
  const bool ty8 = tx == 16 && H >= 32 && !nt2;
  *txv = xp ? 2 * tx : tx;
  *ty = (tx == 8 || ty8) ? 8 : 4;
  *tz = 4;
}
static inline int conv3d_tiles_along(int n, int t) { return (int)(((int64_t)n + t - 1) / t); }
static inline int conv3d_tile_count(int D, int H, int W, int txv, int ty, int tz) {   // (wraps like int for volumes no launch takes)
  return (int)((unsigned)conv3d_tiles_along(W, txv) * (unsigned)conv3d_tiles_along(H, ty) * (unsigned)conv3d_tiles_along(D, tz));
}
// exact tiles per sample of the tile kernel a Cout runs on (what a caller sizes stats_partial rows by)
static inline int conv3d_tiles_for(int D, int H, int W, int Cout, const vx_config& cfg) {
  if (conv_config(8, Cout, cfg).S16) {
    int txv, ty, tz;
    vx_conv3d_s16_tile(H, W, Cout, &txv, &ty, &tz);
    return conv3d_tile_count(D, H, W, txv, ty, tz);
  }
  const TileCfg t = tile_config(W, Cout == 8);
  return conv3d_tile_count(D, H, W, t.TXV, t.TY, t.TZ);
}
// upper bound over every packing, Cout and mode.  Neither tiling dominates: for 8 <= W < 16 the x-pair tile (4 pairs x 4 x 4) makes
// twice the tiles of the plain 8 x 8 x 4 one, for W >= 16 it is the reverse
static inline int conv3d_tiles_max(int D, int H, int W) {
  int best = 0;
  for (int xp = 0; xp < 2; ++xp) {
    const TileCfg t = tile_config(W, xp);
    const int n = conv3d_tile_count(D, H, W, t.TXV, t.TY, t.TZ);
    if (n > best) best = n;
  }
  const int couts[3] = {8, 16, 32};   // split-fp16: x-pair / one row tile (large tile) / two row tiles
  for (int i = 0; i < 3; ++i) {
    int txv, ty, tz;
    vx_conv3d_s16_tile(H, W, couts[i], &txv, &ty, &tz);
    const int n = conv3d_tile_count(D, H, W, txv, ty, tz);
    if (n > best) best = n;
  }
  return best;
}

// ---- packed weights -----------------------------------------------------------------------------------------------------------
static inline int64_t conv3d_s16_packed_floats(int Cin, int Cout) {
  const S16Cfg c = s16_config(Cin, Cout);
  const int TPS = 32 / c.CB, NSTEP = c.XP ? 9 : (27 + TPS - 1) / TPS;
  const int64_t halves = (int64_t)(conv_rows_padded(Cout, c.NT) / 16) * (Cin / c.CB) * NSTEP * 2 * (c.XP ? 32 : 64) * 8;
  return halves / 2;
}
static inline int64_t conv3d_zc16_packed_floats(int Cin, int Cout) {
  return conv3d_zc16_packs(Cin, Cout) ? (int64_t)(Cin == 16 ? 14 : 9) * 2 * 64 * 8 / 2 : 0;
}
static inline int64_t conv3d_deep_packed_floats(int Cin, int Cout) {
  return conv3d_deep_packs(Cin, Cout) ? (int64_t)(Cout / 32) * (Cin / 8) * (DEEP_W_B / 4) : 0;
}
// Kernel family = packed layout of a layer under a configuration (values_amd.h, vx_config):
//   1 split-fp16 fragments, 2 split-fp16 x-pair blocks, 3 fp32 fragments, 4 fp32 x-pair, 5 fp32 4x4x1 (Cout = 8),
//   6 the split-fp16 tile kernel's fragments FOLLOWED BY the z-column kernel's (conv3d_zc16.hip: which of the two runs depends on the
//     volume's shape, known only at launch), 7 the same FOLLOWED BY the deep-layer kernel's (conv3d_deep.hip)
static inline int conv3d_family(int Cin, int Cout, const vx_config& cfg) {
  if (!conv3d_channels_ok(Cin, Cout)) return 0;
  const ConvCfg c = conv_config(Cin, Cout, cfg);
  if (c.S16) {
    if (c.XP) return 2;
    if (conv3d_deep_packs(Cin, Cout)) return 7;      // (never both: the z-column kernel packs Cout = 16)
    return conv3d_zc16_packs(Cin, Cout) ? 6 : 1;
  }
  if (c.C8) return 5;
  return c.XP ? 4 : 3;
}
static inline int64_t conv3d_packed_floats(int Cin, int Cout, const vx_config& cfg) {
  if (!conv3d_channels_ok(Cin, Cout)) return -1;
  const ConvCfg c = conv_config(Cin, Cout, cfg);
  if (c.C8) return (int64_t)27 * Cin * 8;
  if (c.S16) return conv3d_s16_packed_floats(Cin, Cout) + conv3d_zc16_packed_floats(Cin, Cout) + conv3d_deep_packed_floats(Cin, Cout);
  if (c.XP) return (int64_t)16 * Cin * 36;
  return (int64_t)conv_rows_padded(Cout, c.NT) * Cin * 27;
}

// ---- feature rules: what the public vx_conv3d_k3_*_ok predicates answer, and what conv3d_route() applies ----------------------------
// the 16 -> 16 layers of the z-column kernel: partial sums (acc_in), the planar hand-over, the fused ConvTranspose3d(32 -> 16) and
// the (y, x) pooled output all live in its instances only
static inline bool conv3d_zc16_16to16(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  return Cin == 16 && Cout == 16 && conv_config(Cin, Cout, cfg).S16 && conv3d_zc16_applies(D, H, W, Cin, Cout, cfg);
}
static inline int conv3d_head_fusable(int Cin, int Cout, const vx_config& cfg) {
  if (!conv3d_channels_ok(Cin, Cout)) return 0;
  const ConvCfg c = conv_config(Cin, Cout, cfg);
  if (c.S16) return conv3d_s16_head_fusable(Cin, Cout) ? 1 : 0;   // x-pair split-fp16 kernels: halves in lanes l, l ^ 16
  return c.C8;   // the 4x4x1 kernel keeps all channels of a voxel in one lane
}
// in_mean on a dense input in the split-fp16 tile kernel (its plain layers)
static inline bool conv3d_tile_prologue(int Cin, int Cout, const vx_config& cfg) {
  return conv_config(Cin, Cout, cfg).S16 && conv3d_s16_prologue_ok(Cin, Cout);
}
// in_mean on the skip half of an x-blocked concat input in the tile kernel: the halves are whole 16-channel chunks with
// xblk * Cin / 2 a power of two (the element index of the dropout bits follows from the load offset)
static inline bool conv3d_tile_xblk_prologue(int Cin, int Cout, int xblk) {
  const int csrc = Cin / 2;
  return s16_config(Cin, Cout).CB == 16 && csrc % 16 == 0 && conv3d_pow2((int64_t)xblk * csrc);
}
static inline int conv3d_prologue_ok(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  if (!conv3d_channels_ok(Cin, Cout)) return 0;
  return conv3d_xp8_applies(D, H, W, Cin, Cout, cfg) || conv3d_tile_prologue(Cin, Cout, cfg) ? 1 : 0;
}
static inline int conv3d_skip_prologue_ok(int D, int H, int W, int Cin, int Cout, int xblk, const vx_config& cfg) {
  if (Cin <= 0 || Cout <= 0 || Cin % 16 || Cout % 8 || (xblk != 1 && xblk != 2 && xblk != 4)) return 0;
  if (Cin == 16 && conv3d_xp8_applies(D, H, W, Cin, Cout, cfg)) return 1;      // 16 -> 8 at full resolution: the z-column kernel's prologue
  return conv3d_tile_prologue(Cin, Cout, cfg) && conv3d_tile_xblk_prologue(Cin, Cout, xblk) ? 1 : 0;
}
// up_in: 1 = ConvTranspose3d(16 -> 8) as the up half of the full-resolution 16 -> 8 layer; 2 = the 16-channel z-column kernel evaluates
// ConvTranspose3d(32 -> 16) for ALL 16 of its input channels (`in` is not read; up_w = vx_pack_convT_zc16, up_pitch >= 32)
static inline int conv3d_upfuse_ok(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  if (cfg.s16_no_upfuse) return 0;
  if (Cin == 16 && conv3d_xp8_applies(D, H, W, Cin, Cout, cfg)) return 1;
  return conv3d_zc16_16to16(D, H, W, Cin, Cout, cfg) ? 2 : 0;
}
// pool_out: layout 1 = whole windows (xp8w, 8 -> 8), 2 = the (y, x) half of every window (zc16, 16 -> 16)
static inline int conv3d_pool_layout(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  if (cfg.s16_no_poolfuse) return 0;
  if (Cin == 8 && conv3d_xp8_applies(D, H, W, Cin, Cout, cfg)) return 1;
  return conv3d_zc16_16to16(D, H, W, Cin, Cout, cfg) ? 2 : 0;
}
// in_split (vx_prenorm_split's fp16 pairs) is read by xp8w's staging waves only: the tile kernel's prologue takes the raw tensor
// (in_repeat) -- a caller that pre-splits where this says 0 has overwritten its tensor for nothing
static inline int conv3d_presplit_ok(int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  return Cin == 8 && conv3d_xp8_applies(D, H, W, Cin, Cout, cfg) ? 1 : 0;
}
// in_pool_flags: the tile kernel's prologue on a dense 8-channel input (contr_2_1 of the F = 8 networks).  The code lives only in the
// instances an 8 -> 16 layer of a contract block runs on: 8-channel chunks, plain rows, ONE row tile -- Cout % 32 == 0 takes two row
// tiles per wave and Cout == 8 the x-pair kernels, neither carries it
static inline int conv3d_poolfin_ok(int Cin, int Cout, const vx_config& cfg) {
  if (Cin != 8 || Cout <= 0 || Cout % 8 || Cout % 32 == 0) return 0;
  return conv3d_tile_prologue(Cin, Cout, cfg) ? 1 : 0;
}

// ---- the route ----------------------------------------------------------------------------------------------------------------
constexpr int ROUTE_DECLINED = 1;   // a family's step: not taken, the next family is asked

static inline void route_instance(Conv3dRoute* r, int kernel, int np, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0,
                                  int g = 0, int h = 0, int i = 0) {
  const int p[9] = {a, b, c, d, e, f, g, h, i};
  r->kernel = kernel; r->np = np;
  for (int k = 0; k < 9; ++k) r->p[k] = p[k];
}
static inline void route_tiles(Conv3dRoute* r, const vx_conv3d_args& a, int txv, int ty, int tz) {
  r->tiles_x = conv3d_tiles_along(a.W, txv); r->tiles_y = conv3d_tiles_along(a.H, ty); r->tiles_z = conv3d_tiles_along(a.D, tz);
  r->mx = vx_magic_raw(r->tiles_x); r->my = vx_magic_raw(r->tiles_y); r->mz = vx_magic_raw(r->tiles_z);
}
// columns of the z-column kernels: 32 x 8 voxels, tz planes per item
static inline void route_columns(Conv3dRoute* r, const vx_conv3d_args& a, int tz, int stat_tiles) {
  r->tiles_x = a.W / 32; r->tiles_y = a.H / 8; r->tiles_z = 1; r->kz = a.D / tz;
  const int cps = r->tiles_x * r->tiles_y;
  r->nitems = (int)((int64_t)a.N * cps);
  r->mcps = vx_magic_raw(cps); r->mx = vx_magic_raw(r->tiles_x);
  r->stat_epc = stat_tiles / cps;
}

// xp8w (conv3d_xp8w.hip): z-column walk with a rolling LDS window on the full-resolution Cout = 8 layers
static inline int route_xp8w(const vx_conv3d_args& a, int stat_tiles, Conv3dRoute* r) {
  const int nch = a.Cin / 8;
  route_columns(r, a, 4 / nch, stat_tiles);
  const int cps = r->tiles_x * r->tiles_y;
  r->rep = (a.in_mean && a.in_repeat > 1 && a.N % a.in_repeat == 0) ? a.in_repeat : 1;
  r->mrep = vx_magic_raw(r->rep);
  if ((int64_t)a.N * cps >= (1ll << 31)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): too many columns");
  if (a.stats_partial && (stat_tiles % cps || a.act != VX_ACT_NONE || (a.drop_mode != VX_DROP_NONE && !a.pool_out) || a.head_out))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): statistics go with a plain epilogue");
  const int pre = a.in_split ? 2 : (a.in_mean ? 1 : 0);
  if (a.in_split && (a.Cin != 8 || a.in_xblk || a.in_pitch != 8 || a.up_in || !a.stats_partial))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): a pre-split input (vx_prenorm_split) goes with a dense 8-channel tensor and the "
               "statistics epilogue (contr_1_2)");
  int epi;
  if (a.stats_partial) epi = a.pool_out ? 4 : 0;
  else if (a.head_out) epi = 2;
  else if (a.drop_mode == VX_DROP_HASH) epi = 1;
  else epi = 3;
  if (epi == 2 && a.act == VX_ACT_LRELU && a.drop_mode == VX_DROP_NONE) epi = 5;        // head without dropout (ensemble members)
  if (epi == 2 && !(a.act == VX_ACT_LRELU && a.drop_mode == VX_DROP_HASH)) return ROUTE_DECLINED;   // other heads: tile kernel
  if (epi == 1 && a.act != VX_ACT_LRELU) return ROUTE_DECLINED;
  // 2: the up-convolution composed into the weights (vx_pack_conv3d_upfused), 1: evaluated per step by the staging waves
  const int up = a.up_in ? (a.up_fused ? 2 : 1) : 0;
  if (a.pool_out && nch != 1) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): the pooled output goes with Cin = 8");
  if (a.out_split) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): out_split is an epilogue of the tile kernel");
  if (a.up_split && !up) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): up_split without up_in");
  if (a.out_f16 && (epi != 1 || a.out_xblk || a.out_coff))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): fp16 output goes with the LeakyReLU + dropout epilogue and a dense output tensor");
  if (a.in_f16 && !(nch == 1 && epi == 2 && pre == 0 && !up && !a.in_xblk))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): fp16 input goes with the dense 8-channel layer that carries the fused head");
  // IN16: bit 0 the fp16 input, bit 1 the opt-in throughput mode (vx_config.storage16 = 2): one fp16 product per fp32 product
  const int in16 = (a.in_f16 ? 1 : 0) | (a.products == 1 ? 2 : 0);
  route_instance(r, CONV3D_XP8W, 6, nch, epi, pre, up, nch == 2 ? 8 : 4, in16);
  if (conv3d_instance_exists(CONV3D_XP8W, r->p, 6)) return VX_OK;
  if (a.products == 1 && !a.in_f16)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): products = 1 exists for the MC-dropout forward's contr_1_2, upscale2 + expand_1_1 and "
               "expand_1_2 + head (nch %d, epilogue %d, prologue %d, up %d)", nch, epi, pre, up);
  if (up) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): no fused up-convolution for this epilogue (act=%d, drop_mode=%d, statistics=%d)",
                     a.act, a.drop_mode, a.stats_partial ? 1 : 0);
  if (a.pool_out) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(xp8w): no pooled output for this epilogue");
  return ROUTE_DECLINED;
}

// zc16 (conv3d_zc16.hip): the role-split z-column kernel of the Cout = 16 layers below full resolution
static inline int route_zc16(const vx_conv3d_args& a, int stat_tiles, Conv3dRoute* r) {
  if (a.in_xblk || a.head_out || a.in_split || a.in_f16 || a.out_f16 || (a.in_repeat > 1)) return ROUTE_DECLINED;
  if ((a.in_planar || a.out_planar) && (a.drop_mode == VX_DROP_MASK || !a.out || a.in_pitch != a.Cin || a.Cout != 16))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): the planar pre-split hand-over needs hash or no dropout and dense 16-channel tensors");
  if (a.up_in && (a.Cin != 16 || a.in_mean || a.stats_partial || a.up_pitch < 32 || a.up_pitch % 4 || (a.up_fused && (!a.acc_in || a.out_xblk || a.out_split))))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): the fused up-convolution (32 coarse channels -> the conv's 16 input channels) goes with an "
               "activation epilogue, no prologue, up_pitch >= 32 (got %d), up_w packed by vx_pack_convT_zc16; composed weights "
               "(up_fused: vx_pack_conv3d_upfused_zc16) only together with partial sums (acc_in) and a dense float or planar output", a.up_pitch);
  if (a.drop_mode == VX_DROP_MASK || !a.out) return ROUTE_DECLINED;
  route_columns(r, a, 2, stat_tiles);
  const int cps = r->tiles_x * r->tiles_y;
  if ((int64_t)a.N * cps >= (1ll << 31)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): too many columns");
  if (a.in_pitch != a.Cin) return ROUTE_DECLINED;
  if (a.stats_partial && (stat_tiles % cps || a.act != VX_ACT_NONE || (a.drop_mode != VX_DROP_NONE && !a.pool_out)))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): statistics go with a plain epilogue");
  if (a.pool_out && (!a.stats_partial || a.Cin != 16)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): the pooled output goes with statistics, 16 -> 16");
  int pre = 0;
  if (a.in_pool_flags) pre = 3;
  else if (a.in_mean) pre = 1;
  if ((pre == 1 && a.Cin != 16) || (pre == 3 && a.Cin != 8)) return ROUTE_DECLINED;
  if (a.in_planar) {
    if (a.Cin != 16 || pre != 0 || a.up_in || a.acc_in || a.stats_partial || !vx_aligned16(a.in) ||
        (vx_wide)a.D * a.H * a.W * 64 >= CONV3D_2GIB)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): a planar pre-split input (in_planar) goes with 16 -> 16, an activation epilogue, no "
                 "prologue / up-convolution / partial sums, a 16-byte aligned tensor, one sample below 2 GiB");
    pre = 4;
  }
  if (a.out_planar && (a.stats_partial || a.out_pitch != 16 || a.out_coff != 0 || a.out_xblk || a.out_split || a.out == a.acc_in ||
                       (vx_wide)a.D * a.H * a.W * 64 >= CONV3D_2GIB))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): a planar pre-split output (out_planar) goes with an activation epilogue into a dense "
               "16-channel tensor that is not the partial sums' (another layout), one sample below 2 GiB");
  int epi;
  if (a.stats_partial) epi = a.pool_out ? 4 : 0;
  else if (a.drop_mode == VX_DROP_HASH) { if (a.act != VX_ACT_LRELU) return ROUTE_DECLINED; epi = 1; }
  else epi = 3;
  if (a.out_split && a.stats_partial) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): out_split goes with the activation epilogues");
  if (a.out_planar) {
    // the instances that exist: the decoder's up-half launch (partial sums + fused up-convolution) and the plain 16 -> 16 layer
    if (a.Cin != 16 || pre != 0 || (epi != 1 && epi != 3) || ((a.acc_in != nullptr) != (a.up_in != nullptr)))
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): out_planar goes with 16 -> 16, an activation epilogue, no prologue, and either partial "
                 "sums + the fused up-convolution together or neither");
    epi = epi == 1 ? 5 : 6;
  }
  if (a.acc_in && (a.Cin != 16 || pre != 0 || a.stats_partial || a.acc_pitch < 16 || a.acc_pitch % 4 || !vx_aligned16(a.acc_in) ||
                   (vx_wide)a.D * a.H * a.W * a.acc_pitch * 4 >= CONV3D_2GIB))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): partial sums (acc_in) go with 16 -> 16, no prologue, an activation epilogue, a "
               "16-byte aligned tensor of pitch >= 16 (pitch %d), one sample below 2 GiB", a.acc_pitch);
  route_instance(r, CONV3D_ZC16, 5, a.Cin, epi, pre, a.acc_in ? 1 : 0, a.up_in ? 1 : 0);
  if (conv3d_instance_exists(CONV3D_ZC16, r->p, 5)) return VX_OK;
  if (a.up_in && !a.acc_in) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(zc16): no fused up-convolution for this epilogue");
  return ROUTE_DECLINED;
}

// deep (conv3d_deep.hip): the role-split tile kernel of the deep layers (Cout % 32 == 0 on volumes of 32^3 and below)
static inline int route_deep(const vx_conv3d_args& a, int stat_tiles, Conv3dRoute* r) {
  if (a.head_out || a.in_split || a.in_f16 || a.out_f16 || (a.in_repeat > 1) || a.out_xblk || a.up_in || a.pool_out ||
      a.in_pool_flags || a.acc_in)
    return ROUTE_DECLINED;
  if (a.drop_mode == VX_DROP_MASK || !a.out) return ROUTE_DECLINED;
  DeepGeo g;
  const int R = deep_pick(a.D, a.H, a.W, &g);
  if (!R) return ROUTE_DECLINED;
  if (a.in_xblk) {
    const int csrc = a.Cin / 2;
    if (a.in_mean || csrc % 8 || a.W % a.in_xblk) return ROUTE_DECLINED;
  } else if (a.in_pitch % 4) {
    return ROUTE_DECLINED;
  }
  if (a.in_mean && (a.in_pitch != a.Cin || g.ts != 1)) return ROUTE_DECLINED;
  if (a.stats_partial && g.ts != 1) return ROUTE_DECLINED;
  r->tx = g.tx; r->ty = g.ty; r->tz = g.tz; r->ts = g.ts; r->npos = g.npos;
  r->tiles_x = g.tiles_x; r->tiles_y = g.tiles_y; r->tiles_z = g.tiles_z;
  r->nchunks = a.Cin / 8;
  r->ncg = a.Cout / 32;
  const int tps = g.tiles_x * g.tiles_y * g.tiles_z;
  const int64_t npairs = (((int64_t)a.N + g.ts - 1) / g.ts) * tps * r->ncg;
  if (npairs >= (1ll << 31)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(deep): too many tiles");
  r->nitems = (int)npairs;
  r->m_cg = vx_magic_raw(r->ncg); r->mx = vx_magic_raw(g.tiles_x); r->my = vx_magic_raw(g.tiles_y); r->mz = vx_magic_raw(g.tiles_z);
  r->stat_epc = 0;
  r->stat_parts = 1;
  r->tail_cap = 4;
  if (a.stats_partial) {
    // the caller's partials buffer holds stat_tiles entries per sample (the tile kernel's count): this kernel's tiles must divide it,
    // else the tile kernel takes the launch (D % 4 == 2 volumes give 3 tiles against 4 entries)
    if (stat_tiles % tps) return ROUTE_DECLINED;
    if (a.act != VX_ACT_NONE || a.drop_mode != VX_DROP_NONE) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(deep): statistics go with a plain epilogue");
    r->stat_epc = stat_tiles / tps;
    r->tail_cap = r->stat_parts = deep_stat_parts(r->stat_epc);
  }
  if ((vx_wide)g.ts * a.D * a.H * a.W * a.out_pitch * 4 >= CONV3D_2GIB)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(deep): one tile's samples must stay below 2 GiB");
  int epi;
  if (a.stats_partial) epi = 0;
  else if (a.drop_mode == VX_DROP_HASH) { if (a.act != VX_ACT_LRELU) return ROUTE_DECLINED; epi = 1; }
  else epi = 3;
  if (a.out_split && a.stats_partial) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(deep): out_split goes with the activation epilogues");
  route_instance(r, CONV3D_DEEP, 3, R, epi, a.in_mean ? 1 : 0);
  return conv3d_instance_exists(CONV3D_DEEP, r->p, 3) ? VX_OK : ROUTE_DECLINED;
}

// s16 (conv3d_s16.hip): the split-fp16 tile kernel -- takes every launch the kernels above left
static inline int route_s16(const vx_conv3d_args& a, const vx_config& cfg, Conv3dRoute* r) {
  const S16Cfg c = s16_config(a.Cin, a.Cout);
  int txv, ty, tz;
  vx_conv3d_s16_tile(a.H, a.W, a.Cout, &txv, &ty, &tz);
  const int tx = c.XP ? txv / 2 : txv;
  route_tiles(r, a, txv, ty, tz);
  r->nchunks = a.Cin / c.CB;
  r->ty8 = (tx == 16 && ty == 8) ? 1 : 0;
  // EPI, the epilogue fixed at compile time: 0 plain (bias, statistics, store), 1 LeakyReLU + hash dropout, 2 that + the fused head,
  // 3 everything chosen at run time.  s16_generic (parity reference): run-time epilogue, one LDS image, two barriers per item
  const bool generic = cfg.s16_generic != 0;
  int epi = 3;
  if (generic) epi = 3;
  else if (a.act == VX_ACT_NONE && a.drop_mode == VX_DROP_NONE && !a.head_out && a.out) epi = 0;
  else if (a.act == VX_ACT_LRELU && a.drop_mode == VX_DROP_HASH && !a.head_out && a.out) epi = 1;
  else if (a.act == VX_ACT_LRELU && a.drop_mode == VX_DROP_HASH && a.head_out && c.XP) epi = 2;
  // DB: two LDS images, one barrier per item (2: staggered SIMD partners, single-chunk layers; 3: the two-chunk 16 -> 8 layer) where
  // the layer's tile fits twice: x-pair layers on the 16 x 8 x 4 tile, plain single-chunk layers on the 16 x 4 x 4 one (shrinking the
  // tile to make room loses more than the stagger wins)
  int db = 0;
  if (!generic && tx == 16 && c.XP && r->ty8 && r->nchunks <= 2) db = r->nchunks == 1 ? 2 : 3;
  if (!generic && tx == 16 && !c.XP && !r->ty8 && r->nchunks == 1) db = 2;
  // instances that exist per tile: every EPI on the double-buffered x-pair tile (the two-chunk one: 1 and 3), 0 / 1 / 3 on the
  // others, 3 alone on the 4 x 4 x 4 tile
  if (epi == 2 && db != 2) epi = 3;
  if (db == 3 && epi == 0) epi = 3;
  if (tx == 4) epi = 3;
  route_instance(r, CONV3D_S16, 9, c.CB, c.NT, tx, ty, tz, tx == 4 ? 4 : 8, c.XP, db, epi);
  if (!conv3d_instance_exists(CONV3D_S16, r->p, 9)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3(s16): no instance for this tile");   // (not reached)
  return VX_OK;
}

// Every argument check of vx_conv3d_k3, then the families in order.  Returns VX_OK with *r filled, or the VX_E_* code of the refusal
// with its message in r->err.
static inline int conv3d_route(const vx_conv3d_args& a, const vx_config& cfg, Conv3dRoute* r) {
  r->err[0] = 0;
  r->w_off = 0;
  if (!a.in || !a.w_packed || !a.bias || (!a.out && !a.head_out)) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: null tensor pointer");
  const ConvCfg c = conv_config(a.Cin, a.Cout, cfg);
  if (a.head_out) {
    if (!a.head_w || !a.head_b) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: fused head without weights");
    if (a.head_C < 1 || a.head_C > 8) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: fused head takes 1..8 classes, got %d", a.head_C);
    if (c.S16 && a.head_C > S16_HEAD_MAXC)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: the split-fp16 kernel fuses heads of up to 4 classes, got %d", a.head_C);
    if (!conv3d_head_fusable(a.Cin, a.Cout, cfg))
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: no fused head for Cin=%d Cout=%d (see vx_conv3d_k3_head_fusable)", a.Cin, a.Cout);
    if (a.stats_partial) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: fused head on a layer with InstanceNorm statistics");
  }
  if (!conv3d_channels_ok(a.Cin, a.Cout))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: Cin=%d Cout=%d must be positive multiples of 8", a.Cin, a.Cout);
  if (a.N <= 0 || a.D <= 0 || a.H <= 0 || a.W <= 0) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: empty tensor");
  if (a.w_family != conv3d_family(a.Cin, a.Cout, cfg))
    VX_REFUSE(r, VX_E_DTYPE, "vx_conv3d_k3: weights packed for kernel family %d, the library is configured for family %d "
               "(vx_conv3d_k3_family(%d, %d)): re-pack them", a.w_family, conv3d_family(a.Cin, a.Cout, cfg), a.Cin, a.Cout);
  if (a.out_xblk && ((a.out_xblk != 1 && a.out_xblk != 2 && a.out_xblk != 4) || a.W % a.out_xblk || (a.out_half != 0 && a.out_half != 1)))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: bad concat output (xblk=%d, half=%d, W=%d)", a.out_xblk, a.out_half, a.W);
  if ((a.in_mean == nullptr) != (a.in_rstd == nullptr)) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: in_mean / in_rstd must come together");
  // products: 0 / 3 = the split scheme's three products (default); 1 = the opt-in one-product mode of the full-resolution z-column kernel
  if (a.products != 0 && a.products != 1 && a.products != 3)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: products = %d (0 / 3: the default split scheme, 1: one fp16 product)", a.products);
  const bool xp8 = c.S16 && conv3d_xp8_applies(a.D, a.H, a.W, a.Cin, a.Cout, cfg) && a.drop_mode != VX_DROP_MASK;
  if (a.products == 1 && !(xp8 && a.in_drop_mode != VX_DROP_MASK))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: products = 1 is taken by the full-resolution z-column kernel only (got %dx%dx%d, %d -> %d)",
               a.D, a.H, a.W, a.Cin, a.Cout);
  // the planar hand-over only exists in the 16 -> 16 instances of the z-column kernel: refused before any other kernel can take
  // the launch and ignore the flags
  if ((a.in_planar || a.out_planar) && !conv3d_zc16_16to16(a.D, a.H, a.W, a.Cin, a.Cout, cfg))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: the planar pre-split hand-over (in_planar / out_planar) is taken where vx_conv3d_k3_planar_ok "
               "(got %dx%dx%d, %d -> %d)", a.D, a.H, a.W, a.Cin, a.Cout);
  if (a.up_in) {
    if (!a.up_w || !a.up_b) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: fused up-convolution without weights");
    if (!conv3d_upfuse_ok(a.D, a.H, a.W, a.Cin, a.Cout, cfg) || a.drop_mode == VX_DROP_MASK || a.stats_partial || a.head_out)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: no fused up-convolution for this layer (see vx_conv3d_k3_upfuse_ok; hash or no "
                 "dropout, no statistics, no head): %dx%dx%d, %d -> %d", a.D, a.H, a.W, a.Cin, a.Cout);
    if (a.up_pitch < 16 || a.up_pitch % 4 || !vx_aligned16(a.up_in) || !vx_aligned16(a.up_b))
      VX_REFUSE(r, VX_E_ALIGN, "vx_conv3d_k3: up_in pitch %d (>= 16, multiple of 4 floats) / alignment", a.up_pitch);
    if ((vx_wide)(a.D / 2 + 2) * (a.H / 2) * (a.W / 2) * a.up_pitch * 4 >= CONV3D_2GIB)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: one coarse sample must stay below 2 GiB");
    if (a.up_fused && !vx_aligned16(a.up_fused)) VX_REFUSE(r, VX_E_ALIGN, "vx_conv3d_k3: up_fused alignment");
  } else if (a.up_fused) {
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: up_fused (composed up-convolution weights) without up_in");
  }
  if (a.pool_out) {
    if (!a.pool_flags || !a.stats_partial) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: pool_out goes with pool_flags and stats_partial");
    if (!conv3d_pool_layout(a.D, a.H, a.W, a.Cin, a.Cout, cfg) || a.drop_mode == VX_DROP_MASK || a.act != VX_ACT_NONE || a.head_out)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: no pooled output for this layer (see vx_conv3d_k3_poolfuse_ok; hash or no dropout, "
                 "no activation): %dx%dx%d, %d -> %d", a.D, a.H, a.W, a.Cin, a.Cout);
    if (!vx_aligned16(a.pool_out)) VX_REFUSE(r, VX_E_ALIGN, "vx_conv3d_k3: pool_out alignment");
  }
  if (a.in_drop_mode != VX_DROP_NONE && a.in_drop_mode != VX_DROP_HASH) VX_REFUSE(r, VX_E_DTYPE, "vx_conv3d_k3: in_drop_mode %d", a.in_drop_mode);
  if (a.in_pool_flags) {
    if (!a.in_mean) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: in_pool_flags goes with in_mean / in_rstd");
    if (!conv3d_poolfin_ok(a.Cin, a.Cout, cfg) || a.in_xblk || a.in_pitch != 8 || a.in_split || a.up_in || a.in_repeat > 1)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: pool-finish on load takes a dense 8-channel tensor of window maxima (see "
                 "vx_conv3d_k3_poolfin_ok): %d -> %d, pitch %d", a.Cin, a.Cout, a.in_pitch);
    // the first conv of a contract block: bias + statistics (an InstanceNorm follows) -- the only epilogue whose instances carry
    // the pool-finish code; with an activation / dropout / head the launch would fall onto an instance that ignores the flag words
    if (a.act != VX_ACT_NONE || a.drop_mode != VX_DROP_NONE || a.head_out || !a.out)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: pool-finish on load goes with the plain epilogue (no activation, no dropout, no head): "
                 "act=%d drop_mode=%d", a.act, a.drop_mode);
  }
  if (a.out && !a.out_xblk && (a.out_pitch < (int64_t)a.out_coff + a.Cout || a.out_pitch % 4 || a.out_coff % 4))
    VX_REFUSE(r, VX_E_ALIGN, "vx_conv3d_k3: output pitch/offset must be multiples of 4 floats and cover the channels");
  if (a.in_xblk) {
    if (a.in_xblk != 1 && a.in_xblk != 2 && a.in_xblk != 4) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: in_xblk must be 0, 1, 2 or 4");
    if (a.W % a.in_xblk) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: W=%d not a multiple of in_xblk=%d", a.W, a.in_xblk);
    if (a.Cin % 16) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: concat input needs Cin %% 16 == 0 (two halves of Cin/2)");
  } else if (a.in_pitch < (a.up_in ? a.Cin / 2 : a.Cin) || a.in_pitch % 4) {
    VX_REFUSE(r, VX_E_ALIGN, "vx_conv3d_k3: input pitch must be a multiple of 4 floats and cover the channels");
  }
  if (!vx_aligned16(a.in) || !vx_aligned16(a.out) || !vx_aligned16(a.w_packed) || !vx_aligned16(a.bias))
    VX_REFUSE(r, VX_E_ALIGN, "vx_conv3d_k3: pointers must be 16-byte aligned");
  if (a.act < 0 || a.act > 2 || a.drop_mode < 0 || a.drop_mode > 2) VX_REFUSE(r, VX_E_DTYPE, "vx_conv3d_k3: bad act/drop enum");
  if (a.drop_mode == VX_DROP_MASK && !a.drop_mask) VX_REFUSE(r, VX_E_NULL, "vx_conv3d_k3: VX_DROP_MASK without mask");
  const int64_t inrow = a.in_xblk ? (int64_t)a.Cin : (int64_t)a.in_pitch;
  if ((vx_wide)a.D * a.H * a.W * a.out_pitch * 4 >= CONV3D_2GIB || ((vx_wide)a.D + 2) * a.H * a.W * inrow * 4 >= CONV3D_2GIB)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: one sample must stay below 2 GiB (32-bit buffer offsets)");

  // ---- the families, in order ----
  const TileCfg t = tile_config(a.W, c.XP);
  if (c.C8 && !a.in_mean && !a.out_xblk) {   // the 4x4x1 matrix instruction on the x-pair kernel's tile (the same tile count for both)
    route_tiles(r, a, t.TXV, t.TY, t.TZ);
    route_instance(r, CONV3D_C8, 4, a.Cin / 8, t.TXV, t.TY, t.TZ);
    return VX_OK;
  }
  const int stat_tiles = conv3d_tiles_for(a.D, a.H, a.W, a.Cout, cfg);
  r->w_off = conv3d_s16_packed_floats(a.Cin, a.Cout);   // the role-split kernels' weights follow the tile kernel's (families 6 / 7)
  if (xp8) {
    r->w_off = 0;
    const int rc = route_xp8w(a, stat_tiles, r);
    if (rc != ROUTE_DECLINED) return rc;
    if (a.products == 1) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: products = 1, but the z-column kernel does not take this launch");
  }
  if (c.S16 && conv3d_zc16_applies(a.D, a.H, a.W, a.Cin, a.Cout, cfg)) {
    const int rc = route_zc16(a, stat_tiles, r);
    if (rc != ROUTE_DECLINED) return rc;
  }
  if (a.in_planar || a.out_planar)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: the z-column kernel does not take this planar launch (%dx%dx%d, %d -> %d)", a.D, a.H, a.W,
               a.Cin, a.Cout);
  if (c.S16 && conv3d_deep_applies(a.D, a.H, a.W, a.Cin, a.Cout, cfg)) {
    const int rc = route_deep(a, stat_tiles, r);
    if (rc != ROUTE_DECLINED) return rc;
  }
  // the tile kernels: what they do not carry is refused here, once
  r->w_off = 0;
  const bool xblk_pre = a.in_xblk && conv3d_tile_xblk_prologue(a.Cin, a.Cout, a.in_xblk) && !a.in_pool_flags && !(a.in_repeat > 1);
  const bool tile_pre = a.in_mean && conv3d_tile_prologue(a.Cin, a.Cout, cfg) && ((!a.in_xblk && a.in_pitch == a.Cin) || xblk_pre);
  if ((a.in_mean && !tile_pre) || a.out_xblk || a.up_in || a.pool_out || a.in_split || a.in_f16 || a.out_f16)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: the input prologue / concat output / fused up-convolution are only available where "
               "vx_conv3d_k3_prologue_ok(D, H, W, Cin, Cout), with hash or no dropout (got %dx%dx%d, %d -> %d)", a.D, a.H, a.W, a.Cin, a.Cout);
  if (a.up_split) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: up_split goes with the fused up-convolution (up_in)");
  if (a.acc_in) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: partial sums (acc_in) are taken where vx_conv3d_k3_acc_ok (got %dx%dx%d, %d -> %d)",
                           a.D, a.H, a.W, a.Cin, a.Cout);
  if (c.S16) return route_s16(a, cfg, r);
  if (a.out_split) VX_REFUSE(r, VX_E_SHAPE, "vx_conv3d_k3: out_split is an epilogue of the split-fp16 tile kernel");
  route_tiles(r, a, t.TXV, t.TY, t.TZ);
  r->nchunks = a.Cin / c.CB;
  route_instance(r, CONV3D_MFMA, 7, c.CB, c.NT, t.TX, t.TY, t.TZ, t.TX == 4 ? 4 : 8, c.XP);
  return VX_OK;
}

// the instance's name as rocprofv3 prints it (vx_last_kernel_name); returns the length snprintf reports
static inline int conv3d_route_name(const Conv3dRoute& r, char* buf, int cap) {
  static const char* const base[CONV3D_NKERNELS] = {"conv3d_k3_mfma_kernel", "conv3d_k3_c8_kernel", "conv3d_k3_s16_kernel",
                                                    "conv3d_xp8w_kernel",    "conv3d_zc16_kernel",  "conv3d_deep_kernel"};
  char par[64];
  int n = 0;
  for (int i = 0; i < r.np && n < (int)sizeof(par); ++i) n += snprintf(par + n, sizeof(par) - n, i ? ",%d" : "%d", r.p[i]);
  return snprintf(buf, cap > 0 ? cap : 0, "%s<%s>", base[r.kernel], par);
}
