// Routing of vx_conv2d: which kernel family and which instance runs a 2D layer, and with what launch geometry.
// Host only: a pure function of (vx_conv2d_args, vx_config) -- nothing from HIP, compiles with plain g++ (tests/conv2d_route_host.cpp
// walks it under ASan / UBSan).  vx_conv2d is: conv2d_route(), then the family's launcher with the descriptor.
//
//   channel / tile rules    c2_config, c2s_config, conv2d_s16_octets, conv2d_rows_padded, the family numbering (3, 10 + NT, + 100 OCT),
//                           the packed sizes of both schedules and the tile count -- each stated once, here
//   per-instance constants  c2_geo() / c2s_geo(): K steps, halo / plane / image sizes, prologue and epilogue tables, one chunk's
//                           weight bytes and the rest of the LDS -- read by the kernel, the pack launcher, the packed size and the route
//   instance lists          C2_INSTANCES / C2S_INSTANCES: the route asks "does this instance exist?", the family's .hip file
//                           instantiates launch_X<...> from the same list
//   conv2d_route()          every argument check of vx_conv2d in one order, then the instance, the chunks, whether the weights stay
//                           resident, the LDS bytes and the grid
//   conv2d_route_name()     the instance name vx_last_kernel_name() reports (as rocprofv3 prints it)
//
// Adding an instance: one X(...) line in the family's list, plus the rule in conv2d_route() that selects it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/values_amd.h"
#include "host_checks.h"

enum Conv2dKernel { CONV2D_MFMA = 0, CONV2D_S16, CONV2D_NKERNELS };

constexpr int C2_LDS_BYTES = 160 * 1024;   // LDS of one CU
// The CU count the persistent grids are sized by: workgroups per output-channel group = ceil(C2_GRID_CUS x workgroups per CU /
// groups).  A constant, not vx_cu_count(): the grid decides which tiles share a workgroup and with it nothing about the bits, but a
// launch's geometry stays a function of its arguments alone (the dry run needs no device).
constexpr int C2_GRID_CUS = 256;

// ---- instance lists: the template parameters of every instantiated kernel, in the kernel template's order ---------------------
// conv2d_mfma_kernel<KS, S, NT, NSUB, TY>
#define C2_NT3(X, KS, S, NSUB) X(KS, S, 1, NSUB, 16) X(KS, S, 2, NSUB, 16) X(KS, S, 3, NSUB, 16)
#define C2_INSTANCES(X) C2_NT3(X, 3, 1, 1) C2_NT3(X, 3, 2, 1) C2_NT3(X, 1, 1, 4)
// conv2d_s16_kernel<KS, S, NT, NSUB, TY, OCT, EPI>: every schedule with and without the output epilogue (EPI) and with one, two or
// three row tiles; five row tiles on 1x1 layers only (the 3x3 instance needs 256 VGPRs plus scratch).  3x3 schedules: one sub-block
// per item (both strides), two / three sub-blocks per item (stride 1: stride 2 with three does not fit -- 120 KB of parity planes +
// 92 KB of weights), one / three octets (both strides)
#define C2S_NT3(X, KS, S, NSUB, OCT, EPI) X(KS, S, 1, NSUB, 16, OCT, EPI) X(KS, S, 2, NSUB, 16, OCT, EPI) X(KS, S, 3, NSUB, 16, OCT, EPI)
#define C2S_SCHEDULE(X, KS, S, NSUB, OCT) C2S_NT3(X, KS, S, NSUB, OCT, 0) C2S_NT3(X, KS, S, NSUB, OCT, 1)
#define C2S_INSTANCES(X)                                                                                               \
  C2S_SCHEDULE(X, 3, 1, 1, 0) C2S_SCHEDULE(X, 3, 2, 1, 0) C2S_SCHEDULE(X, 3, 1, 2, 0) C2S_SCHEDULE(X, 3, 1, 3, 0)      \
  C2S_SCHEDULE(X, 3, 1, 1, 1) C2S_SCHEDULE(X, 3, 2, 1, 1) C2S_SCHEDULE(X, 3, 1, 1, 3) C2S_SCHEDULE(X, 3, 2, 1, 3)      \
  C2S_SCHEDULE(X, 1, 1, 4, 0) X(1, 1, 5, 4, 16, 0, 0) X(1, 1, 5, 4, 16, 0, 1)

// one integer per instance: the `case` label of the launchers' switches and of conv2d_instance_exists (every parameter < 64)
constexpr uint64_t conv2d_key(int a, int b, int c, int d, int e, int f = 0, int g = 0) {
  return ((((((uint64_t)a * 64 + b) * 64 + c) * 64 + d) * 64 + e) * 64 + f) * 64 + g;
}
static inline uint64_t conv2d_key_of(const int* p) { return conv2d_key(p[0], p[1], p[2], p[3], p[4], p[5], p[6]); }
#define CONV2D_EXISTS_CASE(...) case conv2d_key(__VA_ARGS__):
static inline bool conv2d_instance_exists(int kernel, const int* p) {
  for (int i = 0; i < 7; ++i)
    if (p[i] < 0 || p[i] >= 64) return false;
  const uint64_t key = conv2d_key_of(p);
  switch (kernel) {
    case CONV2D_MFMA: switch (key) { C2_INSTANCES(CONV2D_EXISTS_CASE) return true; default: return false; }
    case CONV2D_S16:  switch (key) { C2S_INSTANCES(CONV2D_EXISTS_CASE) return true; default: return false; }
  }
  return false;
}
// does the split-fp16 family have ANY instance of this kernel size with NT row tiles?  (c2s_config's candidates)
static inline bool c2s_has_row_tiles(int KS, int NT) {
#define C2S_NT_CASE(ks, s, nt, nsub, ty, oct, epi) if (ks == KS && nt == NT) return true;
  C2S_INSTANCES(C2S_NT_CASE)
#undef C2S_NT_CASE
  return false;
}

// ---- per-instance constants ---------------------------------------------------------------------------------------------------
// the 16 (x) x TY (y) output tile's input halo in LDS, both schedules: stride 2 keeps even / odd columns (and rows) in separate
// parity planes, so that a tile's 16 columns stay consecutive positions
struct C2Tile {
  int HX, HY;      // input halo tile
  int NPAR;        // parity planes (stride 2: 4)
  int PXW, PYH;    // positions per parity plane
  int NPP;
  int PLANE;       // positions per (sub-block, channel group) plane, 16-aligned
};
constexpr C2Tile c2_tile(int KS, int S, int TY) {
  C2Tile t{};
  t.HX = 15 * S + KS; t.HY = (TY - 1) * S + KS;
  t.NPAR = S * S;
  t.PXW = (t.HX + S - 1) / S; t.PYH = (t.HY + S - 1) / S;
  t.NPP = t.PXW * t.PYH;
  t.PLANE = ((t.NPAR * t.NPP + 15) / 16) * 16;
  return t;
}
constexpr int C2_RED_FLOATS_PER_NT = 8 * 16 * 2;   // statistics hand-over: [8 waves][NT][16 channels][sum | sum of squares]

// conv2d_mfma_kernel<KS, S, NT, NSUB, TY>
struct C2Geo {
  C2Tile t;
  int IN_FLOATS;   // LDS image
  int W_SUB;       // weight floats per 16-channel sub-block
  int W_FLOATS;    // per item (chunk)
  int lds_bytes;
};
constexpr C2Geo c2_geo(int KS, int S, int NT, int NSUB, int TY) {
  C2Geo g{};
  g.t = c2_tile(KS, S, TY);
  g.IN_FLOATS = NSUB * 4 * g.t.PLANE * 4;
  g.W_SUB = KS * KS * NT * 64 * 4;
  g.W_FLOATS = NSUB * g.W_SUB;
  g.lds_bytes = (g.IN_FLOATS + g.W_FLOATS + NT * C2_RED_FLOATS_PER_NT) * 4;
  return g;
}

// K = 32 steps per item of the split-fp16 schedules.  Octet-granular (3x3 only): four (tap, octet) units of 8 channels per step;
// sub-block 3x3: two taps x one sub-block (9 taps + 1 zero-weight pad = 5 steps per sub-block); 1x1: two sub-blocks per step
constexpr int c2s_nstep(int KS, int NSUB, int OCT) { return OCT ? (9 * OCT + 3) / 4 : (KS == 3 ? 5 * NSUB : NSUB / 2); }

// conv2d_s16_kernel<KS, S, NT, NSUB, TY, OCT, EPI>
struct C2SGeo {
  C2Tile t;
  int NOCTP;           // octet planes of the LDS image
  int IMG_H;           // halves per precision plane (hi + lo planes = 2 IMG_H halves = IMG_H floats)
  int NSTEP;           // K = 32 steps per item
  int TABC;            // channels of the prologue table [scale | shift][TABC]
  int W_STEP;          // weight halves per step
  int W_FLOATS;        // per item (chunk), in floats
  size_t w_bytes;      // one chunk's weights
  size_t rest_bytes;   // image, statistics hand-over, prologue table, epilogue table [scale | shift][NT * 16] (EPI)
};
constexpr C2SGeo c2s_geo(int KS, int S, int NT, int NSUB, int TY, int OCT, bool EPI) {
  C2SGeo g{};
  g.t = c2_tile(KS, S, TY);
  g.NOCTP = OCT ? OCT : 2 * NSUB;
  g.IMG_H = g.NOCTP * g.t.PLANE * 8;
  g.NSTEP = c2s_nstep(KS, NSUB, OCT);
  g.TABC = OCT ? ((OCT * 8 + 15) / 16) * 16 : NSUB * 16;
  g.W_STEP = NT * 2 * 64 * 8;
  g.W_FLOATS = g.NSTEP * g.W_STEP / 2;
  g.w_bytes = (size_t)g.W_FLOATS * 4;
  g.rest_bytes = (size_t)g.IMG_H * 4 + (size_t)NT * C2_RED_FLOATS_PER_NT * 4 + (size_t)2 * g.TABC * 4 + (EPI ? (size_t)2 * NT * 16 * 4 : 0);
  return g;
}

// ---- the descriptor conv2d_route() fills ----------------------------------------------------------------------------------------
struct Conv2dRoute {
  int kernel;                    // Conv2dKernel
  int p[7];                      // the instance's template parameters (lists above; fp32: the first five)
  int OH, OW, tiles_x, tiles_y;  // output size; 16 x TY tiles per image
  unsigned mx, my;               // multiply-high magics floor(2^32 / tiles_*) + 1: exact t / tiles_* for t * tiles_* < 2^32
  int nchunks;                   // work items per tile: input chunks of NSUB sub-blocks (one where the item holds all of Cin)
  int w_all;                     // every chunk's weights stay in LDS for the kernel's life (several chunks, and they fit)
  int lds_bytes;
  int grid_x, grid_y;            // persistent workgroups per output-channel group; groups of NT row tiles
  char err[400];                 // the refusal's message (vx_last_error_string) when conv2d_route returns < 0
};

// the 32-bit offset guards: bytes of an image, as a product no argument can overflow
constexpr int64_t CONV2D_2GIB = 1ll << 31;

// ---- channel and tile rules ---------------------------------------------------------------------------------------------------
static inline bool conv2d_split16(const vx_config& cfg) { return cfg.conv_fp32 == 0; }
static inline bool conv2d_layer_ok(int Cin, int Cout, int KS) { return Cin > 0 && Cout > 0 && (KS == 1 || KS == 3); }

struct C2Cfg { int NT, NSUB, TY; };
// native fp32 (conv2d_mfma.hip)
static inline C2Cfg c2_config(int KS, int Cout) {
  C2Cfg c;
  c.NT = (Cout % 48 == 0) ? 3 : ((Cout % 32 == 0) ? 2 : 1);
  c.NSUB = KS == 1 ? 4 : 1;
  c.TY = 16;
  return c;
}
// split-fp16 (conv2d_s16.hip)
static inline C2Cfg c2s_config(int KS, int Cout) {
  C2Cfg c;
  // row tiles (16 output channels each) per workgroup: every workgroup of a row group stages the SAME input tile and
  // reads the same image fragments, so fewer groups are better as long as the padding they need (rows beyond Cout hold
  // zero weights and are not stored) costs less: minimise groups x (staging + tiles) with the staging of a 1x1 layer
  // weighing ~3 tiles of products and that of a 3x3 layer ~0.7.  HRNet-W18: 18 -> 2 tiles, 36 -> 3, 72 -> 5, 144 -> 3 x 3,
  // the 270 -> 270 head conv 4 groups of 5 (it ran as 17 groups of one tile: 4.8 ms of a 43 ms step); W48: 48 / 96 /
  // 192 / 384 -> 3 tiles, the 720 -> 720 head conv 9 x 5.  The candidates are the tile counts the instance list holds for
  // this kernel size (five tiles: 1x1 layers only).
  const int r16 = (int)(((int64_t)Cout + 15) / 16);
  const float cs = KS == 1 ? 3.0f : 0.7f;
  float bestc = 1e30f;
  c.NT = 1;
  for (int nt : {1, 2, 3, 5}) {
    if (!c2s_has_row_tiles(KS, nt)) continue;
    const float cost = (float)((r16 + nt - 1) / nt) * (cs + (float)nt);
    if (cost < bestc) { bestc = cost; c.NT = nt; }   // ties: the smaller tile count (less padding)
  }
  c.NSUB = KS == 1 ? 4 : 1;
  c.TY = 16;
  return c;
}
// octets of the octet-granular K schedule (conv2d_s16_kernel's OCT) a 3x3 layer of Cin REAL input channels is packed for;
// 0 = the sub-block schedule.  1: up to 8 channels (the image: 3 instead of 5 K steps); 3: 17..24 channels (HRNet-W18's
// full-resolution branch: 7 instead of 10).  Two octets are one sub-block (the same 5 steps), 4 and 6 save one step of 10 /
// 15, and five octets (36 channels) would save 3 of 15 but do not fit beside the stride-2 parity planes: not built.
static inline int conv2d_s16_octets(int Cin, int KS, const vx_config& cfg) {
  if (KS != 3 || cfg.c2s_no_oct) return 0;
  if (Cin <= 8) return 1;
  if (Cin > 16 && Cin <= 24) return 3;
  return 0;
}
static inline int64_t conv2d_rows_padded(int Cout, int NT) { return (((int64_t)Cout + 16 * NT - 1) / (16 * NT)) * (16 * NT); }
static inline int conv2d_ygroups(int Cout, int NT) { return (int)(conv2d_rows_padded(Cout, NT) / (16 * NT)); }

// Kernel family = packed layout of a layer under a configuration: 3 native fp32; split-fp16: 10 + row tiles per workgroup (the
// packed layout is [row group][...][row tile]) + 100 x the octets of the octet-granular K schedule when the layer's REAL input
// channel count is packed for it
static inline int conv2d_family(int Cin, int Cout, int KS, const vx_config& cfg) {
  if (!conv2d_layer_ok(Cin, Cout, KS)) return 0;
  if (!conv2d_split16(cfg)) return 3;
  return 10 + c2s_config(KS, Cout).NT + 100 * conv2d_s16_octets(Cin, KS, cfg);
}

// ---- packed weights -----------------------------------------------------------------------------------------------------------
// a packed size as a product no layer can overflow: -1 (no such layer) beyond int64
static inline int64_t conv2d_floats(vx_wide v) { return v > (vx_wide)INT64_MAX ? -1 : (int64_t)v; }
// split-fp16: [row group][chunk][step][row tile][hi | lo][lane][8 halves] for a layer of Cin REAL input channels
struct C2SPack { int NT, NSUB, OCT, nchunks, nstep; int64_t floats; };
static inline C2SPack conv2d_s16_pack(int Cin, int Cout, int KS, const vx_config& cfg) {
  const C2Cfg c = c2s_config(KS, Cout);
  C2SPack k;
  k.NT = c.NT; k.NSUB = c.NSUB;
  k.OCT = conv2d_s16_octets(Cin, KS, cfg);
  const int nsub_all = (int)(((int64_t)Cin + 15) / 16);
  k.nchunks = k.OCT ? 1 : (nsub_all + c.NSUB - 1) / c.NSUB;
  k.nstep = c2s_nstep(KS, c.NSUB, k.OCT);
  k.floats = conv2d_floats((vx_wide)conv2d_ygroups(Cout, c.NT) * k.nchunks * k.nstep * c.NT * 2 * 64 * 8 / 2);
  return k;
}
// native fp32: [row group][sub-block][tap][row tile][lane][4 floats]
static inline int64_t conv2d_cin_padded(int Cin) { return (((int64_t)Cin + 15) / 16) * 16; }
static inline int64_t conv2d_packed_floats(int Cin, int Cout, int KS, const vx_config& cfg) {
  if (!conv2d_layer_ok(Cin, Cout, KS)) return -1;
  if (conv2d_split16(cfg)) return conv2d_s16_pack(Cin, Cout, KS, cfg).floats;
  return conv2d_floats((vx_wide)conv2d_rows_padded(Cout, c2_config(KS, Cout).NT) * conv2d_cin_padded(Cin) * KS * KS);
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------
static inline int conv2d_out_size(int n, int KS, int S) { return (int)(((int64_t)n + 2 * (KS / 2) - KS) / S + 1); }
// tiles per image (16 x 16 outputs; both schedules): what a caller sizes stats_partial by.  0 for a stride that is none
// (wraps like int for images no launch takes)
static inline int conv2d_tiles(int H, int W, int KS, int S) {
  if (S == 0) return 0;
  const int OH = conv2d_out_size(H, KS, S), OW = conv2d_out_size(W, KS, S), TY = 16;
  return (int)((unsigned)(((int64_t)OW + 15) / 16) * (unsigned)(((int64_t)OH + TY - 1) / TY));
}

// ---- the route ----------------------------------------------------------------------------------------------------------------

// Every argument check of vx_conv2d, then the instance and its launch geometry.  Returns VX_OK with *r filled, or the VX_E_* code
// of the refusal with its message in r->err.
static inline int conv2d_route(const vx_conv2d_args& a, const vx_config& cfg, Conv2dRoute* r) {
  r->err[0] = 0;
  const bool split16 = conv2d_split16(cfg);
  if (!a.in || !a.w_packed || !a.out) VX_REFUSE(r, VX_E_NULL, "vx_conv2d: null tensor pointer");
  if (a.N <= 0 || a.H <= 0 || a.W <= 0) VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: empty tensor");
  if (a.Cin <= 0 || a.Cin % 16 || a.Cout <= 0)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: Cin=%d must be a positive multiple of 16 (pad the input), Cout=%d positive", a.Cin, a.Cout);
  if ((a.KS != 1 && a.KS != 3) || (a.S != 1 && a.S != 2) || (a.KS == 1 && a.S != 1))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: kernel %d stride %d unsupported (3x3 s1/s2, 1x1 s1)", a.KS, a.S);
  // a.Cin is the PADDED channel count; weights packed for the octet-granular schedule carry their octet count in the
  // family (the real count was 8 oct - 7 .. 8 oct): accepted when it pads to this Cin
  const int fam = conv2d_family(a.Cin, a.Cout, a.KS, cfg), oct = a.w_family / 100;
  {
    const bool octet_ok = oct > 0 && split16 && a.KS == 3 && ((int64_t)oct * 8 + 15) / 16 * 16 == a.Cin &&
                          conv2d_s16_octets(oct * 8, a.KS, cfg) == oct && a.w_family % 100 == fam % 100;
    if (a.w_family != fam && !octet_ok)
      VX_REFUSE(r, VX_E_DTYPE, "vx_conv2d: weights packed for kernel family %d, the library is configured for family %d: re-pack them",
                   a.w_family, fam);
  }
  // outputs leave as 16-byte groups of 4 channels: a Cout that is not a multiple of 4 writes its last group up to
  // round4(Cout) (zeros beyond Cout), which the pitch must cover
  const int64_t cout4 = ((int64_t)a.Cout + 3) / 4 * 4;
  if (a.in_pitch <= a.Cin - 16 || a.in_pitch % 4 || a.out_pitch < a.out_coff + cout4 || a.out_pitch % 4 || a.out_coff % 4)
    VX_REFUSE(r, VX_E_ALIGN, "vx_conv2d: pitches/offsets must be multiples of 4 floats and cover the channels");
  if (!vx_aligned16(a.in) || !vx_aligned16(a.out) || !vx_aligned16(a.w_packed) || (a.bias && !vx_aligned16(a.bias)))
    VX_REFUSE(r, VX_E_ALIGN, "vx_conv2d: pointers must be 16-byte aligned");
  r->OH = conv2d_out_size(a.H, a.KS, a.S);
  r->OW = conv2d_out_size(a.W, a.KS, a.S);
  if (((vx_wide)a.H + 2) * a.W * a.in_pitch * 4 >= CONV2D_2GIB || (vx_wide)r->OH * r->OW * a.out_pitch * 4 >= CONV2D_2GIB)
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: one image must stay below 2 GiB");
  if ((a.in_scale == nullptr) != (a.in_shift == nullptr)) VX_REFUSE(r, VX_E_NULL, "vx_conv2d: in_scale / in_shift must come together");
  if (a.in_scale && (a.in_cpitch < a.Cin - 15 || a.in_group_images < 0 || !split16))
    VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: the input prologue needs rows of in_cpitch >= the real channel count and the split-fp16 "
                 "kernels (vx_config.conv_fp32 = 0)");
  // output epilogue (fixed affine + residual + ReLU as the conv stores): refused before any launch where it has no meaning
  if ((a.out_scale == nullptr) != (a.out_shift == nullptr)) VX_REFUSE(r, VX_E_NULL, "vx_conv2d: out_scale / out_shift must come together");
  if (!a.out_scale && a.out_add) VX_REFUSE(r, VX_E_NULL, "vx_conv2d: out_add needs out_scale / out_shift (the output epilogue)");
  if (!a.out_scale && a.out_act != VX_ACT_NONE) VX_REFUSE(r, VX_E_DTYPE, "vx_conv2d: out_act needs out_scale / out_shift (the output epilogue)");
  if (a.out_scale) {
    if (a.stats_partial)
      VX_REFUSE(r, VX_E_DTYPE, "vx_conv2d: out_scale together with stats_partial (batch statistics belong to the raw output, which the "
                   "epilogue does not write)");
    if (!split16)
      VX_REFUSE(r, VX_E_DTYPE, "vx_conv2d: the output epilogue (out_scale) needs the split-fp16 kernels (vx_config.conv_fp32 = 0): run "
                   "the raw conv and vx_affine_gather");
    if (a.out_act != VX_ACT_NONE && a.out_act != VX_ACT_RELU) VX_REFUSE(r, VX_E_DTYPE, "vx_conv2d: out_act must be none or relu");
    if (a.out_add && (a.out_add_pitch % 4 || a.out_add_pitch < cout4))
      VX_REFUSE(r, VX_E_ALIGN, "vx_conv2d: out_add_pitch must be a multiple of 4 floats and cover the channels");
    if (a.out_add && (vx_wide)r->OH * r->OW * a.out_add_pitch * 4 >= CONV2D_2GIB)
      VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: one image of out_add must stay below 2 GiB");
    if (!vx_aligned16(a.out_add)) VX_REFUSE(r, VX_E_ALIGN, "vx_conv2d: out_add must be 16-byte aligned");
  }

  // ---- the instance ----
  const C2Cfg c = split16 ? c2s_config(a.KS, a.Cout) : c2_config(a.KS, a.Cout);
  const int nsub_all = a.Cin / 16;
  r->tiles_x = (int)(((int64_t)r->OW + 15) / 16);
  r->tiles_y = (int)(((int64_t)r->OH + c.TY - 1) / c.TY);
  r->mx = vx_magic_raw(r->tiles_x);
  r->my = vx_magic_raw(r->tiles_y);
  r->nchunks = (nsub_all + c.NSUB - 1) / c.NSUB;
  r->w_all = 0;
  int per_cu_max;
  if (split16) {
    // the octet instance the weights were packed for (the family check above took its octet count); else 3x3 stride-1 layers of
    // 2 / 3 input sub-blocks (HRNet: 18 / 36 / 48 channels) as ONE item per tile with all sub-blocks staged together -- a third /
    // half of the barriers, prefetches and commits, and the weights resident (the packed layout does not change: [chunk][step]
    // with five steps per sub-block is the same sequence either way); else one sub-block (1x1: four) per item
    int nsub = c.NSUB;
    if (oct) r->nchunks = 1;
    else if (a.KS == 3 && a.S == 1 && !cfg.c2s_no_wide && (nsub_all == 2 || nsub_all == 3)) { nsub = nsub_all; r->nchunks = 1; }
    const int p[7] = {a.KS, a.S, c.NT, nsub, c.TY, oct, a.out_scale ? 1 : 0};
    r->kernel = CONV2D_S16;
    for (int i = 0; i < 7; ++i) r->p[i] = p[i];
    if (!conv2d_instance_exists(CONV2D_S16, r->p)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d(s16): no such instance");   // (not reached)
    const C2SGeo g = c2s_geo(a.KS, a.S, c.NT, nsub, c.TY, oct, a.out_scale != nullptr);
    r->w_all = (r->nchunks > 1 && g.rest_bytes + r->nchunks * g.w_bytes <= (size_t)C2_LDS_BYTES) ? 1 : 0;
    r->lds_bytes = (int)(g.rest_bytes + (r->w_all ? r->nchunks : 1) * g.w_bytes);
    per_cu_max = 2;
  } else {
    const int p[7] = {a.KS, a.S, c.NT, c.NSUB, c.TY, 0, 0};
    r->kernel = CONV2D_MFMA;
    for (int i = 0; i < 7; ++i) r->p[i] = p[i];
    if (!conv2d_instance_exists(CONV2D_MFMA, r->p)) VX_REFUSE(r, VX_E_SHAPE, "vx_conv2d: no such instance");         // (not reached)
    r->lds_bytes = c2_geo(a.KS, a.S, c.NT, c.NSUB, c.TY).lds_bytes;
    per_cu_max = 4;
  }
  // ---- the grid: persistent workgroups over a flat list of (tile, chunk) items per output-channel group ----
  const int64_t total_tiles = (int64_t)r->tiles_x * r->tiles_y * a.N;
  r->grid_y = conv2d_ygroups(a.Cout, c.NT);
  int per_cu = C2_LDS_BYTES / r->lds_bytes;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > per_cu_max) per_cu = per_cu_max;
  int gx = (C2_GRID_CUS * per_cu + r->grid_y - 1) / r->grid_y;
  if (gx > total_tiles) gx = (int)total_tiles;
  r->grid_x = gx;
  return VX_OK;
}

// the instance's name as rocprofv3 prints it (vx_last_kernel_name): every template argument, defaulted ones included -- the
// epilogue instances carry a seventh argument, 1; the others keep the six-argument name they always reported.  Returns the length
// snprintf reports
static inline int conv2d_route_name(const Conv2dRoute& r, char* buf, int cap) {
  const int* p = r.p;
  if (cap < 0) cap = 0;
  if (r.kernel == CONV2D_MFMA) return snprintf(buf, cap, "conv2d_mfma_kernel<%d,%d,%d,%d,%d>", p[0], p[1], p[2], p[3], p[4]);
  return snprintf(buf, cap, p[6] ? "conv2d_s16_kernel<%d,%d,%d,%d,%d,%d,1>" : "conv2d_s16_kernel<%d,%d,%d,%d,%d,%d>", p[0], p[1], p[2],
                  p[3], p[4], p[5]);
}
