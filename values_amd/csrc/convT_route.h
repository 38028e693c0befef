// Routing of vx_convT_k2s2: which of the four kernels runs a transposed convolution, which instance, and with what launch geometry.
// Host only: a pure function of (vx_convT_args, vx_config) -- nothing from HIP, compiles with plain g++ (tests/convT_route_host.cpp
// walks it under ASan / UBSan).  vx_convT_k2s2 is: convT_route(), then the family's launcher with the descriptor.
//
//   instance lists        CONVT_MFMA_INSTANCES / CONVT_S16_INSTANCES / CONVT_ROWS_INSTANCES: the route asks "does this instance
//                         exist?", convtranspose.hip generates its launch switches from the same lines
//   rules                 the channel rule, the two bounds of the multiply-high decode, the row-streaming kernel's lane rule, the
//                         grid caps, CT_CO and the packed size -- each stated once, here
//   convT_route()         every argument check of vx_convT_k2s2 in one order, then the family, the instance, the grid and the
//                         decode magics; the bound every int expression of a kernel needs stands next to the rule that sends a
//                         launch to that kernel
//   convT_route_name()    the name vx_last_kernel_name() reports
//
// Adding an instance: one X(...) line in the family's list, plus the channel rule that selects it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/values_amd.h"
#include "host_checks.h"

enum ConvTKernel { CONVT_MFMA = 0, CONVT_S16, CONVT_ROWS, CONVT_GENERIC, CONVT_NKERNELS };

// ---- instance lists: (CIN, RT) of the tile kernels -- each line is the MASK = false / true pair -- and CIN of the rows kernel -----
// convT_k2s2_mfma_kernel<CIN, RT, MASK>: row tiles per workgroup so that the weights stay in <= 128 VGPRs
#define CONVT_MFMA_INSTANCES(X) X(16, 4) X(16, 8) X(32, 4) X(32, 8) X(64, 4) X(64, 8) X(128, 4)
// convT_k2s2_s16_kernel<CIN, RT, MASK>
#define CONVT_S16_INSTANCES(X) X(64, 4) X(128, 2)
// convT_k2s2_rows_kernel<CIN>
#define CONVT_ROWS_INSTANCES(X) X(16) X(32)

// one integer per (CIN, RT): the `case` label of the launch switches and of convT_instance_exists
constexpr int convT_key(int cin, int rt = 0) { return cin * 16 + rt; }
static inline bool convT_instance_exists(int kernel, int cin, int rt, int mask) {
  if (cin < 0 || cin > 128 || rt < 0 || rt >= 16 || (mask != 0 && mask != 1)) return false;
#define CONVT_EXISTS_CASE(...) case convT_key(__VA_ARGS__):
  switch (kernel) {
    case CONVT_MFMA: switch (convT_key(cin, rt)) { CONVT_MFMA_INSTANCES(CONVT_EXISTS_CASE) return true; default: return false; }
    case CONVT_S16:  switch (convT_key(cin, rt)) { CONVT_S16_INSTANCES(CONVT_EXISTS_CASE) return true; default: return false; }
    case CONVT_ROWS: switch (convT_key(cin, rt)) { CONVT_ROWS_INSTANCES(CONVT_EXISTS_CASE) return !mask; default: return false; }
    case CONVT_GENERIC: return cin == 0 && rt == 0 && !mask;     // one kernel, no template parameters
  }
#undef CONVT_EXISTS_CASE
  return false;
}

// ---- rules ------------------------------------------------------------------------------------------------------------------------
constexpr int CT_CO = 8;   // output channels per thread of the generic kernel; the granule of Cout
// The tile kernels decode the flat input voxel v < nvox with three multiply-high divisions by W, H, D (magic 2^32 / d + 1), which
// are exact while v * d < 2^32; they keep v and 16 * (column tile) in an int
constexpr int64_t CONVT_DECODE_NVOX = 1ll << 27;        // nvox = N D H W below this, and
constexpr int64_t CONVT_DECODE_PRODUCT = 1ll << 32;     // nvox * max(D, H, W) below this
// Grid caps.  fp32 tiles: CONVT_GRID_CUS x CONVT_MFMA_PER_CU workgroups in all -- more, shorter address streams write faster (fill:
// 5.1 TB/s at 2048 workgroups, 6.5 at 32768).  Split-fp16 tiles: CONVT_S16_WGS in all (two per CU at these instances' registers),
// each wave walking its share of the column tiles, so that the weight gather of the prologue is paid once per wave.  Measured at
// 320 samples (tools/ab_convT.py): upscale4 0.108 -> 0.056 ms, center.4 0.052 -> 0.033; with one column tile per wave (the fp32
// kernel's grid) the same kernel is 20-30 % SLOWER than the fp32 one, and <64,8> / <128,4> (256 registers, one workgroup per CU)
// reach 0.076 / 0.034.  Constants, not vx_cu_count(): a launch's geometry is a function of its arguments alone
constexpr int CONVT_GRID_CUS = 256, CONVT_MFMA_PER_CU = 32, CONVT_S16_WGS = 512;
constexpr int CONVT_ROWS_MAX_WGS = 4096, CONVT_GENERIC_MAX_WGS = 8192;

static inline bool convT_layer_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 4 == 0 && Cout % CT_CO == 0; }
// packed weights [dz][dy][ci][dx][co]; -1: no such layer (or a size beyond int64)
static inline int64_t convT_packed_floats(int Cin, int Cout) {
  if (!convT_layer_ok(Cin, Cout)) return -1;
  const vx_wide v = (vx_wide)Cin * Cout * 8;
  return v > (vx_wide)INT64_MAX ? -1 : (int64_t)v;
}

// The channel rule of the tile kernels (8 Cout rows = Cout / 2 row tiles of 16; Cout % 8 == 0 is checked before): family and row
// tiles per workgroup, or false.  The deep up-convolutions run on the split-fp16 products under vx_config.conv_fp32 == 0, the
// family the convolutions run in
struct ConvTTiles { int kernel, rt; };
static inline bool convT_tile_rule(int Cin, int Cout, const vx_config& cfg, ConvTTiles* t) {
  const int rt48 = Cout % 16 ? 4 : 8;
  if (Cin == 16 || Cin == 32) { *t = {CONVT_MFMA, rt48}; return true; }
  if (Cin == 64) { *t = cfg.conv_fp32 == 0 ? ConvTTiles{CONVT_S16, 4} : ConvTTiles{CONVT_MFMA, rt48}; return true; }
  if (Cin == 128) { *t = cfg.conv_fp32 == 0 ? ConvTTiles{CONVT_S16, 2} : ConvTTiles{CONVT_MFMA, 4}; return true; }
  return false;
}
// The row-streaming kernel's lane rule: a thread's (dx, channel quad) is fixed by its lane, so the 256 lanes of a workgroup and the
// pieces of an output row must both be multiples of 2 * Cout / 4 -- Cout in {8, 16, 32, 64, 128}
static inline bool convT_rows_rule(int Cin, int Cout) {
  return (Cin == 16 || Cin == 32) && Cout <= 128 && 256 % (Cout / 2) == 0;
}

// ---- the descriptor convT_route() fills -----------------------------------------------------------------------------------------------
struct ConvTRoute {
  int kernel;              // ConvTKernel
  int cin, rt, mask;       // the instance's template parameters (tile kernels: all three; rows: cin; generic: none)
  int grid_x, grid_y;
  int ncoltiles;           // tile kernels: column tiles of 16 input voxels
  int64_t nvox;            // input voxels N D H W
  int64_t total;           // rows kernel: 16-byte pieces of output rows per (dz, dy)
  unsigned mW, mH, mD;     // tile kernels: multiply-high magics of the decode (0: the dimension is 1)
  char err[200];           // the refusal's message (vx_last_error_string) when convT_route returns < 0
};

// Every argument check of vx_convT_k2s2, then the kernel and its launch geometry.  Returns VX_OK with *r filled, or the VX_E_* code
// of the refusal with its message in r->err.
static inline int convT_route(const vx_convT_args& a, const vx_config& cfg, ConvTRoute* r) {
  r->err[0] = 0;
  if (!a.in || !a.w_packed || !a.bias || !a.out) VX_REFUSE(r, VX_E_NULL, "vx_convT_k2s2: null tensor");
  if (!convT_layer_ok(a.Cin, a.Cout)) VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: Cin=%d (mult of 4) Cout=%d (mult of 8)", a.Cin, a.Cout);
  if (a.N <= 0 || a.D <= 0 || a.H <= 0 || a.W <= 0) VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: empty tensor");
  if (a.in_pitch % 4 || a.in_pitch < a.Cin) VX_REFUSE(r, VX_E_ALIGN, "vx_convT_k2s2: input pitch");
  if (a.out_xblk) {
    if ((a.out_xblk != 1 && a.out_xblk != 2 && a.out_xblk != 4) || (2 * (int64_t)a.W) % a.out_xblk || (a.out_half != 0 && a.out_half != 1))
      VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: bad concat layout (xblk=%d, half=%d)", a.out_xblk, a.out_half);
  } else if (a.out_pitch % 4 || a.out_coff % 4 || a.out_pitch < (int64_t)a.out_coff + a.Cout) {
    VX_REFUSE(r, VX_E_ALIGN, "vx_convT_k2s2: pitches/offsets must be multiples of 4 floats");
  }
  if (a.drop_mode == VX_DROP_MASK && !a.drop_mask) VX_REFUSE(r, VX_E_NULL, "vx_convT_k2s2: mask mode without mask");
  // All four kernels: the dropout element index ((oz OH + oy) OW + ox) Cout + co of one sample is a 32-bit word, and the offset
  // inside an interleaved output row, < 4 W Cout, an int.  (What follows from it: D H W < 2^26, so nvox and total fit an int64.)
  if ((vx_wide)a.D * a.H * a.W * 8 * a.Cout >= ((vx_wide)1 << 32)) VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: sample too large");
  r->nvox = (int64_t)a.N * a.D * a.H * a.W;
  r->kernel = -1;
  r->cin = r->rt = r->ncoltiles = 0;
  r->mask = 0;
  r->total = 0;
  r->mW = r->mH = r->mD = 0;

  // ---- tile kernels (matrix cores): v = 16 ct + m and nvox are ints, the decode is exact -- both by the two decode bounds; the
  // sample index n = v / (D H W) goes on as size_t ----
  const int64_t dmax = a.W > a.H ? (a.W > a.D ? a.W : a.D) : (a.H > a.D ? a.H : a.D);
  ConvTTiles t = {-1, 0};
  if (r->nvox < CONVT_DECODE_NVOX && (vx_wide)r->nvox * dmax < CONVT_DECODE_PRODUCT && convT_tile_rule(a.Cin, a.Cout, cfg, &t)) {
    r->kernel = t.kernel; r->cin = a.Cin; r->rt = t.rt;
    r->mask = a.drop_mode == VX_DROP_MASK;
    if (!convT_instance_exists(r->kernel, r->cin, r->rt, r->mask)) VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: no such instance");   // (not reached)
    r->ncoltiles = (int)((r->nvox + 15) / 16);
    r->grid_y = (a.Cout / 2) / t.rt;   // groups of RT row tiles
    const int wgs = t.kernel == CONVT_S16 ? CONVT_S16_WGS : CONVT_GRID_CUS * CONVT_MFMA_PER_CU;
    const int cap = (wgs + r->grid_y - 1) / r->grid_y;
    r->grid_x = (r->ncoltiles + 3) / 4;   // one column tile per wave ...
    if (r->grid_x > cap) r->grid_x = cap; // ... or a grid stride
    r->mW = vx_magic_or0(a.W); r->mH = vx_magic_or0(a.H); r->mD = vx_magic_or0(a.D);
    return VX_OK;
  }
  // ---- rows and generic kernels: flat indices are int64, but the output plane n * 2D + oz (and the input plane n * D + z) is an
  // int before it is widened ----
  if ((int64_t)a.N * 2 * a.D >= (1ll << 31)) VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: N * 2 D must stay below 2^31");
  if (convT_rows_rule(a.Cin, a.Cout)) {
    // large, shallow up-convolutions.  Pieces per output row 2 W Cout / 4 < 2^28 (sample guard): an int
    r->kernel = CONVT_ROWS; r->cin = a.Cin;
    if (!convT_instance_exists(r->kernel, r->cin, 0, 0)) VX_REFUSE(r, VX_E_SHAPE, "vx_convT_k2s2: no such instance");             // (not reached)
    r->total = (int64_t)((vx_wide)r->nvox * 2 * (a.Cout / 4));
    const int64_t bx = (r->total + 255) / 256;
    r->grid_x = bx > CONVT_ROWS_MAX_WGS ? CONVT_ROWS_MAX_WGS : (int)bx;
    r->grid_y = 4;   // (dz, dy)
    return VX_OK;
  }
  r->kernel = CONVT_GENERIC;
  const int64_t bx = (r->nvox + 255) / 256;
  r->grid_x = bx > CONVT_GENERIC_MAX_WGS ? CONVT_GENERIC_MAX_WGS : (int)bx;
  r->grid_y = 4 * (a.Cout / CT_CO);   // (dz, dy) x groups of CT_CO channels
  return VX_OK;
}

// the name vx_last_kernel_name() reports after the launch.  Returns the length snprintf reports
static inline int convT_route_name(const ConvTRoute& r, char* buf, int cap) {
  if (cap < 0) cap = 0;
  const char* m = r.mask ? "true" : "false";
  switch (r.kernel) {
    case CONVT_MFMA: return snprintf(buf, cap, "convT_k2s2_mfma_kernel<%d,%d,%s>", r.cin, r.rt, m);
    case CONVT_S16: return snprintf(buf, cap, "convT_k2s2_s16_kernel<%d,%d,%s>", r.cin, r.rt, m);
    case CONVT_ROWS: return snprintf(buf, cap, "convT_k2s2_rows_kernel");
  }
  return snprintf(buf, cap, "convT_k2s2_kernel");
}
