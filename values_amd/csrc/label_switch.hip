// K44: the raters of the 2D test split (StochasticLabelSwitches.apply_to_mask, augmentations.py:25-40) and the label-switch
// variance map (evaluation/utils/gta.py:15-35) for a whole batch of label maps in ONE launch.
//   An item is a label map [H][W] of 1 / 2 / 4 / 8-byte integers, where the reader left it (element alignment only).  It
//   is cut into tiles of LS_TH rows x LS_TW columns; the tiles of all items are dealt to the workgroups through the items'
//   block0 prefix (the way select.hip deals its work blocks), so a batch of small maps and one large map share one grid.
//   A workgroup
//     1. builds the R 256-entry remap tables of its item in LDS from the item's decisions (given by the host, or drawn
//        here: the first hash word of vx_gauss_words(seed ^ VX_LSWITCH_XOR, r * n_switch + k, item.index) against the
//        row's 24-bit threshold, an integer compare) -- once per item, not per tile;
//     2. loads the tile's labels in aligned 16-byte pieces (lanes along the row: 1 KB per wave and step), narrows them to
//        bytes in an LDS tile (a label outside 0..255 becomes 255 and is counted);
//     3. writes every rater plane in aligned 16-byte pieces, each byte through the rater's table (element stores only in
//        the pieces that hold a row's two ends);
//     4. writes the variance map with ITS axes swapped ([W][H]) from the LDS tile: lanes run along H, so the stores are
//        runs of LS_TH floats while the labels were read along W.
//   A pixel's bytes depend on its item alone (its labels, index and decisions): an item's outputs are equal whether it is
//   submitted alone or in any batch, at any position.  No read outside [labels, labels + H * W elements), no write
//   outside the outputs.  Plain C++ stores; the only atomic is the count of labels outside 0..255.
// The item table and the variance table go up through the pinned staging buffer of staging.h: no wait on the stream, not
// capturable into a hipGraph.
#include <vector>

#include "common.h"
#include "gauss.h"
#include "staging.h"

#define LS_THREADS 256
#define LS_TH 32
#define LS_TW 128
#define LS_PITCH 132   // bytes per tile row in LDS: 33 dwords, so a column of the tile lies in 32 different banks
#define LS_MAX_GRID 2048

struct ls_item {
  const uint8_t* p;   // first label
  uint8_t* refs;      // [R][H * W], or null
  float* var;         // [W][H], or null
  int64_t block0;     // first tile of the item
  int32_t H, W, esl, out;   // esl: log2 of the label's bytes; out: index of the item in the caller's array
  uint32_t index;
  int32_t tiles_x;
  uint8_t dec[32];    // given decisions: bit k of dec[r]
};

struct ls_switch {
  int32_t n, R, drawn;
  uint32_t seed;      // (already seed ^ VX_LSWITCH_XOR)
  uint32_t thr[VX_LSWITCH_MAX_ROWS];
  uint8_t from[VX_LSWITCH_MAX_ROWS], to[VX_LSWITCH_MAX_ROWS];
};

// the last entry whose block0 is not after blk (same for every thread of a workgroup)
__device__ __forceinline__ int ls_find(const ls_item* __restrict__ items, int n, int64_t blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one label of 1 << ESL bytes as (low byte, anything above it set)
template <int ESL>
__device__ __forceinline__ void ls_element(uintptr_t addr, unsigned& lo, bool& high) {
  if constexpr (ESL == 0) { lo = *reinterpret_cast<const uint8_t*>(addr); high = false; }
  if constexpr (ESL == 1) { const unsigned v = *reinterpret_cast<const uint16_t*>(addr); lo = v & 255u; high = v > 255u; }
  if constexpr (ESL == 2) { const unsigned v = *reinterpret_cast<const uint32_t*>(addr); lo = v & 255u; high = v > 255u; }
  if constexpr (ESL == 3) { const unsigned long long v = *reinterpret_cast<const unsigned long long*>(addr); lo = (unsigned)v & 255u; high = v > 255ull; }
}

// step 2: rows x cols labels from (y0, x0) of the map at p into the LDS tile; -> this thread's labels outside 0..255
template <int ESL>
__device__ __forceinline__ unsigned ls_load_tile(const uint8_t* p, int W, int y0, int x0, int rows, int cols, uint8_t* tile, int tid) {
  constexpr int ES = 1 << ESL, PER = 16 >> ESL;
  const int segs = ((cols << ESL) + 15) / 16 + 1;   // aligned 16-byte pieces that can touch one row of the tile
  unsigned bad = 0;
  for (int t = tid; t < rows * segs; t += LS_THREADS) {
    const int row = t / segs, j = t - row * segs;
    const uintptr_t a = (uintptr_t)p + ((((size_t)(y0 + row)) * (size_t)W + (size_t)x0) << ESL);
    const uintptr_t end = a + ((size_t)cols << ESL);
    const uintptr_t s = (a & ~(uintptr_t)15) + ((uintptr_t)j << 4);
    if (s >= end) continue;
    uint8_t* dst = tile + row * LS_PITCH;
    if (s >= a && s + 16 <= end) {
      const uint4 q = *reinterpret_cast<const uint4*>(s);
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
      const int px0 = (int)((s - a) >> ESL);
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        unsigned lo;
        bool high;
        if constexpr (ESL == 0) { lo = (w[e >> 2] >> (8 * (e & 3))) & 255u; high = false; }
        if constexpr (ESL == 1) { const unsigned v = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu; lo = v & 255u; high = v > 255u; }
        if constexpr (ESL == 2) { lo = w[e] & 255u; high = w[e] > 255u; }
        if constexpr (ESL == 3) { lo = w[2 * e] & 255u; high = w[2 * e] > 255u || w[2 * e + 1] != 0u; }
        bad += high ? 1u : 0u;
        dst[px0 + e] = (uint8_t)(high ? 255u : lo);
      }
    } else {   // a piece that holds one of the row's two ends: only the row's own elements are read
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const uintptr_t addr = s + (uintptr_t)(e * ES);
        if (addr >= a && addr < end) {
          unsigned lo;
          bool high;
          ls_element<ESL>(addr, lo, high);
          bad += high ? 1u : 0u;
          dst[(int)((addr - a) >> ESL)] = (uint8_t)(high ? 255u : lo);
        }
      }
    }
  }
  return bad;
}

__global__ __launch_bounds__(LS_THREADS) void label_switch_kernel(const ls_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                                  const float* __restrict__ vtab, const ls_switch sw,
                                                                  int32_t* __restrict__ status) {
  __shared__ uint8_t s_lut[VX_LSWITCH_MAX_R * 256];
  __shared__ uint8_t s_tile[LS_TH * LS_PITCH];
  __shared__ float s_var[256];
  const int tid = threadIdx.x;
  const int R = sw.R;
  s_var[tid] = vtab[tid];   // (LS_THREADS == 256)
  int cur = -1;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int ii = ls_find(items, n_items, blk);
    const ls_item* __restrict__ it = items + ii;
    const uint8_t* p = it->p;
    uint8_t* refs = it->refs;
    float* var = it->var;
    const int H = it->H, W = it->W, tiles_x = it->tiles_x;
    const int64_t tb = blk - it->block0;
    const int y0 = (int)(tb / tiles_x) * LS_TH, x0 = (int)(tb % tiles_x) * LS_TW;
    const int rows = H - y0 < LS_TH ? H - y0 : LS_TH, cols = W - x0 < LS_TW ? W - x0 : LS_TW;
    __syncthreads();   // the previous tile and the previous item's tables have been read (first round: s_var is written)
    if (refs && ii != cur) {   // step 1 (uniform: ii is the same for the workgroup)
      const uint32_t index = it->index;
      for (int t = tid; t < R * 256; t += LS_THREADS) {
        const int r = t >> 8;
        const unsigned v = (unsigned)t & 255u;
        unsigned o = v;
#pragma unroll
        for (int k = 0; k < VX_LSWITCH_MAX_ROWS; ++k) {
          if (k < sw.n && v == sw.from[k]) {
            bool d;
            if (sw.drawn) {
              uint32_t h1, h2;
              vx_gauss_words(sw.seed, (uint32_t)(r * sw.n + k), index, h1, h2);
              d = (h1 >> 8) < sw.thr[k];
            } else {
              d = (it->dec[r] >> k) & 1;
            }
            if (d) o = sw.to[k];
          }
        }
        s_lut[t] = (uint8_t)o;
      }
      cur = ii;
    }
    unsigned bad;
    switch (it->esl) {
      case 0: bad = ls_load_tile<0>(p, W, y0, x0, rows, cols, s_tile, tid); break;
      case 1: bad = ls_load_tile<1>(p, W, y0, x0, rows, cols, s_tile, tid); break;
      case 2: bad = ls_load_tile<2>(p, W, y0, x0, rows, cols, s_tile, tid); break;
      default: bad = ls_load_tile<3>(p, W, y0, x0, rows, cols, s_tile, tid); break;
    }
    __syncthreads();
    if (refs) {   // step 3
      const size_t HW = (size_t)H * (size_t)W;
      const int segs = (cols + 15) / 16 + 1, per_r = rows * segs;
      for (int t = tid; t < R * per_r; t += LS_THREADS) {
        const int r = t / per_r, u = t - r * per_r, row = u / segs, j = u - row * segs;
        const uintptr_t a = (uintptr_t)refs + (size_t)r * HW + (size_t)(y0 + row) * (size_t)W + (size_t)x0;
        const uintptr_t end = a + (uintptr_t)cols;
        const uintptr_t s = (a & ~(uintptr_t)15) + ((uintptr_t)j << 4);
        if (s >= end) continue;
        const uint8_t* lut = s_lut + r * 256;
        const uint8_t* src = s_tile + row * LS_PITCH;
        if (s >= a && s + 16 <= end) {
          const int px0 = (int)(s - a);
          unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
          for (int i = 0; i < 16; ++i) w[i >> 2] |= (unsigned)lut[src[px0 + i]] << (8 * (i & 3));
          *reinterpret_cast<uint4*>(s) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const uintptr_t addr = s + (uintptr_t)i;
            if (addr >= a && addr < end) *reinterpret_cast<uint8_t*>(addr) = lut[src[(int)(addr - a)]];
          }
        }
      }
    }
    if (var) {   // step 4: lanes along y
      for (int t = tid; t < cols * LS_TH; t += LS_THREADS) {
        const int y = t & (LS_TH - 1), x = t / LS_TH;
        if (y < rows) var[(size_t)(x0 + x) * (size_t)H + (size_t)(y0 + y)] = s_var[s_tile[y * LS_PITCH + x]];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if ((tid & 63) == 0 && bad) atomicAdd(&status[it->out], (int)bad);
  }
}

static vx_staging g_ls_stage;

extern "C" int64_t vx_label_switch_batched_workspace_bytes(int n_items, int R) {
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS || R < 1 || R > VX_LSWITCH_MAX_R) return 0;
  return (int64_t)(vx_align256(256 * sizeof(float)) + vx_align256((size_t)n_items * sizeof(ls_item)));
}

extern "C" int vx_label_switch_batched(const vx_lswitch_item* items, int n_items, int R, const vx_lswitch_row* rows, int n_switch,
                                       const uint8_t* decisions, uint32_t seed, const float* var_table, int32_t* status, void* workspace,
                                       int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_label_switch_batched";
  if (!items || !rows) VX_FAIL(VX_E_NULL, "%s: null item or switch table", who);
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) VX_FAIL(VX_E_SHAPE, "%s: n_items %d outside 1..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (R < 1 || R > VX_LSWITCH_MAX_R) VX_FAIL(VX_E_SHAPE, "%s: R %d outside 1..%d", who, R, VX_LSWITCH_MAX_R);
  if (n_switch < 1 || n_switch > VX_LSWITCH_MAX_ROWS) VX_FAIL(VX_E_SHAPE, "%s: n_switch %d outside 1..%d", who, n_switch, VX_LSWITCH_MAX_ROWS);
  ls_switch sw = {};
  sw.n = n_switch; sw.R = R; sw.drawn = decisions ? 0 : 1; sw.seed = seed ^ VX_LSWITCH_XOR;
  for (int k = 0; k < n_switch; ++k) {
    if (rows[k].from < 0 || rows[k].from > 255 || rows[k].to < 0 || rows[k].to > 255)
      VX_FAIL(VX_E_SHAPE, "%s: row %d: %d -> %d is not a pair of uint8 labels", who, k, rows[k].from, rows[k].to);
    if (rows[k].thr > (1u << 24)) VX_FAIL(VX_E_SHAPE, "%s: row %d: thr %u above 2^24", who, k, rows[k].thr);
    sw.from[k] = (uint8_t)rows[k].from; sw.to[k] = (uint8_t)rows[k].to; sw.thr[k] = rows[k].thr;
  }
  for (int k = 0; k < n_switch; ++k)
    for (int l = 0; l < n_switch; ++l) {
      if (l != k && rows[l].from == rows[k].from) VX_FAIL(VX_E_SHAPE, "%s: rows %d and %d start from the same label %d", who, k, l, rows[k].from);
      if (rows[l].to == rows[k].from) VX_FAIL(VX_E_SHAPE, "%s: row %d leads to label %d, which row %d starts from", who, l, rows[l].to, k);
    }
  std::vector<ls_item> table((size_t)n_items);
  int64_t n_blocks = 0;
  bool any_var = false;
  for (int i = 0; i < n_items; ++i) {
    const vx_lswitch_item& it = items[i];
    if (it.kind < VX_COUNT_B1 || it.kind > VX_COUNT_B8) VX_FAIL(VX_E_DTYPE, "%s: item %d: kind %d", who, i, it.kind);
    if (it.H < 1 || it.W < 1 || (int64_t)it.H * it.W > 0x7fffffffLL) VX_FAIL(VX_E_SHAPE, "%s: item %d: H=%d W=%d", who, i, it.H, it.W);
    if (!it.labels) VX_FAIL(VX_E_NULL, "%s: item %d: null labels", who, i);
    const int es = 1 << it.kind;
    if ((uintptr_t)it.labels % es) VX_FAIL(VX_E_ALIGN, "%s: item %d: labels not aligned to their %d-byte elements", who, i, es);
    if ((uintptr_t)it.variance % sizeof(float)) VX_FAIL(VX_E_ALIGN, "%s: item %d: variance not aligned to float", who, i);
    ls_item& d = table[(size_t)i];
    d = ls_item{};
    d.p = (const uint8_t*)it.labels; d.refs = it.refs; d.var = it.variance;
    d.block0 = n_blocks; d.H = it.H; d.W = it.W; d.esl = it.kind; d.out = i; d.index = it.index;
    d.tiles_x = (it.W + LS_TW - 1) / LS_TW;
    if (decisions)
      for (int r = 0; r < R; ++r)
        for (int k = 0; k < n_switch; ++k) {
          const uint8_t v = decisions[((size_t)i * R + r) * n_switch + k];
          if (v > 1) VX_FAIL(VX_E_SHAPE, "%s: item %d: decision (%d, %d) is %d, not 0 / 1", who, i, r, k, (int)v);
          d.dec[r] |= (uint8_t)(v << k);
        }
    n_blocks += (int64_t)d.tiles_x * ((it.H + LS_TH - 1) / LS_TH);
    any_var = any_var || it.variance;
  }
  if (any_var && !var_table) VX_FAIL(VX_E_NULL, "%s: a variance map without the variance table", who);
  if (!status || !workspace) VX_FAIL(VX_E_NULL, "%s: null status or workspace", who);
  if (ws_bytes < vx_label_switch_batched_workspace_bytes(n_items, R))
    VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)vx_label_switch_batched_workspace_bytes(n_items, R));
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)n_items * sizeof(int32_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "%s: memset: %s", who, hipGetErrorString(e));
  static const float zeros[256] = {};
  const size_t tab_off = vx_align256(256 * sizeof(float));
  const vx_stage_part parts[2] = {{var_table ? var_table : zeros, 256 * sizeof(float), 0},
                                  {table.data(), table.size() * sizeof(ls_item), tab_off}};
  const int up = vx_staged_upload(g_ls_stage, who, parts, 2, tab_off + parts[1].bytes, workspace, s);
  if (up != VX_OK) return up;
  const int grid = (int)(n_blocks < LS_MAX_GRID ? n_blocks : LS_MAX_GRID);
  hipLaunchKernelGGL(label_switch_kernel, dim3(grid), dim3(LS_THREADS), 0, s, (const ls_item*)((const char*)workspace + tab_off), n_items,
                     n_blocks, (const float*)workspace, sw, status);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
