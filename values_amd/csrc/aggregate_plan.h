// Host-side plan of vx_aggregate_batched (aggregate.hip): argument checks, the LDS tile of every (item, PATCH spec)
// pair, the workspace layout.  Plain C++ with no HIP in it, so a stand-alone program can run it under a host sanitizer.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/values_amd.h"
#include "host_checks.h"

#define VX_AGG_MAX_SPECS 8
#define VX_AGG_MAX_ITEMS 4096
#define VX_AGG_THREADS 256            // workgroup of the box kernels
#define VX_AGG_LDS_SHARED (60 << 10)  // preferred tile budget: two workgroups per CU (beside the kernels' static LDS)
#define VX_AGG_LDS_WHOLE (156 << 10)  // a patch whose smallest tile needs more than this is refused
#define VX_AGG_TILE_TARGET 512        // D is split into chunks until the call has about two workgroups per CU

// one map of the sums kernel
struct agg_sum_item {
  const void* map;
  int64_t n;
  int32_t dtype, pad;
};

// one (item, PATCH spec) pair of the box kernels: the map, the patch, the tiling of its (od, oh, ow) box sums
struct agg_pair {
  const void* map;
  int64_t tile0;                 // first entry of this pair in the per-tile arrays
  int32_t dtype, out_index;      // out_index = item * n_specs + spec
  int32_t D, H, W, pd, ph, pw;
  int32_t od, oh, ow;
  int32_t TD, TH, tw_log2;       // output tile: TD slices x TH rows x (1 << tw_log2) columns
  int32_t ntd, nth, ntw, pad;
};

struct agg_plan {
  std::vector<agg_sum_item> sums;
  std::vector<agg_pair> pairs;
  int64_t tiles = 0;
  size_t lds = 0;                // dynamic LDS of the box kernels: the largest tile's
  size_t off_pairs = 0, off_tmax = 0, off_first = 0, bytes = 0;   // workspace layout ([0, off_pairs): the sum items)
  bool any_sum = false;
  char err[160] = {0};
};

// LDS of one tile: the float input rows with their halo, the row sums along W as doubles, and (pd > 1) the last pd slices
// of the sums along H for the sum along D
static inline size_t agg_tile_lds(int TH, int TW, int pd, int ph, int pw) {
  const size_t in = vx_align256((size_t)(TH + ph - 1) * (TW + pw - 1) * sizeof(float));
  const size_t ws = (size_t)(TH + ph - 1) * TW * sizeof(double);
  const size_t ring = pd > 1 ? (size_t)pd * TH * TW * sizeof(double) : 0;
  return in + ws + ring;
}

static inline bool agg_fit_tile(size_t budget, int min_th, int min_tw, int pd, int ph, int pw, int* TH, int* TW) {
  while (agg_tile_lds(*TH, *TW, pd, ph, pw) > budget) {
    if (*TW > *TH && *TW > min_tw) *TW >>= 1;
    else if (*TH > min_th) *TH = (*TH + 1) >> 1;
    else if (*TW > min_tw) *TW >>= 1;
    else return false;
  }
  return true;
}

// VX_OK and a filled plan, or a VX_E_* code and plan->err
static inline int agg_make_plan(const vx_agg_item* items, int n_items, const vx_agg_spec* specs, int n_specs, agg_plan* p) {
  if (!items || !specs) VX_REFUSE(p, VX_E_NULL, "vx_aggregate_batched: null items or specs");
  if (n_items < 1 || n_items > VX_AGG_MAX_ITEMS) VX_REFUSE(p, VX_E_SHAPE, "vx_aggregate_batched: n_items %d outside 1..%d", n_items, VX_AGG_MAX_ITEMS);
  if (n_specs < 1 || n_specs > VX_AGG_MAX_SPECS) VX_REFUSE(p, VX_E_SHAPE, "vx_aggregate_batched: n_specs %d outside 1..%d", n_specs, VX_AGG_MAX_SPECS);
  for (int s = 0; s < n_specs; ++s) {
    const vx_agg_spec& sp = specs[s];
    if (sp.kind == VX_AGG_IMAGE || sp.kind == VX_AGG_THRESHOLD) p->any_sum = true;
    else if (sp.kind != VX_AGG_PATCH) VX_REFUSE(p, VX_E_DTYPE, "vx_aggregate_batched: spec %d: kind %d", s, sp.kind);
    else if (sp.pd < 1 || sp.ph < 1 || sp.pw < 1) VX_REFUSE(p, VX_E_SHAPE, "vx_aggregate_batched: spec %d: patch (%d,%d,%d)", s, sp.pd, sp.ph, sp.pw);
  }
  int64_t hw_tiles = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_agg_item& it = items[i];
    if (!it.map) VX_REFUSE(p, VX_E_NULL, "vx_aggregate_batched: item %d: null map", i);
    if (it.dtype != VX_F32 && it.dtype != VX_F64) VX_REFUSE(p, VX_E_DTYPE, "vx_aggregate_batched: item %d: dtype %d", i, it.dtype);
    if (it.D < 1 || it.H < 1 || it.W < 1) VX_REFUSE(p, VX_E_SHAPE, "vx_aggregate_batched: item %d: map (%d,%d,%d)", i, it.D, it.H, it.W);
    if (p->any_sum) p->sums.push_back(agg_sum_item{it.map, (int64_t)it.D * it.H * it.W, it.dtype, 0});
    for (int s = 0; s < n_specs; ++s) {
      const vx_agg_spec& sp = specs[s];
      if (sp.kind != VX_AGG_PATCH) continue;
      if (sp.pd > it.D || sp.ph > it.H || sp.pw > it.W)
        VX_REFUSE(p, VX_E_SHAPE, "vx_aggregate_batched: item %d: patch (%d,%d,%d) of spec %d must fit map (%d,%d,%d)", i, sp.pd, sp.ph,
                   sp.pw, s, it.D, it.H, it.W);
      agg_pair q;
      memset(&q, 0, sizeof(q));
      q.map = it.map; q.dtype = it.dtype; q.out_index = i * n_specs + s;
      q.D = it.D; q.H = it.H; q.W = it.W; q.pd = sp.pd; q.ph = sp.ph; q.pw = sp.pw;
      q.od = it.D - sp.pd + 1; q.oh = it.H - sp.ph + 1; q.ow = it.W - sp.pw + 1;
      int TW = 64, TH = sp.pd > 1 ? 16 : 32;    // no ring for a 2D map: a taller tile repeats less of the halo
      while (TW > 1 && (TW >> 1) >= q.ow) TW >>= 1;
      if (TH > q.oh) TH = q.oh;
      if (!agg_fit_tile(VX_AGG_LDS_SHARED, TH < 4 ? TH : 4, TW < 16 ? TW : 16, sp.pd, sp.ph, sp.pw, &TH, &TW) &&
          !agg_fit_tile(VX_AGG_LDS_WHOLE, 1, 1, sp.pd, sp.ph, sp.pw, &TH, &TW))
        VX_REFUSE(p, VX_E_SHAPE, "vx_aggregate_batched: item %d: patch (%d,%d,%d) of spec %d leaves no LDS tile (%zu bytes at 1x1)", i,
                   sp.pd, sp.ph, sp.pw, s, agg_tile_lds(1, 1, sp.pd, sp.ph, sp.pw));
      q.TH = TH;
      for (q.tw_log2 = 0; (1 << q.tw_log2) < TW; ++q.tw_log2) {}
      q.nth = (q.oh + TH - 1) / TH;
      q.ntw = (q.ow + TW - 1) / TW;
      hw_tiles += (int64_t)q.nth * q.ntw;
      const size_t lds = agg_tile_lds(TH, TW, sp.pd, sp.ph, sp.pw);
      if (lds > p->lds) p->lds = lds;
      p->pairs.push_back(q);
    }
  }
  // chunks along D: only while the call has few workgroups, and never shorter than two patch depths (the pd - 1 leading
  // slices of a chunk are computed again)
  const int64_t want = hw_tiles > 0 ? (VX_AGG_TILE_TARGET + hw_tiles - 1) / hw_tiles : 1;
  for (agg_pair& q : p->pairs) {
    int64_t ntd = q.od / (2 * (int64_t)q.pd);
    if (ntd > want) ntd = want;
    if (ntd < 1) ntd = 1;
    q.TD = (int32_t)((q.od + ntd - 1) / ntd);
    q.ntd = (q.od + q.TD - 1) / q.TD;
    q.tile0 = p->tiles;
    p->tiles += (int64_t)q.ntd * q.nth * q.ntw;
  }
  p->off_pairs = vx_align256(p->sums.size() * sizeof(agg_sum_item));
  p->off_tmax = p->off_pairs + vx_align256(p->pairs.size() * sizeof(agg_pair));
  p->off_first = p->off_tmax + vx_align256((size_t)p->tiles * sizeof(double));
  p->bytes = p->off_first + vx_align256((size_t)p->tiles * sizeof(int64_t));
  if (p->bytes == 0) p->bytes = 256;
  return VX_OK;
}
