// Host-side plan of vx_volume_stats_batched and vx_zscore_pad_batched (preprocess.hip): the argument checks, the work
// blocks of every item and the workspace layout.  Plain C++ with no HIP in it, so a stand-alone program can run it under
// a host sanitizer (tests/prep_plan_host.cpp).
//
// A work block is PP_BLOCK_BYTES of an item's source (statistics) or of its output (normalise-and-pad), counted from the
// item's first element: how an item is cut depends on its own element count and kind alone, never on its batch mates.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/values_amd.h"
#include "host_checks.h"

#define PP_THREADS 256
#define PP_BLOCK_CHUNKS 2048                      // 16-byte chunks per work block: eight per thread
#define PP_BLOCK_BYTES (PP_BLOCK_CHUNKS * 16)
#define PP_MAX_GRID 2048
#define PP_MAX_N ((int64_t)1 << 40)               // elements of one item

// one item of the statistics kernels
struct pp_stat_item {
  const void* p;
  int64_t n;
  int64_t block0, n_blocks;    // its work blocks are [block0, block0 + n_blocks) of the call
  int32_t kind, pad;
};

// what a work block leaves for the item's final workgroup.  Pass 1: s (float kinds) or is (integer kinds) = the block's
// sum, mn its minimum, nan whether it holds a NaN; pass 2 overwrites s with the block's sum of squared deviations.
struct pp_partial {
  double s, mn;
  int64_t is;
  int32_t nan, pad;
};

// one item of the normalise-and-pad kernel
struct pp_pad_item {
  const void* src;
  void* dst;
  int64_t block0;
  int64_t out_n;               // output elements
  int32_t d[3], o[3], lo[3];   // source box, output box, the source's place in it
  int32_t kind, out, mode, row;   // out: VX_F32 / VX_F64 (ZSCORE; COPY keeps the kind)
};

struct pp_plan {
  std::vector<pp_stat_item> stat;
  std::vector<pp_pad_item> pad;
  int64_t n_blocks = 0;
  size_t off_partial = 0, bytes = 0;   // workspace: [0, off_partial) the item table, then the block partials
  int code = VX_OK;
  char err[160] = {0};
};

static inline int pp_elem_bytes(int kind) {
  switch (kind) {
    case VX_PREP_U8: case VX_PREP_I8: return 1;
    case VX_PREP_U16: case VX_PREP_I16: return 2;
    case VX_PREP_U32: case VX_PREP_I32: case VX_PREP_F32: return 4;
    case VX_PREP_F64: return 8;
    default: return 0;
  }
}

// vx_volume_stats_batched: checks of the table, the items' work blocks, the workspace size
static inline int pp_plan_stats(const vx_prep_item* items, int n_items, pp_plan* p) {
  const char* who = "vx_volume_stats_batched";
  if (n_items < 0 || n_items > VX_SELECT_MAX_ITEMS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_items %d outside 0..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (n_items == 0) return VX_OK;
  if (!items) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null items", who);
  p->stat.reserve((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    const vx_prep_item& it = items[i];
    const int es = pp_elem_bytes(it.kind);
    if (!es) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: kind %d", who, i, it.kind);
    if (it.n < 1 || it.n > PP_MAX_N) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: n=%lld outside 1..2^40", who, i, (long long)it.n);
    if (!it.ptr) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null pointer", who, i);
    if ((uintptr_t)it.ptr % (uintptr_t)es) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: item %d: pointer not aligned to its %d-byte elements", who, i, es);
    const int64_t nb = (it.n * es + PP_BLOCK_BYTES - 1) / PP_BLOCK_BYTES;
    p->stat.push_back(pp_stat_item{it.ptr, it.n, p->n_blocks, nb, it.kind, 0});
    p->n_blocks += nb;
  }
  p->off_partial = vx_align256((size_t)n_items * sizeof(pp_stat_item));
  p->bytes = p->off_partial + vx_align256((size_t)p->n_blocks * sizeof(pp_partial));
  return VX_OK;
}

// vx_zscore_pad_batched
static inline int pp_plan_pad(const vx_prep_pad_item* items, int n_items, pp_plan* p) {
  const char* who = "vx_zscore_pad_batched";
  if (n_items < 0 || n_items > VX_SELECT_MAX_ITEMS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_items %d outside 0..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (n_items == 0) return VX_OK;
  if (!items) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null items", who);
  p->pad.reserve((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    const vx_prep_pad_item& it = items[i];
    const int es = pp_elem_bytes(it.kind);
    if (!es) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: kind %d", who, i, it.kind);
    if (it.mode != VX_PREP_ZSCORE && it.mode != VX_PREP_COPY) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: mode %d", who, i, it.mode);
    int out = it.out_dtype, oes = es;
    if (it.mode == VX_PREP_COPY) {
      if (out != VX_PREP_OWN) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: COPY keeps the source's kind (out_dtype VX_PREP_OWN), not %d", who, i, out);
    } else {
      if (out == VX_PREP_OWN) out = it.kind == VX_PREP_F32 ? VX_F32 : VX_F64;   // as numpy promotes (x - float64) / float64
      if (out != VX_F32 && out != VX_F64) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: out_dtype %d", who, i, it.out_dtype);
      oes = out == VX_F32 ? 4 : 8;
    }
    int64_t n = 1, on = 1;
    for (int a = 0; a < 3; ++a) {
      if (it.dims[a] < 1 || it.out_dims[a] < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: axis %d: %d -> %d voxels", who, i, a, it.dims[a], it.out_dims[a]);
      if (it.pad_below[a] < 0) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: axis %d: pad_below %d", who, i, a, it.pad_below[a]);
      if ((int64_t)it.out_dims[a] < (int64_t)it.dims[a] + it.pad_below[a])
        VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: axis %d: %d + %d voxels do not fit %d", who, i, a, it.pad_below[a], it.dims[a], it.out_dims[a]);
      n *= it.dims[a];
      on *= it.out_dims[a];
      if (on > PP_MAX_N) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: more than 2^40 output voxels", who, i);
    }
    if (it.stats_row < 0 || it.stats_row >= VX_SELECT_MAX_ITEMS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: stats_row %d", who, i, it.stats_row);
    if (!it.src || !it.dst) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null src or dst", who, i);
    if ((uintptr_t)it.src % (uintptr_t)es) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: item %d: src not aligned to its %d-byte elements", who, i, es);
    if ((uintptr_t)it.dst % (uintptr_t)oes) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: item %d: dst not aligned to its %d-byte elements", who, i, oes);
    const uintptr_t s0 = (uintptr_t)it.src, s1 = s0 + (uintptr_t)(n * es), d0 = (uintptr_t)it.dst, d1 = d0 + (uintptr_t)(on * oes);
    if (s0 < d1 && d0 < s1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: src and dst overlap", who, i);
    pp_pad_item t;
    t.src = it.src; t.dst = it.dst; t.block0 = p->n_blocks; t.out_n = on;
    for (int a = 0; a < 3; ++a) { t.d[a] = it.dims[a]; t.o[a] = it.out_dims[a]; t.lo[a] = it.pad_below[a]; }
    t.kind = it.kind; t.out = out; t.mode = it.mode; t.row = it.stats_row;
    p->pad.push_back(t);
    p->n_blocks += (on * oes + PP_BLOCK_BYTES - 1) / PP_BLOCK_BYTES;
  }
  p->off_partial = p->bytes = vx_align256((size_t)n_items * sizeof(pp_pad_item));
  return VX_OK;
}
