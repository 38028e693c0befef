// Host-side plan of the toy data set kernels (toydata.hip, K42): the argument checks, the reflect index of the blur, the
// clipped object box of the embed, the tile shapes of the blur passes and the workspace layout of the order statistics.
// Plain C++ with no HIP in it (the two index helpers are also device code when hipcc compiles them), so a stand-alone
// program can run it under a host sanitizer (tests/toy_plan_host.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/values_amd.h"
#include "host_checks.h"

#ifdef __HIPCC__
#define TOY_HD __host__ __device__ __forceinline__
#else
#define TOY_HD static inline
#endif

#define TOY_THREADS 256
#define TOY_MAX_RADIUS 128
#define TOY_MAX_N ((int64_t)1 << 40)   // voxels of one image
#define TOY_LDS_BYTES 65536            // the LDS a blur workgroup may ask for
#define TOY_STRIDED_ROWS 2             // axes 0 / 1: consecutive rows one thread produces (4 measured no faster: DESIGN 4.49)
#define TOY_ROW_SEG 128                // axis 2: outputs of one wave's row segment
#define TOY_ROW_WAVES 4                // axis 2: rows of a workgroup, one per wave
#define TOY_MAX_GRID 2048              // the element-wise kernels' grid-stride grids
#define TOY_OS_MAX_K 32
#define TOY_OS_CHUNK 16                // ranks resolved by one sweep of eight passes
#define TOY_SEG_MAX_R 64

// scipy's `reflect` (d c b a | a b c d | d c b a): index i of the line extended to both sides, for ANY i and n >= 1 --
// period 2n, the second half mirrored
TOY_HD int toy_reflect(int64_t i, int n) {
  const int64_t p = 2 * (int64_t)n;
  int64_t m = i % p;
  if (m < 0) m += p;
  return (int)(m < n ? m : p - 1 - m);
}

// ---------------------------------------------------------------------------------------------------------------
// vx_toy_embed: the object's box clipped to the image, in image coordinates BEFORE the flips
struct toy_embed_plan {
  int32_t lo[3], hi[3];   // image voxels [lo, hi) take gray * obj[voxel - off]; hi <= lo on an axis: nothing to place
  int64_t n = 0;
  int code = VX_OK;
  char err[160] = {0};
};

static inline int toy_plan_embed(const void* obj, const int32_t* obj_dims, const int32_t* offset, const void* image,
                                 const int32_t* dims, toy_embed_plan* p) {
  const char* who = "vx_toy_embed";
  if (!obj || !obj_dims || !offset || !image || !dims) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null pointer", who);
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || obj_dims[a] < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: axis %d: image %d, object %d voxels", who, a, dims[a], obj_dims[a]);
    n *= dims[a];
    if (n > TOY_MAX_N) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: more than 2^40 voxels", who);
    const int64_t lo = offset[a] > 0 ? offset[a] : 0;
    const int64_t end = (int64_t)offset[a] + obj_dims[a];
    const int64_t hi = end < dims[a] ? end : dims[a];
    p->lo[a] = (int32_t)(lo < dims[a] ? lo : dims[a]);
    p->hi[a] = (int32_t)(hi > 0 ? hi : 0);
  }
  if ((uintptr_t)obj & 3) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: obj not aligned to its 4-byte elements", who);
  if ((uintptr_t)image & 7) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: image not aligned to its 8-byte elements", who);
  p->n = n;
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// vx_gauss_blur_axis_f64.  Axes 0 and 1 are one kernel on the view [outer][len][inner] (axis 0: outer 1, inner D1 D2; axis
// 1: outer D0, inner D2): a workgroup owns `tw` columns of one outer index and walks len in steps of `step` rows with
// the 2 radius + step rows it needs in an LDS ring.  Axis 2 stages a row segment plus halo per wave.
struct toy_blur_plan {
  int64_t outer = 0, len = 0, inner = 0;
  int tw = 0, step = 0, ring_rows = 0;   // axes 0 / 1
  int64_t slabs = 0;                     // column slabs per outer index (axes 0 / 1); row segments per row (axis 2)
  int64_t blocks = 0;
  size_t lds = 0;
  int vec = 0;                           // 16-byte loads and stores (an even contiguous extent, both pointers aligned)
  int code = VX_OK;
  char err[160] = {0};
};

static inline int toy_strided_step(int tw) { return TOY_STRIDED_ROWS * (TOY_THREADS / (tw / 2)); }

static inline int toy_plan_blur(const void* src, const void* dst, const int32_t* dims, int axis, const void* weights, int radius,
                                toy_blur_plan* p) {
  const char* who = "vx_gauss_blur_axis_f64";
  if (!src || !dst || !dims || !weights) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null pointer", who);
  if (axis < 0 || axis > 2) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: axis %d", who, axis);
  if (radius < 0 || radius > TOY_MAX_RADIUS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: radius %d outside 0..%d", who, radius, TOY_MAX_RADIUS);
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: axis %d: %d voxels", who, a, dims[a]);
    n *= dims[a];
    if (n > TOY_MAX_N) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: more than 2^40 voxels", who);
  }
  if (((uintptr_t)src & 7) || ((uintptr_t)dst & 7) || ((uintptr_t)weights & 7))
    VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: src, dst or weights not aligned to its 8-byte elements", who);
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)n * 8, d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)n * 8;
  if (s0 < d1 && d0 < s1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: src and dst overlap (a pass never runs in place)", who);
  const bool al16 = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  if (axis == 2) {
    p->outer = (int64_t)dims[0] * dims[1]; p->len = dims[2]; p->inner = 1;
    p->slabs = (dims[2] + TOY_ROW_SEG - 1) / TOY_ROW_SEG;
    p->blocks = ((p->outer + TOY_ROW_WAVES - 1) / TOY_ROW_WAVES) * p->slabs;
    p->lds = (size_t)TOY_ROW_WAVES * (TOY_ROW_SEG + 2 * radius) * 8;
    p->vec = al16 && dims[2] % 2 == 0;
  } else {
    p->outer = axis == 0 ? 1 : dims[0];
    p->len = dims[axis];
    p->inner = axis == 0 ? (int64_t)dims[1] * dims[2] : dims[2];
    for (int tw = 64; tw >= 16; tw >>= 1) {   // the widest slab whose ring fits
      p->tw = tw; p->step = toy_strided_step(tw); p->ring_rows = 2 * radius + p->step;
      p->lds = (size_t)p->ring_rows * tw * 8;
      if (p->lds <= TOY_LDS_BYTES) break;
    }
    p->slabs = (p->inner + p->tw - 1) / p->tw;
    p->blocks = p->outer * p->slabs;
    p->vec = al16 && p->inner % 2 == 0;
  }
  if (p->lds > TOY_LDS_BYTES) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: radius %d: no tile fits the LDS", who, radius);
  if (p->blocks > 0x7fffffffLL) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: %lld workgroups", who, (long long)p->blocks);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// vx_order_stats_f64: the distinct ranks {k, min(k + 1, n - 1)} in ascending order, which of them each output takes, and
// the workspace [prefix 16 x u64 | remaining rank 16 x i64 | histograms 16 x 256 x u64 | values 64 x f64]
struct toy_os_plan {
  int n_u = 0;
  int64_t u[2 * TOY_OS_MAX_K];
  int32_t idx[TOY_OS_MAX_K][2];
  int chunks = 0, reads = 0;           // sweeps of eight passes; reads of the data (one per pass)
  size_t off_krem = 0, off_hist = 0, off_vals = 0, bytes = 0;
  int code = VX_OK;
  char err[160] = {0};
};

static inline size_t toy_os_bytes() {
  return vx_align256(2 * TOY_OS_CHUNK * 8) + vx_align256((size_t)TOY_OS_CHUNK * 256 * 8) + vx_align256(2 * TOY_OS_MAX_K * 8);
}

static inline int toy_plan_order_stats(const void* x, int64_t n, const int64_t* ks, int n_k, const void* out, const void* status,
                                       const void* workspace, int64_t ws_bytes, toy_os_plan* p) {
  const char* who = "vx_order_stats_f64";
  if (n_k < 1 || n_k > TOY_OS_MAX_K) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_k %d outside 1..%d", who, n_k, TOY_OS_MAX_K);
  if (n < 1 || n > TOY_MAX_N) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n=%lld outside 1..2^40", who, (long long)n);
  if (!x || !ks || !out || !status || !workspace) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null pointer", who);
  for (int i = 0; i < n_k; ++i)
    if (ks[i] < 0 || ks[i] >= n) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: rank %d: k=%lld outside [0, %lld)", who, i, (long long)ks[i], (long long)n);
  if (((uintptr_t)x & 7) || ((uintptr_t)out & 7) || ((uintptr_t)status & 3))
    VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: x, out or status not aligned to its elements", who);
  if ((uintptr_t)workspace & 15) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  p->off_krem = TOY_OS_CHUNK * 8;
  p->off_hist = vx_align256(2 * TOY_OS_CHUNK * 8);
  p->off_vals = p->off_hist + vx_align256((size_t)TOY_OS_CHUNK * 256 * 8);
  p->bytes = toy_os_bytes();
  if (ws_bytes < (int64_t)p->bytes) VX_REFUSE_CODE(p, VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)p->bytes);
  // insertion into the sorted list of distinct ranks (at most 64)
  for (int i = 0; i < n_k; ++i) {
    for (int h = 0; h < 2; ++h) {
      const int64_t k = h == 0 ? ks[i] : (ks[i] + 1 < n ? ks[i] + 1 : ks[i]);
      int pos = 0;
      while (pos < p->n_u && p->u[pos] < k) ++pos;
      if (pos == p->n_u || p->u[pos] != k) {
        for (int j = p->n_u; j > pos; --j) p->u[j] = p->u[j - 1];
        p->u[pos] = k;
        ++p->n_u;
      }
    }
  }
  for (int i = 0; i < n_k; ++i) {
    for (int h = 0; h < 2; ++h) {
      const int64_t k = h == 0 ? ks[i] : (ks[i] + 1 < n ? ks[i] + 1 : ks[i]);
      int pos = 0;
      while (p->u[pos] != k) ++pos;
      p->idx[i][h] = pos;
    }
  }
  p->chunks = (p->n_u + TOY_OS_CHUNK - 1) / TOY_OS_CHUNK;
  p->reads = 8 * p->chunks;
  return VX_OK;
}
