// Host-side plan of vx_train_patches_3d (train_patches3d.hip): the argument checks, the device item table and the work
// decomposition -- which output voxels a lane writes and which source elements it reads for them.  Plain C++ with no HIP
// in it, so a stand-alone program can run it under a host sanitizer (tests/train3d_plan_host.cpp); the two functions the
// kernel shares with that program are marked T3_HD, which is empty outside hipcc.
//
// A lane takes four consecutive z of one output row (the last lane of a row the rest of it).  The lanes of an item are
// counted from the item's first voxel, so how an item is cut depends on the patch shape alone, never on its batch mates.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/values_amd.h"
#include "host_checks.h"

#if defined(__HIPCC__)
#define T3_HD __host__ __device__ __forceinline__
#else
#define T3_HD static inline
#endif

#define T3_THREADS 256
#define T3_MAX_GRID 2048   // workgroups of a launch: past T3_MAX_GRID * T3_THREADS lanes the grid-stride loop takes another trip

// one item as the kernel reads it
struct t3_item {
  const void* image;
  const void* label;           // null: no label (seg, where there is one, gets zeros)
  int32_t kind, esl, sgn;      // image kind; log2 of the label's bytes; 1: signed label elements
  int32_t D1, D2, o0, o1, o2;
  int32_t flags;
  uint32_t index;
};

struct t3_shape {
  int32_t P0, P1, P2, nq;      // nq: lanes of a row
  int64_t per, pv;             // lanes, voxels of an item
};

// what lane r (0 .. per) of an item moves: output row (a, b), z in [k0, k0 + n); the n source elements start at element
// `src` of the volume and run FORWARD; rev: they are the output's in reverse order (z-mirror)
struct t3_lane {
  int32_t a, b, k0, n, rev;
  int64_t src, dst;            // dst: offset of (a, b, k0) in the item's output patch = the noise stream's element index
};

T3_HD t3_shape t3_shape_of(int P0, int P1, int P2) {
  t3_shape s;
  s.P0 = P0; s.P1 = P1; s.P2 = P2; s.nq = (P2 + 3) >> 2;
  s.per = (int64_t)P0 * P1 * s.nq;
  s.pv = (int64_t)P0 * P1 * P2;
  return s;
}

T3_HD t3_lane t3_lane_of(const t3_shape& s, int64_t r, int D1, int D2, int o0, int o1, int o2, int flags) {
  t3_lane l;
  l.k0 = (int32_t)(r % s.nq) << 2;
  const int64_t row = r / s.nq;
  l.b = (int32_t)(row % s.P1);
  l.a = (int32_t)(row / s.P1);
  l.n = s.P2 - l.k0 < 4 ? s.P2 - l.k0 : 4;
  l.rev = (flags >> 2) & 1;
  const int sa = (flags & 1) ? s.P0 - 1 - l.a : l.a;
  const int sb = (flags & 2) ? s.P1 - 1 - l.b : l.b;
  const int sz = l.rev ? s.P2 - l.k0 - l.n : l.k0;     // output z = k0 + u reads source z = P2 - 1 - k0 - u: [sz, sz + n)
  l.src = ((int64_t)(o0 + sa) * D1 + (o1 + sb)) * D2 + (o2 + sz);
  l.dst = row * s.P2 + l.k0;
  return l;
}

static inline int t3_grid(int64_t lanes) {
  const int64_t b = (lanes + T3_THREADS - 1) / T3_THREADS;
  return (int)(b < 1 ? 1 : b > T3_MAX_GRID ? T3_MAX_GRID : b);
}

static inline int t3_elem_bytes(int kind) {
  switch (kind) {
    case VX_PREP_U8: case VX_PREP_I8: return 1;
    case VX_PREP_U16: case VX_PREP_I16: return 2;
    case VX_PREP_U32: case VX_PREP_I32: case VX_PREP_F32: return 4;
    case VX_PREP_F64: return 8;
    default: return 0;
  }
}

static inline int64_t t3_workspace_bytes(int n_items) {
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) return 0;
  return (int64_t)vx_align256((size_t)n_items * sizeof(t3_item));
}

struct t3_plan {
  std::vector<t3_item> table;
  t3_shape shape = {};
  int64_t lanes = 0;
  int grid = 0;
  int code = VX_OK;
  char err[200] = {0};
};

// every check of vx_train_patches_3d, in its order; the pointers are only tested for null and alignment
static inline int t3_make_plan(const vx_train3d_item* items, int n_items, int P0, int P1, int P2, const void* data, const void* seg,
                               int seg_u8, float var_lo, float var_hi, int sigma_law, const void* sigma_out, const void* status,
                               const void* workspace, int64_t ws_bytes, t3_plan* p) {
  const char* who = "vx_train_patches_3d";
  if (!items) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null item table", who);
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_items %d outside 1..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (P0 < 1 || P1 < 1 || P2 < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: patch %d x %d x %d", who, P0, P1, P2);
  if ((vx_wide)P0 * P1 * P2 >= ((vx_wide)1 << 32)) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: patch %d x %d x %d holds 2^32 voxels or more", who, P0, P1, P2);
  if (!(var_lo >= 0.f)) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: variance range starts below 0", who);
  if (!(var_hi >= var_lo) || !(var_hi < __builtin_inff())) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: variance range (%g, %g)", who, var_lo, var_hi);
  if (sigma_law != 0 && sigma_law != 1) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: sigma_law %d (0: sqrt(var), 1: var)", who, sigma_law);
  if (!data) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null data", who);
  if (!status) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null status", who);
  if ((uintptr_t)data % sizeof(float)) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: data not aligned to float", who);
  if (!seg_u8 && (uintptr_t)seg % sizeof(float)) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: float32 seg not aligned to float", who);
  if ((uintptr_t)sigma_out % sizeof(float)) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: sigma_out not aligned to float", who);
  if ((uintptr_t)status % sizeof(int32_t)) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: status not aligned to int32", who);
  p->table.resize((size_t)n_items);
  const int P[3] = {P0, P1, P2};
  for (int i = 0; i < n_items; ++i) {
    const vx_train3d_item& it = items[i];
    const int es = t3_elem_bytes(it.image_kind);
    if (!es) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: image kind %d", who, i, it.image_kind);
    if (it.flags & ~15) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: flags %d (bits 0-2 mirror, bit 3 noise)", who, i, it.flags);
    for (int a = 0; a < 3; ++a) {
      if (it.dims[a] < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: dims[%d] = %d", who, i, a, it.dims[a]);
      if (it.origin[a] < 0 || (int64_t)it.origin[a] + P[a] > it.dims[a])
        VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: crop [%d, %lld) of axis %d is not inside the volume's %d", who, i, it.origin[a],
                       (long long)it.origin[a] + P[a], a, it.dims[a]);
    }
    if (!it.image) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null image", who, i);
    if ((uintptr_t)it.image % (uintptr_t)es) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: item %d: image not aligned to its %d-byte elements", who, i, es);
    if (it.label) {
      if (it.label_kind < VX_COUNT_B1 || it.label_kind > VX_COUNT_B8) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: label kind %d", who, i, it.label_kind);
      if (it.label_flags & ~VX_LABEL_SIGNED) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: label flags %d", who, i, it.label_flags);
      if ((uintptr_t)it.label % ((uintptr_t)1 << it.label_kind))
        VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: item %d: label not aligned to its %d-byte elements", who, i, 1 << it.label_kind);
    }
    t3_item& d = p->table[(size_t)i];
    d.image = it.image; d.label = seg ? it.label : nullptr; d.kind = it.image_kind;
    d.esl = it.label ? it.label_kind : 0; d.sgn = it.label ? (it.label_flags & VX_LABEL_SIGNED) : 0;
    d.D1 = it.dims[1]; d.D2 = it.dims[2]; d.o0 = it.origin[0]; d.o1 = it.origin[1]; d.o2 = it.origin[2];
    d.flags = it.flags; d.index = it.index;
  }
  if (!workspace) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null workspace", who);
  if (ws_bytes < t3_workspace_bytes(n_items)) VX_REFUSE_CODE(p, VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)t3_workspace_bytes(n_items));
  if (!vx_aligned16(workspace)) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  p->shape = t3_shape_of(P0, P1, P2);
  p->lanes = (int64_t)n_items * p->shape.per;
  p->grid = t3_grid(p->lanes);
  return VX_OK;
}
