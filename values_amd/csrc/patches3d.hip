// K45-K47: the three batched streaming passes of the 3D test split (values_amd.sliding.run_test_3d).
//   vx_gather_patches_3d         the crops of a forward batch, taken from volumes of different cases, shapes and stored
//                                dtypes, converted to float32 as numpy's astype converts, in ONE launch
//   vx_softmax_accumulate_cases  softmax_accumulate_kernel (accumulate.hip, K14) with the destination image taken per patch
//   vx_case_composite            what DataCarrier3D.concat_data / save_data / calculate_metrics make of a case's input and
//                                raters (data_carrier_3D.py:130-153, 173-179, 209-214; test_3D.py:555-562), in float64
// All three are HBM-bound.  Lanes run along z, the contiguous axis of volumes, patches and outputs: a lane takes FOUR
// consecutive z positions of one row and moves them in one access of up to 16 bytes wherever the four elements lie inside
// the row and their address is aligned to the access (vx4_load / vx4_store decide per access); a row's ragged end, a row
// that starts off the access's phase and everything the atomics touch go element by element.  No byte outside a source
// volume's crop, a destination box or an output array is read or written.  Plain C++ loads and stores; the only atomics are
// the float adds of overlapping patches and the integer count of labels outside 0..255.
// The item tables go up through the pinned staging buffer of staging.h: no wait on the stream, not capturable into a
// hipGraph.  Every argument check runs before any device call.
#include <algorithm>
#include <vector>

#include "common.h"
#include "staging.h"
#include "vx4_access.h"   // four consecutive elements per lane: vx4_load / vx4_store / vx4_load_kind / vx4_load_label

#define P3_THREADS 256
#define P3_MAX_GRID 2048
#define P3_CHUNK (P3_THREADS * 4)   // voxels of a composite work block: four per lane

static inline int p3_esize(int kind) {
  switch (kind) {
    case VX_PREP_U8: case VX_PREP_I8: return 1;
    case VX_PREP_U16: case VX_PREP_I16: return 2;
    case VX_PREP_U32: case VX_PREP_I32: case VX_PREP_F32: return 4;
    case VX_PREP_F64: return 8;
    default: return 0;
  }
}

static inline int p3_grid(int64_t work_threads) {
  const int64_t b = (work_threads + P3_THREADS - 1) / P3_THREADS;
  return (int)(b < 1 ? 1 : b > P3_MAX_GRID ? P3_MAX_GRID : b);
}

// ---------------------------------------------------------------------------------------------------------------
// K45 gather

struct p3_gather_item {
  const void* src;
  int32_t kind, D1, D2, o0, o1, o2;
};

__global__ __launch_bounds__(P3_THREADS) void gather_patches_3d_kernel(const p3_gather_item* __restrict__ items, int n_items,
                                                                       float* __restrict__ out, int P0, int P1, int P2) {
  const int nq = (P2 + 3) >> 2;                      // lanes of a row
  const int64_t rows = (int64_t)P0 * P1;
  const int64_t per = rows * nq;                     // lanes of an item
  const int64_t pv = rows * P2;
  const int64_t total = (int64_t)n_items * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int it = (int)(i / per);
    const int64_t r = i - (int64_t)it * per;
    const int k0 = (int)(r % nq) << 2;
    const int64_t row = r / nq;
    const int b = (int)(row % P1), a = (int)(row / P1);
    const p3_gather_item g = items[it];
    const int n = P2 - k0 < 4 ? P2 - k0 : 4;
    const int64_t e = ((int64_t)(g.o0 + a) * g.D1 + (g.o1 + b)) * g.D2 + (g.o2 + k0);
    double d[4];
    vx4_load_kind(g.src, g.kind, e, n, d);
    float f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = (float)d[u];   // round to nearest even, as astype(float32)
    vx4_store<float>(out + (int64_t)it * pv + row * P2 + k0, n, f);
  }
}

static vx_staging g_gather_stage;

extern "C" int64_t vx_gather_patches_3d_workspace_bytes(int n_items) {
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) return 0;
  return (int64_t)vx_align256((size_t)n_items * sizeof(p3_gather_item));
}

extern "C" int vx_gather_patches_3d(const vx_gather3d_item* items, int n_items, float* out, int P0, int P1, int P2, void* workspace,
                                    int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_gather_patches_3d";
  if (!items) VX_FAIL(VX_E_NULL, "%s: null item table", who);
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) VX_FAIL(VX_E_SHAPE, "%s: n_items %d outside 1..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (P0 < 1 || P1 < 1 || P2 < 1) VX_FAIL(VX_E_SHAPE, "%s: patch %d x %d x %d", who, P0, P1, P2);
  if (!out) VX_FAIL(VX_E_NULL, "%s: null out", who);
  if ((uintptr_t)out % sizeof(float)) VX_FAIL(VX_E_ALIGN, "%s: out not aligned to float", who);
  std::vector<p3_gather_item> table((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    const vx_gather3d_item& it = items[i];
    const int es = p3_esize(it.kind);
    if (!es) VX_FAIL(VX_E_DTYPE, "%s: item %d: kind %d", who, i, it.kind);
    for (int a = 0; a < 3; ++a) {
      const int P = a == 0 ? P0 : a == 1 ? P1 : P2;
      if (it.dims[a] < 1) VX_FAIL(VX_E_SHAPE, "%s: item %d: dims[%d] = %d", who, i, a, it.dims[a]);
      if (it.origin[a] < 0 || (int64_t)it.origin[a] + P > it.dims[a])
        VX_FAIL(VX_E_SHAPE, "%s: item %d: crop [%d, %lld) of axis %d is not inside the volume's %d", who, i, it.origin[a],
                (long long)it.origin[a] + P, a, it.dims[a]);
    }
    if (!it.src) VX_FAIL(VX_E_NULL, "%s: item %d: null src", who, i);
    if ((uintptr_t)it.src % es) VX_FAIL(VX_E_ALIGN, "%s: item %d: src not aligned to its %d-byte elements", who, i, es);
    p3_gather_item& d = table[(size_t)i];
    d.src = it.src; d.kind = it.kind; d.D1 = it.dims[1]; d.D2 = it.dims[2];
    d.o0 = it.origin[0]; d.o1 = it.origin[1]; d.o2 = it.origin[2];
  }
  if (!workspace) VX_FAIL(VX_E_NULL, "%s: null workspace", who);
  if (ws_bytes < vx_gather_patches_3d_workspace_bytes(n_items))
    VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)vx_gather_patches_3d_workspace_bytes(n_items));
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const vx_stage_part part = {table.data(), table.size() * sizeof(p3_gather_item), 0};
  const int up = vx_staged_upload(g_gather_stage, who, &part, 1, part.bytes, workspace, s);
  if (up != VX_OK) return up;
  const int64_t lanes = (int64_t)n_items * P0 * P1 * ((P2 + 3) / 4);
  hipLaunchKernelGGL(gather_patches_3d_kernel, dim3(p3_grid(lanes)), dim3(P3_THREADS), 0, s, (const p3_gather_item*)workspace, n_items,
                     out, P0, P1, P2);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// K46 accumulate: per voxel the expressions of softmax_accumulate_kernel, in its order

struct p3_acc_item {
  float* sum;
  float* count;
  int32_t X, Y, Z, o0, o1, o2;
};

template <int C>
__global__ __launch_bounds__(P3_THREADS) void softmax_accumulate_cases_kernel(const float* __restrict__ logits, int B, int T, int P0,
                                                                              int P1, int P2, const p3_acc_item* __restrict__ items,
                                                                              int overlap) {
  const int nq = (P2 + 3) >> 2;
  const int64_t pv = (int64_t)P0 * P1 * P2;
  const int64_t per = (int64_t)P0 * P1 * nq;
  const int64_t total = (int64_t)B * T * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i % per;
    const int t = (int)((i / per) % T);
    const int b = (int)(i / (per * T));
    const int k0 = (int)(r % nq) << 2;
    const int64_t row = r / nq;
    const int j = (int)(row % P1), ii = (int)(row / P1);
    const p3_acc_item it = items[b];
    const int x = it.o0 + ii, y = it.o1 + j, z0 = it.o2 + k0;
    if (x >= it.X || y >= it.Y || z0 >= it.Z) continue;
    int n = P2 - k0 < 4 ? P2 - k0 : 4;                 // voxels of the patch row this lane holds
    const int64_t v = row * P2 + k0;
    const float* lg = logits + ((size_t)(b * (int64_t)T + t) * C) * pv + v;
    float l[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) vx4_load<float>(lg + (size_t)c * pv, n, l[c]);
    if (it.Z - z0 < n) n = it.Z - z0;                  // ... of which n lie inside the image
    float p[C][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float e[C];
      float m = l[0][u];
#pragma unroll
      for (int c = 1; c < C; ++c) m = fmaxf(m, l[c][u]);
      float den = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) { e[c] = expf(l[c][u] - m); den += e[c]; }
      const float inv = 1.f / den;
#pragma unroll
      for (int c = 0; c < C; ++c) p[c][u] = e[c] * inv;
    }
    const int64_t img = (int64_t)it.X * it.Y * it.Z;
    const int64_t o = ((int64_t)x * it.Y + y) * it.Z + z0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float* dst = it.sum + ((size_t)t * C + c) * img + o;
      if (overlap) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < n) atomicAdd(dst + u, p[c][u]);
      } else {
        float d[4];
        vx4_load<float>(dst, n, d);
#pragma unroll
        for (int u = 0; u < 4; ++u) d[u] += p[c][u];
        vx4_store<float>(dst, n, d);
      }
    }
    if (t == 0) {
      float* cnt = it.count + o;
      if (overlap) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < n) atomicAdd(cnt + u, 1.f);
      } else {
        float d[4];
        vx4_load<float>(cnt, n, d);
#pragma unroll
        for (int u = 0; u < 4; ++u) d[u] += 1.f;
        vx4_store<float>(cnt, n, d);
      }
    }
  }
}

static vx_staging g_acc_stage;

extern "C" int64_t vx_softmax_accumulate_cases_workspace_bytes(int B) {
  if (B < 1 || B > VX_SELECT_MAX_ITEMS) return 0;
  return (int64_t)vx_align256((size_t)B * sizeof(p3_acc_item));
}

extern "C" int vx_softmax_accumulate_cases(const float* logits, int B, int T, int C, int P0, int P1, int P2, const vx_acc3d_item* items,
                                           int sum_overlap, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_softmax_accumulate_cases";
  if (!logits || !items) VX_FAIL(VX_E_NULL, "%s: null logits or item table", who);
  if (B < 1 || B > VX_SELECT_MAX_ITEMS) VX_FAIL(VX_E_SHAPE, "%s: B %d outside 1..%d", who, B, VX_SELECT_MAX_ITEMS);
  if (T <= 0 || P0 <= 0 || P1 <= 0 || P2 <= 0) VX_FAIL(VX_E_SHAPE, "%s: empty shape", who);
  if (C < 2 || C > 8) VX_FAIL(VX_E_SHAPE, "%s: 2 <= C <= 8 (got %d)", who, C);
  if ((uintptr_t)logits % sizeof(float)) VX_FAIL(VX_E_ALIGN, "%s: logits not aligned to float", who);
  std::vector<p3_acc_item> table((size_t)B);
  for (int b = 0; b < B; ++b) {
    const vx_acc3d_item& it = items[b];
    if (!it.sum || !it.count) VX_FAIL(VX_E_NULL, "%s: item %d: null sum or count", who, b);
    if ((uintptr_t)it.sum % sizeof(float) || (uintptr_t)it.count % sizeof(float))
      VX_FAIL(VX_E_ALIGN, "%s: item %d: sum or count not aligned to float", who, b);
    for (int a = 0; a < 3; ++a) {
      if (it.dims[a] < 1) VX_FAIL(VX_E_SHAPE, "%s: item %d: dims[%d] = %d", who, b, a, it.dims[a]);
      if (it.origin[a] < 0) VX_FAIL(VX_E_SHAPE, "%s: item %d: origin[%d] = %d", who, b, a, it.origin[a]);
    }
    p3_acc_item& d = table[(size_t)b];
    d.sum = it.sum; d.count = it.count; d.X = it.dims[0]; d.Y = it.dims[1]; d.Z = it.dims[2];
    d.o0 = it.origin[0]; d.o1 = it.origin[1]; d.o2 = it.origin[2];
  }
  if (!sum_overlap) {   // plain read-modify-write: no voxel may be named twice in one launch
    std::vector<int> order((size_t)B);
    for (int b = 0; b < B; ++b) order[(size_t)b] = b;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return (uintptr_t)table[(size_t)a].sum < (uintptr_t)table[(size_t)b].sum; });
    const int P[3] = {P0, P1, P2};
    for (int i = 0; i < B; ++i)
      for (int k = i + 1; k < B && table[(size_t)order[(size_t)k]].sum == table[(size_t)order[(size_t)i]].sum; ++k) {
        const vx_acc3d_item &p = items[order[(size_t)i]], &q = items[order[(size_t)k]];
        bool meet = true;
        for (int a = 0; a < 3; ++a) {   // the boxes cut to the image (p.dims: one sum is one image)
          const int64_t pe = std::min<int64_t>((int64_t)p.origin[a] + P[a], p.dims[a]), qe = std::min<int64_t>((int64_t)q.origin[a] + P[a], p.dims[a]);
          meet = meet && std::max(p.origin[a], q.origin[a]) < std::min(pe, qe);
        }
        if (meet) VX_FAIL(VX_E_SHAPE, "%s: items %d and %d add into overlapping boxes of one sum without sum_overlap", who,
                          order[(size_t)i], order[(size_t)k]);
      }
  }
  if (!workspace) VX_FAIL(VX_E_NULL, "%s: null workspace", who);
  if (ws_bytes < vx_softmax_accumulate_cases_workspace_bytes(B))
    VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)vx_softmax_accumulate_cases_workspace_bytes(B));
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const vx_stage_part part = {table.data(), table.size() * sizeof(p3_acc_item), 0};
  const int up = vx_staged_upload(g_acc_stage, who, &part, 1, part.bytes, workspace, s);
  if (up != VX_OK) return up;
  const int grid = p3_grid((int64_t)B * T * P0 * P1 * ((P2 + 3) / 4));
  const p3_acc_item* tab = (const p3_acc_item*)workspace;
#define VX_ACC(CC)                                                                                                              \
  case CC:                                                                                                                      \
    hipLaunchKernelGGL(softmax_accumulate_cases_kernel<CC>, dim3(grid), dim3(P3_THREADS), 0, s, logits, B, T, P0, P1, P2, tab, \
                       sum_overlap);                                                                                            \
    break;
  switch (C) {
    VX_ACC(2) VX_ACC(3) VX_ACC(4) VX_ACC(5) VX_ACC(6) VX_ACC(7) VX_ACC(8)
    default: break;
  }
#undef VX_ACC
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// K47 composite

struct p3_comp_item {
  const void* image;   // or null when data is null
  const float* count;
  double* data;
  double* gt_seg;
  uint8_t* gt;
  int64_t block0, n;   // first work block of the item; voxels
  int32_t kind, first_label, R, out;
};

struct p3_comp_label {
  const void* p;
  int32_t esl, sgn;   // log2 of the label's bytes; 1: signed elements
};

// the last entry whose block0 is not after blk (same for every thread of a workgroup)
__device__ __forceinline__ int p3_find(const p3_comp_item* __restrict__ items, int n, int64_t blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(P3_THREADS) void case_composite_kernel(const p3_comp_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                                    const p3_comp_label* __restrict__ labels, int32_t* __restrict__ status) {
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const p3_comp_item it = items[p3_find(items, n_items, blk)];
    const int64_t e = (blk - it.block0) * P3_CHUNK + (int64_t)threadIdx.x * 4;
    unsigned nbad = 0;
    if (e < it.n) {
      const int n = it.n - e < 4 ? (int)(it.n - e) : 4;
      float cnt[4];
      vx4_load<float>(it.count + e, n, cnt);
      double cl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) cl[u] = cnt[u] < 1.f ? 1.0 : (double)cnt[u];   // np.clip(num_predictions, 1, None)
      if (it.data) {
        double d[4], o[4];
        vx4_load_kind(it.image, it.kind, e, n, d);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          double s = 0.0;
          for (int k = 0; k < (int)cnt[u]; ++k) s += d[u];   // data[crop] += patch, once per covering patch
          o[u] = s / cl[u];
        }
        vx4_store<double>(it.data + e, n, o);
      }
      for (int r = 0; r < it.R; ++r) {
        const p3_comp_label lb = labels[it.first_label + r];
        int32_t lab[4];
        bool bad[4];
        vx4_load_label(lb.p, lb.esl, lb.sgn, e, n, lab, bad);
        double g[4];
        uint8_t g8[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          nbad += bad[u] ? 1u : 0u;
          uint32_t s = 0;                                    // the intc sum (wraps as numpy's does)
          for (int k = 0; k < (int)cnt[u]; ++k) s += (uint32_t)lab[u];
          g[u] = (double)(int32_t)s / cl[u];
          g8[u] = (uint8_t)(int32_t)g[u];                    // np.asarray(..., dtype=np.intc), narrowed
        }
        if (it.gt_seg) vx4_store<double>(it.gt_seg + (int64_t)r * it.n + e, n, g);
        if (it.gt) vx4_store<uint8_t>(it.gt + (int64_t)r * it.n + e, n, g8);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(&status[it.out], (int)nbad);
  }
}

static vx_staging g_comp_stage;

extern "C" int64_t vx_case_composite_workspace_bytes(int n_items, int n_labels) {
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS || n_labels < 0 || n_labels > VX_COMPOSITE_MAX_LABELS) return 0;
  return (int64_t)(vx_align256((size_t)n_items * sizeof(p3_comp_item)) + vx_align256((size_t)(n_labels > 0 ? n_labels : 1) * sizeof(p3_comp_label)));
}

extern "C" int vx_case_composite(const vx_composite_item* items, int n_items, const vx_composite_label* labels, int n_labels,
                                 int32_t* status, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_case_composite";
  if (!items) VX_FAIL(VX_E_NULL, "%s: null item table", who);
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) VX_FAIL(VX_E_SHAPE, "%s: n_items %d outside 1..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (n_labels < 0 || n_labels > VX_COMPOSITE_MAX_LABELS) VX_FAIL(VX_E_SHAPE, "%s: n_labels %d outside 0..%d", who, n_labels, VX_COMPOSITE_MAX_LABELS);
  if (n_labels > 0 && !labels) VX_FAIL(VX_E_NULL, "%s: null label table", who);
  std::vector<p3_comp_item> table((size_t)n_items);
  std::vector<p3_comp_label> ltab((size_t)(n_labels > 0 ? n_labels : 1));
  ltab[0] = p3_comp_label{};
  for (int l = 0; l < n_labels; ++l) {
    if (labels[l].kind < VX_COUNT_B1 || labels[l].kind > VX_COUNT_B8) VX_FAIL(VX_E_DTYPE, "%s: label %d: kind %d", who, l, labels[l].kind);
    if (!labels[l].ptr) VX_FAIL(VX_E_NULL, "%s: label %d: null pointer", who, l);
    if ((uintptr_t)labels[l].ptr % (1u << labels[l].kind)) VX_FAIL(VX_E_ALIGN, "%s: label %d: not aligned to its %d-byte elements", who, l, 1 << labels[l].kind);
    if (labels[l].flags & ~VX_LABEL_SIGNED) VX_FAIL(VX_E_DTYPE, "%s: label %d: flags %d", who, l, labels[l].flags);
    ltab[(size_t)l].p = labels[l].ptr; ltab[(size_t)l].esl = labels[l].kind; ltab[(size_t)l].sgn = labels[l].flags & VX_LABEL_SIGNED;
  }
  int64_t n_blocks = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_composite_item& it = items[i];
    for (int a = 0; a < 3; ++a)
      if (it.dims[a] < 1) VX_FAIL(VX_E_SHAPE, "%s: item %d: dims[%d] = %d", who, i, a, it.dims[a]);
    const int64_t n = (int64_t)it.dims[0] * it.dims[1] * it.dims[2];
    if (n > (1ll << 40)) VX_FAIL(VX_E_SHAPE, "%s: item %d: more than 2^40 voxels", who, i);
    if (it.R < 0 || it.first_label < 0 || (int64_t)it.first_label + it.R > n_labels)
      VX_FAIL(VX_E_SHAPE, "%s: item %d: labels [%d, %lld) outside the table of %d", who, i, it.first_label, (long long)it.first_label + it.R, n_labels);
    if (!it.count) VX_FAIL(VX_E_NULL, "%s: item %d: null count", who, i);
    if ((uintptr_t)it.count % sizeof(float)) VX_FAIL(VX_E_ALIGN, "%s: item %d: count not aligned to float", who, i);
    if (it.data) {
      const int es = p3_esize(it.image_kind);
      if (!es) VX_FAIL(VX_E_DTYPE, "%s: item %d: image kind %d", who, i, it.image_kind);
      if (!it.image) VX_FAIL(VX_E_NULL, "%s: item %d: data without an image", who, i);
      if ((uintptr_t)it.image % es) VX_FAIL(VX_E_ALIGN, "%s: item %d: image not aligned to its %d-byte elements", who, i, es);
    }
    if ((uintptr_t)it.data % sizeof(double) || (uintptr_t)it.gt_seg % sizeof(double))
      VX_FAIL(VX_E_ALIGN, "%s: item %d: data or gt_seg not aligned to double", who, i);
    p3_comp_item& d = table[(size_t)i];
    d.image = it.image; d.count = it.count; d.data = it.data; d.gt_seg = it.gt_seg; d.gt = it.gt;
    d.block0 = n_blocks; d.n = n; d.kind = it.image_kind; d.first_label = it.first_label; d.R = it.R; d.out = i;
    n_blocks += (n + P3_CHUNK - 1) / P3_CHUNK;
  }
  if (!status || !workspace) VX_FAIL(VX_E_NULL, "%s: null status or workspace", who);
  if (ws_bytes < vx_case_composite_workspace_bytes(n_items, n_labels))
    VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)vx_case_composite_workspace_bytes(n_items, n_labels));
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)n_items * sizeof(int32_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "%s: memset: %s", who, hipGetErrorString(e));
  const size_t lab_off = vx_align256(table.size() * sizeof(p3_comp_item));
  const vx_stage_part parts[2] = {{table.data(), table.size() * sizeof(p3_comp_item), 0},
                                  {ltab.data(), ltab.size() * sizeof(p3_comp_label), lab_off}};
  const int up = vx_staged_upload(g_comp_stage, who, parts, 2, lab_off + parts[1].bytes, workspace, s);
  if (up != VX_OK) return up;
  const int grid = (int)(n_blocks < P3_MAX_GRID ? n_blocks : P3_MAX_GRID);
  hipLaunchKernelGGL(case_composite_kernel, dim3(grid), dim3(P3_THREADS), 0, s, (const p3_comp_item*)workspace, n_items, n_blocks,
                     (const p3_comp_label*)((const char*)workspace + lab_off), status);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
