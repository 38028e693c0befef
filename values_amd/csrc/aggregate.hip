// K38: the map -> scalar aggregations of evaluation/uncertainty_aggregation/aggregate_uncertainties.py:13-67
// (patch_level_aggregation, image_level_aggregation, threshold_aggregation) for a batch of maps in one call;
// one map is a batch of one.
//   vx_aggregate_batched: every IMAGE / THRESHOLD spec of an item from ONE read of its map (agg_sums_kernel, one
//     workgroup of 1024 threads per item), every PATCH spec from separable box sums on LDS tiles (agg_box_kernel: tile
//     maxima, then the first index close to the item's maximum in the tiles that can hold one) and a per-pair finish
//     (agg_box_finish_kernel: minimum index, unravel, store).
// Every value is a float64 formed in the order include/values_amd.h documents for K38 (stated again at the kernels below),
// so the results do not depend on the batch, the tiling or the chunking.  At most four launches per call, whatever n_items
// and n_specs are; no atomics; nothing but the descriptor upload touches the host.
#include "aggregate_plan.h"
#include "common.h"
#include "staging.h"

// the IMAGE / THRESHOLD specs of a call, by value: thr[j] is the j-th distinct THRESHOLD spec, slot[s] its j for spec s
struct agg_sum_specs {
  int32_t n_specs, n_thr;
  int32_t kind[VX_AGG_MAX_SPECS];
  int32_t slot[VX_AGG_MAX_SPECS];
  double thr[VX_AGG_MAX_SPECS];
};

struct agg_acc {
  double s;
  double st[VX_AGG_MAX_SPECS], ct[VX_AGG_MAX_SPECS];
};

// (every loop over the thresholds is unrolled with constant bounds: st / ct stay in registers)
__device__ __forceinline__ void agg_add(agg_acc& a, double x, const double (&thr)[VX_AGG_MAX_SPECS], int n_thr) {
  a.s += x;
#pragma unroll
  for (int t = 0; t < VX_AGG_MAX_SPECS; ++t)
    if (t < n_thr && x >= thr[t]) { a.st[t] += x; a.ct[t] += 1.0; }
}

// element i to thread i % 1024, each thread adding its elements in ascending i from 0.0; eight loads in flight per thread
template <typename T>
__device__ __forceinline__ void agg_accumulate(agg_acc& a, const T* __restrict__ v, int64_t n, int tid,
                                               const double (&thr)[VX_AGG_MAX_SPECS], int n_thr) {
  int64_t i = tid;
  for (; i + 7 * 1024 < n; i += 8 * 1024) {
    T x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = v[i + k * 1024];
#pragma unroll
    for (int k = 0; k < 8; ++k) agg_add(a, (double)x[k], thr, n_thr);
  }
  for (; i < n; i += 1024) agg_add(a, (double)v[i], thr, n_thr);
}

// The comparison runs in float64 on both sides: the reference compares the stored map (float64 when it was read back
// from NIfTI) with a float64 threshold (aggregate_uncertainties.py:61-66); a float32 threshold could move voxels within
// one float32 ulp of it across the >= boundary.  After the per-thread sums: in every wave the xor butterfly
// v += v[lane ^ off] for off = 1, 2, ..., 32, then the 16 wave partials added in wave order from 0.0.
__global__ __launch_bounds__(1024) void agg_sums_kernel(const agg_sum_item* __restrict__ items, agg_sum_specs sp, double* __restrict__ out) {
  __shared__ double s_red[1 + 2 * VX_AGG_MAX_SPECS][16];
  __shared__ int s_kind[VX_AGG_MAX_SPECS], s_slot[VX_AGG_MAX_SPECS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const agg_sum_item it = items[blockIdx.x];
  double thr[VX_AGG_MAX_SPECS];
#pragma unroll
  for (int t = 0; t < VX_AGG_MAX_SPECS; ++t) thr[t] = sp.thr[t];
  if (tid == 0) {
#pragma unroll
    for (int t = 0; t < VX_AGG_MAX_SPECS; ++t) { s_kind[t] = sp.kind[t]; s_slot[t] = sp.slot[t]; }
  }
  const int n_thr = sp.n_thr;
  agg_acc a;
  a.s = 0.0;
#pragma unroll
  for (int t = 0; t < VX_AGG_MAX_SPECS; ++t) { a.st[t] = 0.0; a.ct[t] = 0.0; }
  if (it.dtype == VX_F64) agg_accumulate(a, (const double*)it.map, it.n, tid, thr, n_thr);
  else agg_accumulate(a, (const float*)it.map, it.n, tid, thr, n_thr);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    a.s += __shfl_xor(a.s, off, 64);
#pragma unroll
    for (int t = 0; t < VX_AGG_MAX_SPECS; ++t)
      if (t < n_thr) { a.st[t] += __shfl_xor(a.st[t], off, 64); a.ct[t] += __shfl_xor(a.ct[t], off, 64); }
  }
  if (lane == 0) {
    s_red[0][wave] = a.s;
#pragma unroll
    for (int t = 0; t < VX_AGG_MAX_SPECS; ++t)
      if (t < n_thr) { s_red[1 + 2 * t][wave] = a.st[t]; s_red[2 + 2 * t][wave] = a.ct[t]; }
  }
  __syncthreads();
  if (tid < sp.n_specs && s_kind[tid] != VX_AGG_PATCH) {
    const int row = s_kind[tid] == VX_AGG_IMAGE ? 0 : 1 + 2 * s_slot[tid];
    double t0 = 0.0, t1 = 0.0;
    for (int w = 0; w < 16; ++w) t0 += s_red[row][w];
    if (row > 0)
      for (int w = 0; w < 16; ++w) t1 += s_red[row + 1][w];
    double* o = out + ((int64_t)blockIdx.x * sp.n_specs + tid) * 4;
    o[0] = t0; o[1] = t1; o[2] = 0.0; o[3] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Box sums of one tile: TD output slices x TH rows x TW columns of one (item, PATCH spec) pair.  The workgroup walks the
// TD + pd - 1 input slices of the tile; per slice it loads the (TH + ph - 1) x (TW + pw - 1) input rows as floats, sums
// along W into doubles, along H into the ring slot of the slice, and (from slice pd - 1 on) along D over the ring in
// ascending slice order.  Every sum starts from 0.0 and adds its p terms in ascending k (an axis with p = 1 keeps its
// 0.0 + x), so a box sum has the same bits whatever tile it falls in.
__device__ __forceinline__ double agg_block_max(double m, double* s_d) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) m = fmax(m, __shfl_xor(m, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmax(fmax(s_d[0], s_d[1]), fmax(s_d[2], s_d[3]));
}

__device__ __forceinline__ long long agg_block_min(long long f, long long* s_i) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long o = __shfl_xor(f, off, 64);
    f = o < f ? o : f;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_i[threadIdx.x >> 6] = f;
  __syncthreads();
  const long long a = s_i[0] < s_i[1] ? s_i[0] : s_i[1], b = s_i[2] < s_i[3] ? s_i[2] : s_i[3];
  return a < b ? a : b;
}

#define AGG_NO_INDEX 0x7fffffffffffffffLL

template <bool SECOND>
__global__ __launch_bounds__(VX_AGG_THREADS) void agg_box_kernel(const agg_pair* __restrict__ pairs, int n_pairs,
                                                                 double* __restrict__ tmax, long long* __restrict__ first) {
  extern __shared__ __attribute__((aligned(16))) unsigned char agg_smem[];
  __shared__ double s_d[4];
  __shared__ long long s_i[4];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  int lo = 0, hi = n_pairs - 1;          // the last pair whose first tile is not after this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const agg_pair q = pairs[lo];
  const int n_tiles = q.ntd * q.nth * q.ntw;
  double g = 0.0, tol = 0.0;
  if (SECOND) {
    double m = -INFINITY;
    for (int t = tid; t < n_tiles; t += VX_AGG_THREADS) m = fmax(m, tmax[q.tile0 + t]);
    g = agg_block_max(m, s_d);
    tol = 1e-8 + 1e-5 * fabs(g);
    // every box sum of a tile is <= its maximum <= g, so a tile whose maximum is not close holds no close element
    if (!(fabs(tmax[tile] - g) <= tol)) {
      if (tid == 0) first[tile] = AGG_NO_INDEX;
      return;
    }
  }
  const int t = (int)(tile - q.tile0);
  const int tw = t % q.ntw, th = (t / q.ntw) % q.nth, td = t / (q.ntw * q.nth);
  const int TW = 1 << q.tw_log2;
  const int d0 = td * q.TD, h0 = th * q.TH, w0 = tw * TW;
  const int nd = min(q.TD, q.od - d0), nh = min(q.TH, q.oh - h0), nw = min(TW, q.ow - w0);
  const int IH = nh + q.ph - 1, IW = nw + q.pw - 1;
  const int in_stride = TW + q.pw - 1;
  float* s_in = (float*)agg_smem;
  double* s_ws = (double*)(agg_smem + (((size_t)(q.TH + q.ph - 1) * in_stride * sizeof(float) + 255) & ~(size_t)255));
  double* s_ring = s_ws + (size_t)(q.TH + q.ph - 1) * TW;
  const int slice = q.TH * TW;
  const bool f64 = q.dtype == VX_F64;

  double m = -INFINITY;
  long long fi = AGG_NO_INDEX;
  int slot = 0;                                            // ring slot of input slice s: s % pd
  for (int s = 0; s < nd + q.pd - 1; ++s) {
    const int64_t base = ((int64_t)(d0 + s) * q.H + h0) * q.W + w0;
    for (int i = tid; i < IH * IW; i += VX_AGG_THREADS) {
      const int r = i / IW, c = i - r * IW;
      const int64_t a = base + (int64_t)r * q.W + c;
      s_in[r * in_stride + c] = f64 ? (float)((const double*)q.map)[a] : ((const float*)q.map)[a];   // a float64 map is narrowed first
    }
    __syncthreads();
    for (int i = tid; i < (IH << q.tw_log2); i += VX_AGG_THREADS) {
      const int r = i >> q.tw_log2, c = i & (TW - 1);
      if (c < nw) {
        const float* src = s_in + r * in_stride + c;
        double v = 0.0;
        for (int k = 0; k < q.pw; ++k) v += (double)src[k];
        s_ws[i] = v;
      }
    }
    __syncthreads();
    // a thread sums along H and along D for the same (row, column) cells in every slice: it reads only its own ring entries
    const int oldest = slot + 1 == q.pd ? 0 : slot + 1;    // ring slot of input slice s - (pd - 1)
    for (int i = tid; i < (nh << q.tw_log2); i += VX_AGG_THREADS) {
      const int r = i >> q.tw_log2, c = i & (TW - 1);
      if (c < nw) {
        double hs = 0.0;
        for (int k = 0; k < q.ph; ++k) hs += s_ws[i + (k << q.tw_log2)];
        double v = 0.0;
        if (q.pd == 1) {
          v += hs;
        } else {
          s_ring[slot * slice + i] = hs;
          if (s >= q.pd - 1) {
            int j = oldest;
            for (int k = 0; k < q.pd; ++k) {
              v += s_ring[j * slice + i];
              j = j + 1 == q.pd ? 0 : j + 1;
            }
          }
        }
        if (s >= q.pd - 1) {
          if (!SECOND) m = fmax(m, v);
          else if (fabs(v - g) <= tol) {
            const long long gi = ((long long)(d0 + s - (q.pd - 1)) * q.oh + (h0 + r)) * q.ow + (w0 + c);
            fi = gi < fi ? gi : fi;
          }
        }
      }
    }
    slot = oldest;
    // (the next slice's loads wait at its first barrier for every thread to leave this loop; s_ws is rewritten after it)
  }
  if (!SECOND) {
    m = agg_block_max(m, s_d);
    if (tid == 0) tmax[tile] = m;
  } else {
    fi = agg_block_min(fi, s_i);
    if (tid == 0) first[tile] = fi;
  }
}

// one wave per pair: the item's maximum, the lowest close index, its (d, h, w), stored as exact integers in doubles
__global__ __launch_bounds__(64) void agg_box_finish_kernel(const agg_pair* __restrict__ pairs, const double* __restrict__ tmax,
                                                            const long long* __restrict__ first, double* __restrict__ out) {
  const agg_pair q = pairs[blockIdx.x];
  const int n_tiles = q.ntd * q.nth * q.ntw;
  double m = -INFINITY;
  long long f = AGG_NO_INDEX;
  for (int t = threadIdx.x; t < n_tiles; t += 64) {
    m = fmax(m, tmax[q.tile0 + t]);
    const long long o = first[q.tile0 + t];
    f = o < f ? o : f;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    m = fmax(m, __shfl_xor(m, off, 64));
    const long long o = __shfl_xor(f, off, 64);
    f = o < f ? o : f;
  }
  if (threadIdx.x == 0) {
    double* o = out + (int64_t)q.out_index * 4;
    o[0] = m;
    o[1] = (double)(f / ((long long)q.oh * q.ow));
    o[2] = (double)((f / q.ow) % q.oh);
    o[3] = (double)(f % q.ow);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The two tables go up through the pinned staging buffer of staging.h: no wait on the stream.
static vx_staging g_stage;

static int agg_upload(const agg_plan& p, void* workspace, hipStream_t s) {
  const vx_stage_part parts[2] = {{p.sums.data(), p.sums.size() * sizeof(agg_sum_item), 0},
                                  {p.pairs.data(), p.pairs.size() * sizeof(agg_pair), p.off_pairs}};
  return vx_staged_upload(g_stage, "vx_aggregate_batched", parts, 2, p.off_tmax, workspace, s);
}

extern "C" size_t vx_aggregate_workspace_bytes(const vx_agg_item* items, int n_items, const vx_agg_spec* specs, int n_specs) {
  agg_plan p;
  return agg_make_plan(items, n_items, specs, n_specs, &p) == VX_OK ? p.bytes : 0;
}

extern "C" int vx_aggregate_batched(const vx_agg_item* items, int n_items, const vx_agg_spec* specs, int n_specs, double* out,
                                    void* workspace, size_t workspace_bytes, vx_stream_t stream) {
  agg_plan p;
  const int rc = agg_make_plan(items, n_items, specs, n_specs, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if (!out || !workspace) VX_FAIL(VX_E_NULL, "vx_aggregate_batched: null out or workspace");
  if (workspace_bytes < p.bytes) VX_FAIL(VX_E_WORKSPACE, "vx_aggregate_batched: workspace needs %zu bytes", p.bytes);
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "vx_aggregate_batched: workspace not 16-byte aligned");
  if (p.tiles > 0x7fffffffLL) VX_FAIL(VX_E_SHAPE, "vx_aggregate_batched: %lld tiles in one call", (long long)p.tiles);
  hipStream_t s = (hipStream_t)stream;
  const int up = agg_upload(p, workspace, s);
  if (up != VX_OK) return up;
  char* ws = (char*)workspace;
  if (p.any_sum) {
    agg_sum_specs sp;
    memset(&sp, 0, sizeof(sp));
    sp.n_specs = n_specs;
    for (int i = 0; i < n_specs; ++i) {
      sp.kind[i] = specs[i].kind;
      if (specs[i].kind == VX_AGG_THRESHOLD) { sp.slot[i] = sp.n_thr; sp.thr[sp.n_thr++] = specs[i].thr; }
    }
    hipLaunchKernelGGL(agg_sums_kernel, dim3(n_items), dim3(1024), 0, s, (const agg_sum_item*)ws, sp, out);
  }
  if (!p.pairs.empty()) {
    const agg_pair* pairs = (const agg_pair*)(ws + p.off_pairs);
    double* tmax = (double*)(ws + p.off_tmax);
    long long* first = (long long*)(ws + p.off_first);
    if (p.lds > (size_t)VX_AGG_LDS_SHARED) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(agg_box_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
      if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(agg_box_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
      if (e != hipSuccess) VX_FAIL((int)e, "vx_aggregate_batched: hipFuncSetAttribute(%zu B LDS): %s", p.lds, hipGetErrorString(e));
    }
    const int n_pairs = (int)p.pairs.size();
    hipLaunchKernelGGL(agg_box_kernel<false>, dim3((unsigned)p.tiles), dim3(VX_AGG_THREADS), p.lds, s, pairs, n_pairs, tmax, first);
    hipLaunchKernelGGL(agg_box_kernel<true>, dim3((unsigned)p.tiles), dim3(VX_AGG_THREADS), p.lds, s, pairs, n_pairs, tmax, first);
    hipLaunchKernelGGL(agg_box_finish_kernel, dim3(n_pairs), dim3(64), 0, s, pairs, tmax, first, out);
  }
  VX_CHECK_LAUNCH("vx_aggregate_batched");
  return VX_OK;
}
