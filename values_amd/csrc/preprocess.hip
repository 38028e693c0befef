// K41: preprocessing of a 3D data set (datasets/preprocess_datasets_3d.py:135-168) for a batch of raw volumes and labels
// (DESIGN 4.48).
//   vx_volume_stats_batched: {mean, std, min, n} of every item, as numpy computes them on the data widened to float64.
//     Two passes like np.std: sum and minimum, then the squared deviations from the mean of pass one.  An item is cut
//     into work blocks of 32 KB from its first element (prep_plan.h); the blocks of all items are taken in turn by one
//     grid, the way select.hip deals its blocks.  A thread adds its eight 16-byte chunks in order, the 64 lanes of a
//     wave fold by butterfly, thread 0 adds the four waves in order, and the block's partial goes to the block's own slot:
//     which workgroup computed it does not matter.  One workgroup per item then adds the item's partials: thread t the
//     t-th run of consecutive blocks, thread 0 the 256 runs in order.  Every order depends on the item's own n and kind
//     only, so the four numbers are bit-equal alone or in any batch, at any position, on any grid.  Integer kinds sum in
//     int64 (exact) and convert once.
//   vx_zscore_pad_batched: the fused normalise-and-pad pass.  The OUTPUT is cut into 32 KB work blocks over all items;
//     lanes run along z; a thread produces the 16 / sizeof(out) elements of a 16-byte chunk and stores them at once.  The
//     chunk's source run is one load where it lies in one source row, the per-element walk where it crosses a row end
//     or a padding slab.  (double(x) - mean) / (std + 1e-8) with a true float64 division, rounded once to the output.
// Plain C++ stores only, no atomics.  Both calls upload their item table through the pinned staging buffer of staging.h:
// no wait on the stream, not capturable into a hipGraph.  The file is compiled with -ffp-contract=off (Makefile) and says
// so again below: x - mean, its square and the sum stay three roundings.
#include <type_traits>

#include "common.h"
#include "prep_plan.h"
#include "staging.h"

#pragma clang fp contract(off)

#define PP_PER_THREAD (PP_BLOCK_CHUNKS / PP_THREADS)

// the last entry whose block0 is not after blk (same for every thread of a workgroup)
template <typename T>
__device__ __forceinline__ int pp_find(const T* __restrict__ items, int n, int64_t blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// PER consecutive elements: one load where the address allows it
template <typename S, int PER>
__device__ __forceinline__ void pp_load_run(const S* __restrict__ p, S (&v)[PER]) {
  constexpr int B = PER * (int)sizeof(S), A = B < 16 ? B : 16;
  if (((uintptr_t)p & (uintptr_t)(A - 1)) == 0) {
    __builtin_memcpy(v, __builtin_assume_aligned(p, A), B);
  } else {
#pragma unroll
    for (int t = 0; t < PER; ++t) v[t] = p[t];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// statistics

struct pp_acc {
  double s;        // float kinds: sum (pass 1); all kinds: sum of squared deviations (pass 2)
  double mn;
  long long is;    // integer kinds: sum and minimum (pass 1)
  long long imn;
  int nan;
};

template <typename T, int PASS>
__device__ __forceinline__ void st_add(T v, double mean, pp_acc& a) {
  if (PASS == 0) {
    if (std::is_integral<T>::value) {
      const long long x = (long long)v;
      a.is += x;
      a.imn = x < a.imn ? x : a.imn;
    } else {
      const double x = (double)v;
      a.s += x;
      a.nan |= x != x;
      a.mn = x < a.mn ? x : a.mn;
    }
  } else {
    const double d = (double)v - mean;
    const double q = d * d;
    a.s += q;
  }
}

// A thread adds the elements of its chunks tid, tid + 256, ... of the block, in that order.  Two ways to read them, one
// order of adding: a whole block behind a 16-byte aligned pointer loads its eight chunks first, one 16-byte load each;
// an item's last block and an item off 16 bytes go element by element.
template <typename T, int PASS>
__device__ __forceinline__ void st_block(const pp_stat_item& it, int64_t lb, int tid, double mean, pp_acc& a) {
  constexpr int PER = 16 / (int)sizeof(T);
  const T* __restrict__ p = (const T*)it.p;
  const int64_t c0 = lb * PP_BLOCK_CHUNKS + tid;
  if ((((uintptr_t)p) & 15) == 0 && (lb + 1) * (int64_t)(PP_BLOCK_CHUNKS * PER) <= it.n) {
    uint4 w[PP_PER_THREAD];
#pragma unroll
    for (int u = 0; u < PP_PER_THREAD; ++u) w[u] = *reinterpret_cast<const uint4*>(p + (c0 + (int64_t)u * PP_THREADS) * PER);
#pragma unroll
    for (int u = 0; u < PP_PER_THREAD; ++u) {
      T v[PER];
      __builtin_memcpy(v, &w[u], 16);
#pragma unroll
      for (int t = 0; t < PER; ++t) st_add<T, PASS>(v[t], mean, a);
    }
    return;
  }
#pragma unroll 1
  for (int u = 0; u < PP_PER_THREAD; ++u) {
    const int64_t e0 = (c0 + (int64_t)u * PP_THREADS) * PER;
#pragma unroll 1
    for (int t = 0; t < PER; ++t)
      if (e0 + t < it.n) st_add<T, PASS>(p[e0 + t], mean, a);
  }
}

template <int PASS>
__global__ __launch_bounds__(PP_THREADS) void stats_partial_kernel(const pp_stat_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                                   const double* __restrict__ stats, pp_partial* __restrict__ part) {
  __shared__ double s_s[PP_THREADS / 64], s_mn[PP_THREADS / 64];
  __shared__ long long s_is[PP_THREADS / 64], s_imn[PP_THREADS / 64];
  __shared__ int s_nan[PP_THREADS / 64];
  const int tid = threadIdx.x;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int idx = pp_find(items, n_items, blk);
    const pp_stat_item it = items[idx];
    const int64_t lb = blk - it.block0;
    const double mean = PASS == 1 ? stats[(int64_t)idx * 4] : 0.0;
    pp_acc a;
    a.s = 0.0; a.mn = __builtin_huge_val(); a.is = 0; a.imn = 0x7fffffffffffffffLL; a.nan = 0;
    switch (it.kind) {
      case VX_PREP_U8: st_block<uint8_t, PASS>(it, lb, tid, mean, a); break;
      case VX_PREP_I8: st_block<int8_t, PASS>(it, lb, tid, mean, a); break;
      case VX_PREP_U16: st_block<uint16_t, PASS>(it, lb, tid, mean, a); break;
      case VX_PREP_I16: st_block<int16_t, PASS>(it, lb, tid, mean, a); break;
      case VX_PREP_U32: st_block<uint32_t, PASS>(it, lb, tid, mean, a); break;
      case VX_PREP_I32: st_block<int32_t, PASS>(it, lb, tid, mean, a); break;
      case VX_PREP_F32: st_block<float, PASS>(it, lb, tid, mean, a); break;
      default: st_block<double, PASS>(it, lb, tid, mean, a); break;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a.s += __shfl_xor(a.s, off, 64);
      if (PASS == 0) {
        const double om = __shfl_xor(a.mn, off, 64);
        a.mn = om < a.mn ? om : a.mn;
        a.is += __shfl_xor(a.is, off, 64);
        const long long oi = __shfl_xor(a.imn, off, 64);
        a.imn = oi < a.imn ? oi : a.imn;
        a.nan |= __shfl_xor(a.nan, off, 64);
      }
    }
    __syncthreads();   // (the previous block's LDS words have been read)
    if ((tid & 63) == 0) {
      s_s[tid >> 6] = a.s;
      if (PASS == 0) { s_mn[tid >> 6] = a.mn; s_is[tid >> 6] = a.is; s_imn[tid >> 6] = a.imn; s_nan[tid >> 6] = a.nan; }
    }
    __syncthreads();
    if (tid == 0) {
      double s = s_s[0];
      for (int w = 1; w < PP_THREADS / 64; ++w) s += s_s[w];
      if (PASS == 0) {
        double mn = s_mn[0];
        long long is = s_is[0], imn = s_imn[0];
        int nan = s_nan[0];
        for (int w = 1; w < PP_THREADS / 64; ++w) {
          mn = s_mn[w] < mn ? s_mn[w] : mn;
          is += s_is[w];
          imn = s_imn[w] < imn ? s_imn[w] : imn;
          nan |= s_nan[w];
        }
        pp_partial o;
        o.s = s; o.mn = it.kind < VX_PREP_F32 ? (double)imn : mn; o.is = is; o.nan = nan; o.pad = 0;
        part[blk] = o;
      } else {
        part[blk].s = s;
      }
    }
  }
}

// one workgroup per item: thread t adds the t-th run of consecutive block partials, thread 0 the runs in order
template <int PASS>
__global__ __launch_bounds__(PP_THREADS) void stats_final_kernel(const pp_stat_item* __restrict__ items, const pp_partial* __restrict__ part,
                                                                 double* __restrict__ stats) {
  __shared__ double s_s[PP_THREADS], s_mn[PP_THREADS];
  __shared__ long long s_is[PP_THREADS];
  __shared__ int s_nan[PP_THREADS];
  const int tid = threadIdx.x;
  const pp_stat_item it = items[blockIdx.x];
  const int64_t run = (it.n_blocks + PP_THREADS - 1) / PP_THREADS;
  const int64_t b0 = (int64_t)tid * run, b1 = b0 + run < it.n_blocks ? b0 + run : it.n_blocks;
  double s = 0.0, mn = __builtin_huge_val();
  long long is = 0;
  int nan = 0;
  for (int64_t b = b0; b < b1; ++b) {
    const pp_partial q = part[it.block0 + b];
    s += q.s;
    if (PASS == 0) { mn = q.mn < mn ? q.mn : mn; is += q.is; nan |= q.nan; }
  }
  s_s[tid] = s;
  if (PASS == 0) { s_mn[tid] = mn; s_is[tid] = is; s_nan[tid] = nan; }
  __syncthreads();
  if (tid != 0) return;
  const int used = (int)((it.n_blocks + run - 1) / run);   // threads that had blocks
  for (int t = 1; t < used; ++t) {
    s += s_s[t];
    if (PASS == 0) { mn = s_mn[t] < mn ? s_mn[t] : mn; is += s_is[t]; nan |= s_nan[t]; }
  }
  double* o = stats + (int64_t)blockIdx.x * 4;
  const double n = (double)it.n;
  if (PASS == 0) {
    const double total = it.kind < VX_PREP_F32 ? (double)is : s;
    o[0] = total / n;
    o[2] = nan ? __builtin_nan("") : mn;
    o[3] = n;
  } else {
    o[1] = sqrt(s / n);
  }
}

static vx_staging g_stat_stage, g_pad_stage;

extern "C" int64_t vx_volume_stats_batched_workspace_bytes(const vx_prep_item* items, int n_items) {
  pp_plan p;
  if (pp_plan_stats(items, n_items, &p) != VX_OK) return 0;
  return (int64_t)p.bytes;
}

extern "C" int vx_volume_stats_batched(const vx_prep_item* items, int n_items, double* stats, void* workspace, int64_t ws_bytes,
                                       vx_stream_t stream) {
  const char* who = "vx_volume_stats_batched";
  pp_plan p;
  const int rc = pp_plan_stats(items, n_items, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if (n_items == 0) return VX_OK;
  if (!stats || !workspace) VX_FAIL(VX_E_NULL, "%s: null stats or workspace", who);
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  if (((uintptr_t)stats & 7) != 0) VX_FAIL(VX_E_ALIGN, "%s: stats not aligned to its 8-byte elements", who);
  if (ws_bytes < (int64_t)p.bytes) VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)p.bytes);
  hipStream_t s = (hipStream_t)stream;
  const vx_stage_part up = {p.stat.data(), p.stat.size() * sizeof(pp_stat_item), 0};
  const int urc = vx_staged_upload(g_stat_stage, who, &up, 1, up.bytes, workspace, s);
  if (urc != VX_OK) return urc;
  const pp_stat_item* table = (const pp_stat_item*)workspace;
  pp_partial* part = (pp_partial*)((char*)workspace + p.off_partial);
  const dim3 grid((unsigned)(p.n_blocks < PP_MAX_GRID ? p.n_blocks : PP_MAX_GRID)), wg(PP_THREADS), per_item((unsigned)n_items);
  hipLaunchKernelGGL(stats_partial_kernel<0>, grid, wg, 0, s, table, n_items, p.n_blocks, (const double*)stats, part);
  hipLaunchKernelGGL(stats_final_kernel<0>, per_item, wg, 0, s, table, (const pp_partial*)part, stats);
  hipLaunchKernelGGL(stats_partial_kernel<1>, grid, wg, 0, s, table, n_items, p.n_blocks, (const double*)stats, part);
  hipLaunchKernelGGL(stats_final_kernel<1>, per_item, wg, 0, s, table, (const pp_partial*)part, stats);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// normalise and pad

template <typename S, typename O, bool Z>
__device__ __forceinline__ O pp_value(S x, double mean, double den) {
  if (Z) {
    const double d = (double)x - mean;
    return (O)(d / den);
  }
  return (O)x;
}

template <typename S, typename O, bool Z>
__device__ __forceinline__ void pad_block(const pp_pad_item& it, int64_t lb, int tid, const double* __restrict__ st) {
  constexpr int PER = 16 / (int)sizeof(O);
  const double mean = st[0], den = st[1] + 1e-8, mn = st[2];
  const O fill = Z ? (O)((mn - mean) / den) : (O)mn;
  const S* __restrict__ src = (const S*)it.src;
  O* __restrict__ dst = (O*)it.dst;
  const bool dst_vec = ((uintptr_t)dst & 15) == 0;
  const int o1 = it.o[1], o2 = it.o[2];
  const int64_t plane = (int64_t)o1 * o2;
  const bool small = it.out_n <= 0xFFFFFFFFLL;   // 32-bit index arithmetic (uniform per item)
  const int64_t c0 = lb * PP_BLOCK_CHUNKS + tid;
#pragma unroll 2
  for (int u = 0; u < PP_PER_THREAD; ++u) {
    const int64_t e0 = (c0 + (int64_t)u * PP_THREADS) * PER;
    if (e0 >= it.out_n) break;
    int x, y, z;
    if (small) {
      const uint32_t e = (uint32_t)e0, pl = (uint32_t)plane;
      const uint32_t xx = e / pl, r = e - xx * pl, yy = r / (uint32_t)o2;
      x = (int)xx; y = (int)yy; z = (int)(r - yy * (uint32_t)o2);
    } else {
      const int64_t xx = e0 / plane, r = e0 - xx * plane, yy = r / o2;
      x = (int)xx; y = (int)yy; z = (int)(r - yy * o2);
    }
    O r[PER];
    const int xs = x - it.lo[0], ys = y - it.lo[1], zs = z - it.lo[2];
    if ((unsigned)xs < (unsigned)it.d[0] && (unsigned)ys < (unsigned)it.d[1] && zs >= 0 && zs + PER <= it.d[2]) {
      // the whole chunk lies in one source row (and so in one output row: lo[2] + d[2] <= o[2])
      S v[PER];
      pp_load_run<S, PER>(src + ((int64_t)xs * it.d[1] + ys) * it.d[2] + zs, v);
#pragma unroll
      for (int t = 0; t < PER; ++t) r[t] = pp_value<S, O, Z>(v[t], mean, den);
    } else {
      // a row end, a padding slab or the item's end inside the chunk: element by element.  Past the item's last
      // element x reaches o[0], which is outside the source box: nothing is read there.
#pragma unroll
      for (int t = 0; t < PER; ++t) {
        const int xa = x - it.lo[0], ya = y - it.lo[1], za = z - it.lo[2];
        const bool in = (unsigned)xa < (unsigned)it.d[0] && (unsigned)ya < (unsigned)it.d[1] && (unsigned)za < (unsigned)it.d[2];
        r[t] = fill;
        if (in) r[t] = pp_value<S, O, Z>(src[((int64_t)xa * it.d[1] + ya) * it.d[2] + za], mean, den);
        if (++z == o2) {
          z = 0;
          if (++y == o1) { y = 0; ++x; }
        }
      }
    }
    if (dst_vec && e0 + PER <= it.out_n) {
      uint4 w;
      __builtin_memcpy(&w, r, 16);
      *reinterpret_cast<uint4*>(dst + e0) = w;
    } else {
#pragma unroll
      for (int t = 0; t < PER; ++t)
        if (e0 + t < it.out_n) dst[e0 + t] = r[t];
    }
  }
}

template <typename S>
__device__ __forceinline__ void pad_dispatch(const pp_pad_item& it, int64_t lb, int tid, const double* __restrict__ st) {
  if (it.mode == VX_PREP_COPY) pad_block<S, S, false>(it, lb, tid, st);
  else if (it.out == VX_F32) pad_block<S, float, true>(it, lb, tid, st);
  else pad_block<S, double, true>(it, lb, tid, st);
}

__global__ __launch_bounds__(PP_THREADS) void zscore_pad_kernel(const pp_pad_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                                const double* __restrict__ stats) {
  const int tid = threadIdx.x;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const pp_pad_item it = items[pp_find(items, n_items, blk)];
    const int64_t lb = blk - it.block0;
    const double* st = stats + (int64_t)it.row * 4;
    switch (it.kind) {
      case VX_PREP_U8: pad_dispatch<uint8_t>(it, lb, tid, st); break;
      case VX_PREP_I8: pad_dispatch<int8_t>(it, lb, tid, st); break;
      case VX_PREP_U16: pad_dispatch<uint16_t>(it, lb, tid, st); break;
      case VX_PREP_I16: pad_dispatch<int16_t>(it, lb, tid, st); break;
      case VX_PREP_U32: pad_dispatch<uint32_t>(it, lb, tid, st); break;
      case VX_PREP_I32: pad_dispatch<int32_t>(it, lb, tid, st); break;
      case VX_PREP_F32: pad_dispatch<float>(it, lb, tid, st); break;
      default: pad_dispatch<double>(it, lb, tid, st); break;
    }
  }
}

extern "C" int64_t vx_zscore_pad_batched_workspace_bytes(const vx_prep_pad_item* items, int n_items) {
  pp_plan p;
  if (pp_plan_pad(items, n_items, &p) != VX_OK) return 0;
  return (int64_t)p.bytes;
}

extern "C" int vx_zscore_pad_batched(const vx_prep_pad_item* items, int n_items, const double* stats, void* workspace, int64_t ws_bytes,
                                     vx_stream_t stream) {
  const char* who = "vx_zscore_pad_batched";
  pp_plan p;
  const int rc = pp_plan_pad(items, n_items, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if (n_items == 0) return VX_OK;
  if (!stats || !workspace) VX_FAIL(VX_E_NULL, "%s: null stats or workspace", who);
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  if (((uintptr_t)stats & 7) != 0) VX_FAIL(VX_E_ALIGN, "%s: stats not aligned to its 8-byte elements", who);
  if (ws_bytes < (int64_t)p.bytes) VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)p.bytes);
  hipStream_t s = (hipStream_t)stream;
  const vx_stage_part up = {p.pad.data(), p.pad.size() * sizeof(pp_pad_item), 0};
  const int urc = vx_staged_upload(g_pad_stage, who, &up, 1, up.bytes, workspace, s);
  if (urc != VX_OK) return urc;
  const dim3 grid((unsigned)(p.n_blocks < PP_MAX_GRID ? p.n_blocks : PP_MAX_GRID)), wg(PP_THREADS);
  hipLaunchKernelGGL(zscore_pad_kernel, grid, wg, 0, s, (const pp_pad_item*)workspace, n_items, p.n_blocks, stats);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
