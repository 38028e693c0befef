// K40: the threshold search (find_threshold.py:11-13, :63-68) for a whole reader batch / a whole split in one call each
// (DESIGN 4.40).
//   vx_count_nonzero_batched: np.count_nonzero of every item of a batch -- masks of any integer / bool / float type and any
//     size -- in ONE launch.  An item is cut into 16-byte aligned chunks, 1024 chunks make a work block, and the work
//     blocks of all items are dealt to the workgroups through the items' block0 prefix (the way aggregate.hip
//     deals its tiles): thousands of small 2D masks and a few large volumes share one grid.
//   vx_select_segments: the k-th and (k+1)-th smallest of the UNION of the items' elements (float32, or float64 narrowed
//     on load), where the reader left them: no concatenation, no cast copy.  MSB-first radix select over the
//     usual order-preserving map of IEEE floats to unsigned keys (negative: all bits flipped, non-negative: sign bit set, so
//     any finite input is handled) in three passes of 11, 11 and 10 bits; a pass builds its histogram in LDS and
//     folds it into 64-bit global bins, one workgroup then walks the bins to the one that holds rank k.  The last walk
//     knows how many keys equal the k-th and the rank of k among them: if another equal key remains the second order
//     statistic is the first, otherwise ONE more pass takes the minimum key above it (integer atomicMin).  That decision
//     is a flag in the state the pass reads: every workgroup leaves uniformly when it is not set, and the host never
//     waits between passes.  NaNs are detected in the first pass.  Integer arithmetic only: exact, and independent of
//     order and grid size.
// Plain C++ stores and integer atomics only.  Both calls upload their item table through the pinned staging buffer of
// staging.h: no wait on the stream, not capturable into a hipGraph.
#include <vector>

#include "common.h"
#include "staging.h"

#define SB_THREADS 256
#define SB_BLOCK_CHUNKS 1024   // 16-byte chunks per work block: four per thread
#define SB_MAX_GRID 2048

// ---------------------------------------------------------------------------------------------------------------
// the device tables: only the items that have elements, with the first work block of each
struct cnt_item {
  const uint8_t* p;   // first byte
  int64_t bytes;
  int64_t block0;
  int32_t kind, out;  // out: index of the item in the caller's array
};

struct seg_item {
  const void* p;      // first element
  int64_t n;
  int64_t block0;
  int32_t dtype, lead;  // lead: elements between the 16-byte boundary at or below p and p
};

// the last entry whose block0 is not after blk (same for every thread of a workgroup)
template <typename T>
__device__ __forceinline__ int sb_find(const T* __restrict__ items, int n, int64_t blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------
// counts

// non-zero elements among the 16 bytes of w; bytes outside the item are zero
__device__ __forceinline__ unsigned cnt_chunk(const uint4 w, int kind) {
  const unsigned x[4] = {w.x, w.y, w.z, w.w};
  unsigned c = 0;
  switch (kind) {
    case VX_COUNT_B1:
#pragma unroll
      for (int i = 0; i < 4; ++i) c += __popc((((x[i] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x[i]) & 0x80808080u);
      break;
    case VX_COUNT_B2:
#pragma unroll
      for (int i = 0; i < 4; ++i) c += __popc((((x[i] & 0x7fff7fffu) + 0x7fff7fffu) | x[i]) & 0x80008000u);
      break;
    case VX_COUNT_B4:
#pragma unroll
      for (int i = 0; i < 4; ++i) c += x[i] != 0u;
      break;
    case VX_COUNT_B8:
      c = ((x[0] | x[1]) != 0u) + ((x[2] | x[3]) != 0u);
      break;
    case VX_COUNT_F32:   // x != 0: any bit beside the sign (NaN counts, -0.0 does not)
#pragma unroll
      for (int i = 0; i < 4; ++i) c += (x[i] & 0x7fffffffu) != 0u;
      break;
    default:             // VX_COUNT_F64, little endian: the sign is bit 31 of the high word
      c = ((x[0] | (x[1] & 0x7fffffffu)) != 0u) + ((x[2] | (x[3] & 0x7fffffffu)) != 0u);
      break;
  }
  return c;
}

__global__ __launch_bounds__(SB_THREADS) void count_batched_kernel(const cnt_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                                   unsigned long long* __restrict__ counts) {
  __shared__ unsigned s_c[SB_THREADS / 64];
  const int tid = threadIdx.x;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const cnt_item it = items[sb_find(items, n_items, blk)];
    const uintptr_t first = (uintptr_t)it.p, end = first + (uintptr_t)it.bytes;
    const uintptr_t a0 = first & ~(uintptr_t)15;
    const int64_t n_chunks = (int64_t)((end - a0 + 15) >> 4);
    const int64_t c0 = (blk - it.block0) * SB_BLOCK_CHUNKS + tid;
    unsigned c = 0;
#pragma unroll
    for (int u = 0; u < SB_BLOCK_CHUNKS / SB_THREADS; ++u) {
      const int64_t ch = c0 + u * SB_THREADS;
      if (ch < n_chunks) {
        const uintptr_t a = a0 + ((uintptr_t)ch << 4);
        uint4 w;
        if (a >= first && a + 16 <= end) {
          w = *reinterpret_cast<const uint4*>(a);
        } else {   // the item's first or last chunk: only its own bytes are read
          unsigned x[4] = {0u, 0u, 0u, 0u};
          for (int b = 0; b < 16; ++b)
            if (a + b >= first && a + b < end) x[b >> 2] |= (unsigned)*reinterpret_cast<const uint8_t*>(a + b) << (8 * (b & 3));
          w = make_uint4(x[0], x[1], x[2], x[3]);
        }
        c += cnt_chunk(w, it.kind);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    __syncthreads();   // (the previous block's s_c has been read)
    if ((tid & 63) == 0) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
      const unsigned t = s_c[0] + s_c[1] + s_c[2] + s_c[3];
      if (t) atomicAdd(&counts[it.out], (unsigned long long)t);
    }
  }
}

static const int cnt_elem_bytes[6] = {1, 2, 4, 8, 4, 8};
static vx_staging g_cnt_stage, g_seg_stage;

extern "C" int64_t vx_count_nonzero_batched_workspace_bytes(int n_items) {
  if (n_items < 0 || n_items > VX_SELECT_MAX_ITEMS) return 0;
  return (int64_t)vx_align256((size_t)(n_items > 0 ? n_items : 1) * sizeof(cnt_item));
}

extern "C" int vx_count_nonzero_batched(const vx_count_item* items, int n_items, uint64_t* counts, void* workspace, int64_t ws_bytes,
                                        vx_stream_t stream) {
  if (n_items < 0 || n_items > VX_SELECT_MAX_ITEMS)
    VX_FAIL(VX_E_SHAPE, "vx_count_nonzero_batched: n_items %d outside 0..%d", n_items, VX_SELECT_MAX_ITEMS);
  if (n_items == 0) return VX_OK;
  if (!items) VX_FAIL(VX_E_NULL, "vx_count_nonzero_batched: null items");
  std::vector<cnt_item> table;
  int64_t n_blocks = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_count_item& it = items[i];
    if (it.kind < VX_COUNT_B1 || it.kind > VX_COUNT_F64) VX_FAIL(VX_E_DTYPE, "vx_count_nonzero_batched: item %d: kind %d", i, it.kind);
    if (it.n < 0 || it.n > (int64_t)1 << 59) VX_FAIL(VX_E_SHAPE, "vx_count_nonzero_batched: item %d: n=%lld", i, (long long)it.n);
    if (it.n == 0) continue;
    if (!it.ptr) VX_FAIL(VX_E_NULL, "vx_count_nonzero_batched: item %d: null pointer", i);
    const int es = cnt_elem_bytes[it.kind];
    if ((uintptr_t)it.ptr % es) VX_FAIL(VX_E_ALIGN, "vx_count_nonzero_batched: item %d: pointer not aligned to its %d-byte elements", i, es);
    const int64_t bytes = it.n * es;
    const int64_t chunks = (int64_t)(((uintptr_t)it.ptr & 15) + bytes + 15) >> 4;
    table.push_back(cnt_item{(const uint8_t*)it.ptr, bytes, n_blocks, it.kind, i});
    n_blocks += (chunks + SB_BLOCK_CHUNKS - 1) / SB_BLOCK_CHUNKS;
  }
  if (!counts || !workspace) VX_FAIL(VX_E_NULL, "vx_count_nonzero_batched: null counts or workspace");
  if (ws_bytes < vx_count_nonzero_batched_workspace_bytes(n_items))
    VX_FAIL(VX_E_WORKSPACE, "vx_count_nonzero_batched: workspace needs %lld bytes", (long long)vx_count_nonzero_batched_workspace_bytes(n_items));
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "vx_count_nonzero_batched: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_items * sizeof(uint64_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "vx_count_nonzero_batched: memset: %s", hipGetErrorString(e));
  if (table.empty()) return VX_OK;
  const vx_stage_part part = {table.data(), table.size() * sizeof(cnt_item), 0};
  const int up = vx_staged_upload(g_cnt_stage, "vx_count_nonzero_batched", &part, 1, part.bytes, workspace, s);
  if (up != VX_OK) return up;
  const int grid = (int)(n_blocks < SB_MAX_GRID ? n_blocks : SB_MAX_GRID);
  hipLaunchKernelGGL(count_batched_kernel, dim3(grid), dim3(SB_THREADS), 0, s, (const cnt_item*)workspace, (int)table.size(), n_blocks,
                     reinterpret_cast<unsigned long long*>(counts));
  VX_CHECK_LAUNCH("vx_count_nonzero_batched");
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// selection

struct SegState {
  unsigned long long k;      // rank still to find among the keys that match the prefix
  unsigned prefix;           // key bits fixed so far
  unsigned kkey;             // the k-th key (after the last pass)
  unsigned above;            // minimum key above it
  int need_above;            // the pass that finds `above` has to run
  int nan, pad;
  unsigned long long hist[2048 + 2048 + 1024];   // one set of bins per pass: nothing is cleared between passes
};

__device__ __forceinline__ unsigned seg_float_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float seg_key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// chunk ch of an item: up to four elements as float32 in v, the bit mask of those that exist is returned.  A float64 is
// narrowed with the conversion instruction's round-to-nearest-even, what astype(float32) does.
__device__ __forceinline__ unsigned seg_load(const seg_item& it, int64_t ch, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (it.dtype == VX_F32) {
    const int64_t e0 = ch * 4 - it.lead;
    if (e0 >= it.n) return 0u;
    const float* p = (const float*)it.p;
    if (e0 >= 0 && e0 + 4 <= it.n) {
      const float4 x = *reinterpret_cast<const float4*>(p + e0);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
      return 15u;
    }
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (e0 + t >= 0 && e0 + t < it.n) { v[t] = p[e0 + t]; m |= 1u << t; }
    return m;
  }
  const int64_t e0 = ch * 2 - it.lead;
  if (e0 >= it.n) return 0u;
  const double* p = (const double*)it.p;
  if (e0 >= 0 && e0 + 2 <= it.n) {
    const double2 x = *reinterpret_cast<const double2*>(p + e0);
    v[0] = (float)x.x; v[1] = (float)x.y;
    return 3u;
  }
  unsigned m = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t)
    if (e0 + t >= 0 && e0 + t < it.n) { v[t] = (float)p[e0 + t]; m |= 1u << t; }
  return m;
}

// one more key in LDS bin `bin` for every lane with `valid`.  Uncertainty maps hold long runs of one value (zeros): the
// lanes that share the first lane's bin add their number with ONE atomic.  Called by all 64 lanes of a wave together.
__device__ __forceinline__ void seg_hist_add(unsigned* h, unsigned bin, bool valid) {
  const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)bin);
  const bool same = valid && bin == first;
  const unsigned long long m = __ballot(same);
  if (same) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&h[first], (unsigned)__popcll(m));
  } else if (valid) {
    atomicAdd(&h[bin], 1u);
  }
}

// (a workgroup counts in 32-bit LDS bins: vx_select_segments refuses a call whose share per workgroup could pass 2^32 elements)
template <int PASS>
__global__ __launch_bounds__(SB_THREADS) void seg_hist_kernel(const seg_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                              SegState* __restrict__ st) {
  constexpr int BITS = PASS == 2 ? 10 : 11, SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0, NB = 1 << BITS;
  constexpr int OFF = PASS == 0 ? 0 : PASS == 1 ? 2048 : 4096;
  __shared__ unsigned h[NB];
  __shared__ int s_nan;
  const int tid = threadIdx.x;
  for (int b = tid; b < NB; b += SB_THREADS) h[b] = 0u;
  if (tid == 0) s_nan = 0;
  __syncthreads();
  const unsigned prefix = PASS == 0 ? 0u : st->prefix >> (SHIFT + BITS);
  bool nan = false;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const seg_item it = items[sb_find(items, n_items, blk)];
    const int64_t c0 = (blk - it.block0) * SB_BLOCK_CHUNKS + tid;
    float v[SB_BLOCK_CHUNKS / SB_THREADS][4];
    unsigned m[SB_BLOCK_CHUNKS / SB_THREADS];
#pragma unroll
    for (int u = 0; u < SB_BLOCK_CHUNKS / SB_THREADS; ++u) m[u] = seg_load(it, c0 + u * SB_THREADS, v[u]);
#pragma unroll
    for (int u = 0; u < SB_BLOCK_CHUNKS / SB_THREADS; ++u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned key = seg_float_key(v[u][t]);
        bool valid = (m[u] >> t) & 1u;
        if (PASS == 0) nan |= valid && (__float_as_uint(v[u][t]) & 0x7fffffffu) > 0x7f800000u;
        else valid = valid && (key >> (SHIFT + BITS)) == prefix;
        seg_hist_add(h, (key >> SHIFT) & (unsigned)(NB - 1), valid);
      }
    }
  }
  if (PASS == 0 && nan) s_nan = 1;
  __syncthreads();
  for (int b = tid; b < NB; b += SB_THREADS)
    if (h[b]) atomicAdd(&st->hist[OFF + b], (unsigned long long)h[b]);
  if (PASS == 0 && tid == 0 && s_nan) atomicOr(&st->nan, 1);
}

// one workgroup: the bin that holds rank k.  Thread t sums its NB / 256 consecutive bins, the sums are scanned in LDS, and
// the one thread whose range holds k walks its bins.
template <int PASS>
__global__ __launch_bounds__(SB_THREADS) void seg_pick_kernel(SegState* __restrict__ st, unsigned long long k_call, unsigned long long n_total,
                                                              float* __restrict__ out, int32_t* __restrict__ status) {
  constexpr int BITS = PASS == 2 ? 10 : 11, SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0, NB = 1 << BITS;
  constexpr int OFF = PASS == 0 ? 0 : PASS == 1 ? 2048 : 4096, PER = NB / SB_THREADS;
  __shared__ unsigned long long s_sum[SB_THREADS];
  const int tid = threadIdx.x;
  const unsigned long long k = PASS == 0 ? k_call : st->k;
  const unsigned prefix = PASS == 0 ? 0u : st->prefix;
  unsigned long long c[PER], mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) { c[j] = st->hist[OFF + tid * PER + j]; mine += c[j]; }
  s_sum[tid] = mine;
  __syncthreads();
  for (int off = 1; off < SB_THREADS; off <<= 1) {   // inclusive scan
    const unsigned long long add = tid >= off ? s_sum[tid - off] : 0ull;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  const unsigned long long incl = s_sum[tid];
  unsigned long long acc = incl - mine;
  if (!(acc <= k && k < incl)) return;   // (k < n_total: exactly one thread stays)
  int b = 0;
#pragma unroll
  for (int j = 0; j < PER - 1; ++j)
    if (b == j && k >= acc + c[j]) { acc += c[j]; b = j + 1; }
  unsigned long long cb = c[0];
#pragma unroll
  for (int j = 1; j < PER; ++j)
    if (b == j) cb = c[j];
  const unsigned key = prefix | ((unsigned)(tid * PER + b) << SHIFT);
  st->k = k - acc;
  st->prefix = key;
  if (PASS == 2) {
    const float kth = seg_key_float(key);
    out[0] = kth;
    out[1] = kth;
    *status = st->nan ? VX_SELECT_NAN : VX_SELECT_OK;
    // another key equal to the k-th behind it, or no element behind it at all: the second order statistic is the first
    const bool need = !(k - acc + 1 < cb) && k_call + 1 < n_total;
    st->kkey = key;
    st->above = 0xFFFFFFFFu;
    st->need_above = need ? 1 : 0;
  }
}

__global__ __launch_bounds__(SB_THREADS) void seg_above_kernel(const seg_item* __restrict__ items, int n_items, int64_t n_blocks,
                                                               SegState* __restrict__ st) {
  __shared__ unsigned s_m[SB_THREADS / 64];
  if (!st->need_above) return;   // written by the last pick: the same for every thread of the grid
  const int tid = threadIdx.x;
  const unsigned kkey = st->kkey;
  unsigned best = 0xFFFFFFFFu;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const seg_item it = items[sb_find(items, n_items, blk)];
    const int64_t c0 = (blk - it.block0) * SB_BLOCK_CHUNKS + tid;
    float v[SB_BLOCK_CHUNKS / SB_THREADS][4];
    unsigned m[SB_BLOCK_CHUNKS / SB_THREADS];
#pragma unroll
    for (int u = 0; u < SB_BLOCK_CHUNKS / SB_THREADS; ++u) m[u] = seg_load(it, c0 + u * SB_THREADS, v[u]);
#pragma unroll
    for (int u = 0; u < SB_BLOCK_CHUNKS / SB_THREADS; ++u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned key = seg_float_key(v[u][t]);
        if (((m[u] >> t) & 1u) && key > kkey && key < best) best = key;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)best, off, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) s_m[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SB_THREADS / 64; ++w) best = s_m[w] < best ? s_m[w] : best;
    if (best != 0xFFFFFFFFu) atomicMin(&st->above, best);
  }
}

__global__ void seg_finish_kernel(const SegState* __restrict__ st, float* __restrict__ out) {
  if (threadIdx.x == 0 && st->need_above) out[1] = seg_key_float(st->above);
}

extern "C" int64_t vx_select_segments_workspace_bytes(int n_items) {
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS) return 0;
  return (int64_t)(vx_align256((size_t)n_items * sizeof(seg_item)) + vx_align256(sizeof(SegState)));
}

extern "C" int vx_select_segments(const vx_select_item* items, int n_items, int64_t k, float* out, int32_t* status, void* workspace,
                                  int64_t ws_bytes, vx_stream_t stream) {
  if (!items) VX_FAIL(VX_E_NULL, "vx_select_segments: null items");
  if (n_items < 1 || n_items > VX_SELECT_MAX_ITEMS)
    VX_FAIL(VX_E_SHAPE, "vx_select_segments: n_items %d outside 1..%d", n_items, VX_SELECT_MAX_ITEMS);
  std::vector<seg_item> table;
  int64_t n_blocks = 0, n_total = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_select_item& it = items[i];
    if (it.dtype != VX_F32 && it.dtype != VX_F64) VX_FAIL(VX_E_DTYPE, "vx_select_segments: item %d: dtype %d", i, it.dtype);
    if (it.n < 0 || it.n > (int64_t)1 << 59) VX_FAIL(VX_E_SHAPE, "vx_select_segments: item %d: n=%lld", i, (long long)it.n);
    if (it.n == 0) continue;
    if (!it.ptr) VX_FAIL(VX_E_NULL, "vx_select_segments: item %d: null pointer", i);
    const int es = it.dtype == VX_F64 ? 8 : 4, per = 16 / es;
    if ((uintptr_t)it.ptr % es) VX_FAIL(VX_E_ALIGN, "vx_select_segments: item %d: pointer not aligned to its %d-byte elements", i, es);
    const int lead = (int)(((uintptr_t)it.ptr & 15) / es);
    const int64_t chunks = (lead + it.n + per - 1) / per;
    table.push_back(seg_item{it.ptr, it.n, n_blocks, it.dtype, lead});
    n_blocks += (chunks + SB_BLOCK_CHUNKS - 1) / SB_BLOCK_CHUNKS;
    n_total += it.n;
    // 4096 elements per work block at most, SB_MAX_GRID workgroups: below 2^32 elements per workgroup
    if (n_blocks >= (int64_t)SB_MAX_GRID << 20) VX_FAIL(VX_E_SHAPE, "vx_select_segments: more than 2^31 work blocks (about 2^43 elements)");
  }
  if (n_total == 0) VX_FAIL(VX_E_SHAPE, "vx_select_segments: no elements");
  if (k < 0 || k >= n_total) VX_FAIL(VX_E_SHAPE, "vx_select_segments: k=%lld outside [0, %lld)", (long long)k, (long long)n_total);
  if (!out || !status || !workspace) VX_FAIL(VX_E_NULL, "vx_select_segments: null out, status or workspace");
  if (ws_bytes < vx_select_segments_workspace_bytes(n_items))
    VX_FAIL(VX_E_WORKSPACE, "vx_select_segments: workspace needs %lld bytes", (long long)vx_select_segments_workspace_bytes(n_items));
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "vx_select_segments: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const seg_item* tab = (const seg_item*)workspace;
  SegState* st = (SegState*)((char*)workspace + vx_align256((size_t)n_items * sizeof(seg_item)));
  hipError_t e = hipMemsetAsync(st, 0, sizeof(SegState), s);
  if (e != hipSuccess) VX_FAIL((int)e, "vx_select_segments: memset: %s", hipGetErrorString(e));
  const vx_stage_part part = {table.data(), table.size() * sizeof(seg_item), 0};
  const int up = vx_staged_upload(g_seg_stage, "vx_select_segments", &part, 1, part.bytes, workspace, s);
  if (up != VX_OK) return up;
  const int n = (int)table.size();
  const dim3 grid((unsigned)(n_blocks < SB_MAX_GRID ? n_blocks : SB_MAX_GRID)), wg(SB_THREADS);
  const unsigned long long kk = (unsigned long long)k, nt = (unsigned long long)n_total;
  hipLaunchKernelGGL(seg_hist_kernel<0>, grid, wg, 0, s, tab, n, n_blocks, st);
  hipLaunchKernelGGL(seg_pick_kernel<0>, dim3(1), wg, 0, s, st, kk, nt, out, status);
  hipLaunchKernelGGL(seg_hist_kernel<1>, grid, wg, 0, s, tab, n, n_blocks, st);
  hipLaunchKernelGGL(seg_pick_kernel<1>, dim3(1), wg, 0, s, st, kk, nt, out, status);
  hipLaunchKernelGGL(seg_hist_kernel<2>, grid, wg, 0, s, tab, n, n_blocks, st);
  hipLaunchKernelGGL(seg_pick_kernel<2>, dim3(1), wg, 0, s, st, kk, nt, out, status);
  hipLaunchKernelGGL(seg_above_kernel, grid, wg, 0, s, tab, n, n_blocks, st);
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(64), 0, s, st, out);
  VX_CHECK_LAUNCH("vx_select_segments");
  return VX_OK;
}
