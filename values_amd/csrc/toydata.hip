// K42: the generator of the toy 3D data sets (datasets/toy_data_generation/dataset_generation.py:144-254) on the device,
// all of it in float64 (DESIGN 4.49 ff.).
//   vx_toy_embed            the object placed in the zero image, gray value and flips applied
//   vx_gauss_blur_axis_f64  one pass of scipy.ndimage.gaussian_filter's separable filter, in scipy's order of operations:
//                           centre tap first, then the pairs from the farthest to the nearest as (x[-i] + x[+i]) * w[i],
//                           one rounding per operation, `reflect` boundary.  Lanes run along axis 2 in all three passes.
//                           Axes 0 and 1: a workgroup owns a slab of columns and walks the filter axis with the rows it needs
//                           in an LDS ring; a thread produces two consecutive rows of two columns, so a row it loads from
//                           LDS serves both (two 16-byte LDS loads per tap and four outputs).  Axis 2: each wave stages a
//                           row segment plus halo in LDS and a thread produces two neighbouring outputs the same way.
//   vx_count_ge_f64         #{x >= thr}: ballot, popcount and one integer atomic per wave
//   vx_order_stats_f64      MSB-first radix select (eight 8-bit digits) on the order-preserving 64-bit keys, up to sixteen
//                           distinct ranks per sweep: integer arithmetic only
//   vx_toy_segment          x >= thr_r for all raters from one read of the image
//   vx_toy_noise            the background noise from the two hash words of gauss.h
// Plain C++ stores and integer atomics only.  Nothing is uploaded: ranks, thresholds and boxes travel as kernel arguments.
// The file is compiled with -ffp-contract=off (Makefile) and says so again below.
#include "common.h"
#include "gauss.h"
#include "toy_plan.h"

#pragma clang fp contract(off)

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------
// embed

struct toy_box { int32_t lo[3], hi[3], off[3], od[3], d[3]; int32_t flip0, flip1; };

__global__ __launch_bounds__(TOY_THREADS) void toy_embed_kernel(const float* __restrict__ obj, double* __restrict__ image, toy_box b, double gray) {
  const int64_t rows = (int64_t)b.d[0] * b.d[1];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int i0 = (int)(row / b.d[1]), i1 = (int)(row - (int64_t)i0 * b.d[1]);
    // the flips act on the finished image: output voxel (i0, i1) shows the unflipped image's (j0, j1)
    const int j0 = b.flip0 ? b.d[0] - 1 - i0 : i0, j1 = b.flip1 ? b.d[1] - 1 - i1 : i1;
    const bool in01 = j0 >= b.lo[0] && j0 < b.hi[0] && j1 >= b.lo[1] && j1 < b.hi[1];
    const float* __restrict__ orow = obj + ((int64_t)(j0 - b.off[0]) * b.od[1] + (j1 - b.off[1])) * b.od[2] - b.off[2];
    double* __restrict__ out = image + row * b.d[2];
    for (int z = threadIdx.x; z < b.d[2]; z += TOY_THREADS) {
      double v = 0.0;
      if (in01 && z >= b.lo[2] && z < b.hi[2]) v = gray * (double)orow[z];
      out[z] = v;
    }
  }
}

extern "C" int vx_toy_embed(const float* obj, const int32_t* obj_dims, const int32_t* offset, double gray, int flip0, int flip1,
                            double* image, const int32_t* dims, vx_stream_t stream) {
  const char* who = "vx_toy_embed";
  toy_embed_plan p;
  const int rc = toy_plan_embed(obj, obj_dims, offset, image, dims, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  toy_box b;
  for (int a = 0; a < 3; ++a) { b.lo[a] = p.lo[a]; b.hi[a] = p.hi[a]; b.off[a] = offset[a]; b.od[a] = obj_dims[a]; b.d[a] = dims[a]; }
  b.flip0 = flip0 != 0; b.flip1 = flip1 != 0;
  const int64_t rows = (int64_t)dims[0] * dims[1];
  const dim3 grid((unsigned)(rows < 65536 ? rows : 65536)), wg(TOY_THREADS);
  hipLaunchKernelGGL(toy_embed_kernel, grid, wg, 0, (hipStream_t)stream, obj, image, b, gray);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// blur

// The NR outputs at consecutive positions l .. l + NR - 1 of one thread.  At tap i (from radius down to 1) output j needs
// x[l + j - i] and x[l + j + i]: the low operands of tap i - 1 are those of tap i shifted by one output plus ONE new value,
// and so are the high operands, so a tap costs two loads for NR outputs.  V is double (axis 2) or a pair of columns (axes 0
// and 1).  The staged line is a ring of RB >= 2 r + NR slots `stride` elements apart, s0 the slot of position l - r; the
// two cursors step with a compare, no division.  Per output the order is scipy's: the centre product, then the pairs
// (x[-i] + x[+i]) * w[i] from the farthest to the nearest, each operation rounded on its own.
template <typename V, int NR>
__device__ __forceinline__ void toy_taps(const double* __restrict__ w, int r, const V* line, int stride, int RB, int s0, V (&acc)[NR]) {
  auto wrap = [RB](int s) { return s >= RB ? s - RB : s; };
  const double wc = w[r];
  V lo[NR], hi[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    acc[j] = line[wrap(s0 + r + j) * stride] * wc;
    lo[j] = line[wrap(s0 + j) * stride];               // x[l + j - r]
    hi[j] = line[wrap(s0 + 2 * r + j) * stride];       // x[l + j + r]
  }
  int ilo = wrap(s0 + NR), ihi = wrap(s0 + 2 * r);   // x[l + NR - r] and, one slot below x[l + r], x[l + r - 1]: what tap r - 1 adds
  ihi = ihi == 0 ? RB - 1 : ihi - 1;
#pragma unroll 2
  for (int i = r; i >= 1; --i) {
    const double wi = w[r - i];
    const V nlo = line[ilo * stride];
    const V nhi = line[ihi * stride];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const V pair = lo[j] + hi[j];
      const V prod = pair * wi;
      acc[j] = acc[j] + prod;
    }
#pragma unroll
    for (int j = 0; j < NR - 1; ++j) lo[j] = lo[j + 1];
    lo[NR - 1] = nlo;
#pragma unroll
    for (int j = NR - 1; j > 0; --j) hi[j] = hi[j - 1];
    hi[0] = nhi;
    ilo = ilo + 1 == RB ? 0 : ilo + 1;
    ihi = ihi == 0 ? RB - 1 : ihi - 1;
  }
}

// Axes 0 and 1 on the view [outer][L][inner].  ring[slot][TW] holds the extended rows e in [l0 - r, l0 + STEP + r) of the
// workgroup's columns at slot (e + r) mod RB, RB = 2 r + STEP: the rows a step adds replace exactly the rows the step
// before needed last.  Extended row e is source row toy_reflect(e, L).
template <int TW>
__global__ __launch_bounds__(TOY_THREADS) void blur_strided_kernel(const double* __restrict__ src, double* __restrict__ dst, int L, int64_t inner,
                                                                   int64_t slabs, const double* __restrict__ w, int r, int vec) {
  extern __shared__ f64x2 toy_ring[];
  constexpr int NR = TOY_STRIDED_ROWS, TPR = TW / 2, RPS = TOY_THREADS / TPR, STEP = NR * RPS;
  const int RB = 2 * r + STEP;
  const int64_t o = blockIdx.x / slabs;
  const int64_t c0 = (int64_t)(blockIdx.x - o * slabs) * TW;
  const int tid = threadIdx.x, tcp = tid % TPR, trow = tid / TPR;
  const int64_t col = c0 + 2 * tcp;
  const double* __restrict__ s = src + o * L * inner;
  double* __restrict__ d = dst + o * L * inner;
  const bool c_in = col < inner, c1_in = col + 1 < inner;
  for (int l0 = 0; l0 < L; l0 += STEP) {
    const int e_begin = l0 == 0 ? -r : l0 + r;
    const int e_end = l0 + STEP + r < L + r ? l0 + STEP + r : L + r;
    for (int e = e_begin + trow; e < e_end; e += RPS) {
      const double* __restrict__ p = s + (int64_t)toy_reflect(e, L) * inner + col;
      f64x2 v = {0.0, 0.0};
      if (vec) {
        if (c_in) v = *reinterpret_cast<const f64x2*>(p);
      } else {
        if (c_in) v.x = p[0];
        if (c1_in) v.y = p[1];
      }
      toy_ring[((e + r) % RB) * TPR + tcp] = v;
    }
    __syncthreads();
    const int l = l0 + NR * trow;
    if (l < L && c_in) {
      f64x2 acc[NR];
      // rows l - r .. l + NR - 1 + r lie in [l0 - r, l0 + STEP + r); a row past L + r - 1 was not staged and feeds only
      // rows >= L, which are not stored
      toy_taps<f64x2, NR>(w, r, toy_ring + tcp, TPR, RB, l % RB, acc);   // slot of row l - r: (l - r + r) mod RB
      double* __restrict__ q = d + (int64_t)l * inner + col;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        if (l + j >= L) break;
        if (vec) {
          *reinterpret_cast<f64x2*>(q + j * inner) = acc[j];
        } else {
          q[j * inner] = acc[j].x;
          if (c1_in) q[j * inner + 1] = acc[j].y;
        }
      }
    }
    __syncthreads();
  }
}

// Axis 2: wave v of a workgroup stages positions [z0 - r, z0 + SEG + r) of its row and lane t produces z0 + 2 t and the
// next one.
__global__ __launch_bounds__(TOY_THREADS) void blur_row_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t rows, int n, int64_t segs,
                                                               const double* __restrict__ w, int r, int vec) {
  extern __shared__ double toy_tile[];
  const int P = TOY_ROW_SEG + 2 * r;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t rb = blockIdx.x / segs;
  const int64_t row = rb * TOY_ROW_WAVES + wave;
  const int z0 = (int)(blockIdx.x - rb * segs) * TOY_ROW_SEG;
  double* __restrict__ t = toy_tile + wave * P;
  if (row < rows) {
    const double* __restrict__ s = src + row * n;
    for (int j = lane; j < P; j += 64) {
      const int z = z0 - r + j;
      t[j] = z < n + r ? s[toy_reflect(z, n)] : 0.0;
    }
  }
  __syncthreads();
  const int z = z0 + 2 * lane;
  if (row >= rows || z >= n) return;
  double acc[2];
  toy_taps<double, 2>(w, r, t, 1, P, 2 * lane, acc);   // positions 2 t .. 2 t + 1 + 2 r < P: only the spent cursors wrap
  const double a = acc[0], b = acc[1];
  double* __restrict__ q = dst + row * n + z;
  if (vec) {
    f64x2 v = {a, b};
    *reinterpret_cast<f64x2*>(q) = v;
  } else {
    q[0] = a;
    if (z + 1 < n) q[1] = b;
  }
}

extern "C" int vx_gauss_blur_axis_f64(const double* src, double* dst, const int32_t* dims, int axis, const double* weights, int radius,
                                      vx_stream_t stream) {
  const char* who = "vx_gauss_blur_axis_f64";
  toy_blur_plan p;
  const int rc = toy_plan_blur(src, dst, dims, axis, weights, radius, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks), wg(TOY_THREADS);
  if (axis == 2) {
    hipLaunchKernelGGL(blur_row_kernel, grid, wg, p.lds, s, src, dst, p.outer, (int)p.len, p.slabs, weights, radius, p.vec);
  } else if (p.tw == 64) {
    hipLaunchKernelGGL(blur_strided_kernel<64>, grid, wg, p.lds, s, src, dst, (int)p.len, p.inner, p.slabs, weights, radius, p.vec);
  } else if (p.tw == 32) {
    hipLaunchKernelGGL(blur_strided_kernel<32>, grid, wg, p.lds, s, src, dst, (int)p.len, p.inner, p.slabs, weights, radius, p.vec);
  } else {
    hipLaunchKernelGGL(blur_strided_kernel<16>, grid, wg, p.lds, s, src, dst, (int)p.len, p.inner, p.slabs, weights, radius, p.vec);
  }
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// count

__global__ __launch_bounds__(TOY_THREADS) void toy_count_kernel(const double* __restrict__ x, int64_t n, double thr, unsigned long long* __restrict__ count) {
  unsigned long long c = 0;
  const int64_t stride = (int64_t)gridDim.x * TOY_THREADS;
  // every lane of a wave makes the same number of trips, so the ballot sees the whole wave
  for (int64_t base = (int64_t)blockIdx.x * TOY_THREADS; base < n; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool ge = i < n && x[i] >= thr;
    c += (unsigned long long)__popcll(__ballot(ge));
  }
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

extern "C" int vx_count_ge_f64(const double* x, int64_t n, double thr, int64_t* count, vx_stream_t stream) {
  const char* who = "vx_count_ge_f64";
  if (n < 0 || n > TOY_MAX_N) VX_FAIL(VX_E_SHAPE, "%s: n=%lld outside 0..2^40", who, (long long)n);
  if (!count || (n > 0 && !x)) VX_FAIL(VX_E_NULL, "%s: null x or count", who);
  if (((uintptr_t)x & 7) || ((uintptr_t)count & 7)) VX_FAIL(VX_E_ALIGN, "%s: x or count not aligned to its 8-byte elements", who);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(count, 0, 8, s);
  if (e != hipSuccess) VX_FAIL((int)e, "%s: memset: %s", who, hipGetErrorString(e));
  if (n == 0) return VX_OK;
  const int64_t blocks = (n + TOY_THREADS - 1) / TOY_THREADS;
  const dim3 grid((unsigned)(blocks < TOY_MAX_GRID ? blocks : TOY_MAX_GRID)), wg(TOY_THREADS);
  hipLaunchKernelGGL(toy_count_kernel, grid, wg, 0, s, x, n, thr, (unsigned long long*)count);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// order statistics

// ascending keys = ascending doubles (-0.0 directly below +0.0, NaNs at the two ends)
__device__ __forceinline__ uint64_t toy_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double toy_unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

struct toy_os_ranks { long long k[TOY_OS_CHUNK]; int32_t m, first; };
struct toy_os_pick { int32_t idx[TOY_OS_MAX_K][2]; int32_t n_k; };

struct toy_os_state {
  uint64_t* prefix;              // [16] the key bits found so far (the digits above `shift`)
  long long* krem;               // [16] the rank among the elements that share the prefix
  unsigned long long* hist;      // [16][256]
  double* vals;                  // [64]
};

__global__ __launch_bounds__(TOY_THREADS) void toy_os_init_kernel(toy_os_state st, toy_os_ranks r, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  if (tid < TOY_OS_CHUNK) { st.prefix[tid] = 0; st.krem[tid] = tid < r.m ? r.k[tid] : 0; }
  for (int i = tid; i < TOY_OS_CHUNK * 256; i += TOY_THREADS) st.hist[i] = 0;
  if (r.first && tid == 0) *status = VX_SELECT_OK;
}

__global__ __launch_bounds__(TOY_THREADS) void toy_os_hist_kernel(const double* __restrict__ x, int64_t n, toy_os_state st, int m, int shift, int check_nan,
                                                                  int32_t* __restrict__ status) {
  __shared__ uint32_t h[TOY_OS_CHUNK * 256];
  __shared__ uint64_t pre[TOY_OS_CHUNK];
  const int tid = threadIdx.x;
  for (int i = tid; i < TOY_OS_CHUNK * 256; i += TOY_THREADS) h[i] = 0;
  if (tid < TOY_OS_CHUNK) pre[tid] = shift == 56 ? 0 : st.prefix[tid] >> (shift + 8);
  __syncthreads();
  int nan = 0;
  const int64_t stride = (int64_t)gridDim.x * TOY_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * TOY_THREADS; base < n; base += stride) {   // same trips for every lane of a wave
    const int64_t i = base + tid;
    const bool valid = i < n;
    const double v = valid ? x[i] : 0.0;
    nan |= v != v;
    const uint64_t key = toy_key(v);
    const uint64_t k0 = __shfl(key, 0, 64);   // lane 0 is valid whenever a lane of the wave is
    const unsigned long long vb = __ballot(valid), same = __ballot(valid && key == k0);
    const uint64_t up = shift == 56 ? 0 : key >> (shift + 8);
    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
    if (same == vb) {
      // a wave of equal values (the zero background of a blurred image): one add of the lane count, not 64 adds on one word
      if ((tid & 63) == 0) {
        const uint32_t c = (uint32_t)__popcll(vb);
        for (int j = 0; j < m && c; ++j)
          if (up == pre[j]) atomicAdd(&h[j * 256 + digit], c);
      }
    } else if (valid) {
      for (int j = 0; j < m; ++j)
        if (up == pre[j]) atomicAdd(&h[j * 256 + digit], 1u);
    }
  }
  if (check_nan && nan) atomicOr(status, VX_SELECT_NAN);
  __syncthreads();
  for (int i = tid; i < m * 256; i += TOY_THREADS)
    if (h[i]) atomicAdd(&st.hist[i], (unsigned long long)h[i]);
}

// one workgroup: rank j walks its 256 bins, takes the digit that holds it, and the histograms are cleared for the next pass
__global__ __launch_bounds__(TOY_THREADS) void toy_os_scan_kernel(toy_os_state st, int m, int shift, int vals_base) {
  __shared__ unsigned long long h[TOY_OS_CHUNK * 256];
  const int tid = threadIdx.x;
  for (int i = tid; i < m * 256; i += TOY_THREADS) { h[i] = st.hist[i]; st.hist[i] = 0; }
  __syncthreads();
  if (tid >= m) return;
  long long k = st.krem[tid];
  unsigned long long cum = 0;
  int d = 0;
  for (; d < 255; ++d) {
    const unsigned long long c = h[tid * 256 + d];
    if ((unsigned long long)k < cum + c) break;
    cum += c;
  }
  const uint64_t prefix = st.prefix[tid] | ((uint64_t)d << shift);
  st.prefix[tid] = prefix;
  st.krem[tid] = k - (long long)cum;
  if (shift == 0) st.vals[vals_base + tid] = toy_unkey(prefix);
}

__global__ void toy_os_pick_kernel(const double* __restrict__ vals, toy_os_pick p, double* __restrict__ out) {
  const int i = threadIdx.x;
  if (i < p.n_k) { out[2 * i] = vals[p.idx[i][0]]; out[2 * i + 1] = vals[p.idx[i][1]]; }
}

extern "C" int64_t vx_order_stats_f64_workspace_bytes(int n_k) {
  return n_k >= 1 && n_k <= TOY_OS_MAX_K ? (int64_t)toy_os_bytes() : 0;
}

extern "C" int vx_order_stats_f64_reads(int64_t n, const int64_t* ks, int n_k) {
  toy_os_plan p;
  const double dummy = 0.0;   // the plan only tests the pointers
  if (toy_plan_order_stats(&dummy, n, ks, n_k, &dummy, &dummy, (const void*)(uintptr_t)256, (int64_t)toy_os_bytes(), &p) != VX_OK) return 0;
  return p.reads;
}

extern "C" int vx_order_stats_f64(const double* x, int64_t n, const int64_t* ks, int n_k, double* out, int32_t* status, void* workspace,
                                  int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_order_stats_f64";
  toy_os_plan p;
  const int rc = toy_plan_order_stats(x, n, ks, n_k, out, status, workspace, ws_bytes, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  hipStream_t s = (hipStream_t)stream;
  toy_os_state st;
  st.prefix = (uint64_t*)workspace;
  st.krem = (long long*)((char*)workspace + p.off_krem);
  st.hist = (unsigned long long*)((char*)workspace + p.off_hist);
  st.vals = (double*)((char*)workspace + p.off_vals);
  const int64_t blocks = (n + TOY_THREADS - 1) / TOY_THREADS;
  const dim3 grid((unsigned)(blocks < TOY_MAX_GRID ? blocks : TOY_MAX_GRID)), wg(TOY_THREADS), one(1);
  for (int c = 0; c < p.chunks; ++c) {
    toy_os_ranks r;
    r.m = p.n_u - c * TOY_OS_CHUNK < TOY_OS_CHUNK ? p.n_u - c * TOY_OS_CHUNK : TOY_OS_CHUNK;
    r.first = c == 0;
    for (int j = 0; j < TOY_OS_CHUNK; ++j) r.k[j] = j < r.m ? p.u[c * TOY_OS_CHUNK + j] : 0;
    hipLaunchKernelGGL(toy_os_init_kernel, one, wg, 0, s, st, r, status);
    for (int shift = 56; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(toy_os_hist_kernel, grid, wg, 0, s, x, n, st, r.m, shift, c == 0 && shift == 56, status);
      hipLaunchKernelGGL(toy_os_scan_kernel, one, wg, 0, s, st, r.m, shift, c * TOY_OS_CHUNK);
    }
  }
  toy_os_pick pick;
  pick.n_k = n_k;
  for (int i = 0; i < TOY_OS_MAX_K; ++i) { pick.idx[i][0] = i < n_k ? p.idx[i][0] : 0; pick.idx[i][1] = i < n_k ? p.idx[i][1] : 0; }
  hipLaunchKernelGGL(toy_os_pick_kernel, one, dim3(64), 0, s, (const double*)st.vals, pick, out);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// segmentations

struct toy_thr { double t[TOY_SEG_MAX_R]; };

__global__ __launch_bounds__(TOY_THREADS) void toy_segment_kernel(const double* __restrict__ x, int64_t n, toy_thr thr, int R, int32_t* __restrict__ out, int vec) {
  const int64_t stride = (int64_t)gridDim.x * TOY_THREADS * 4;
  for (int64_t e = ((int64_t)blockIdx.x * TOY_THREADS + threadIdx.x) * 4; e < n; e += stride) {
    if (vec) {   // n % 4 == 0 and both pointers 16-byte aligned: every plane starts aligned
      const f64x2 a = *reinterpret_cast<const f64x2*>(x + e), b = *reinterpret_cast<const f64x2*>(x + e + 2);
      for (int r = 0; r < R; ++r) {
        const double t = thr.t[r];
        const i32x4 v = {a.x >= t, a.y >= t, b.x >= t, b.y >= t};
        *reinterpret_cast<i32x4*>(out + (int64_t)r * n + e) = v;
      }
    } else {
      for (int u = 0; u < 4 && e + u < n; ++u) {
        const double v = x[e + u];
        for (int r = 0; r < R; ++r) out[(int64_t)r * n + e + u] = v >= thr.t[r];
      }
    }
  }
}

extern "C" int vx_toy_segment(const double* x, int64_t n, const double* thresholds, int R, int32_t* out, vx_stream_t stream) {
  const char* who = "vx_toy_segment";
  if (R < 1 || R > TOY_SEG_MAX_R) VX_FAIL(VX_E_SHAPE, "%s: R=%d outside 1..%d", who, R, TOY_SEG_MAX_R);
  if (n < 1 || n > TOY_MAX_N) VX_FAIL(VX_E_SHAPE, "%s: n=%lld outside 1..2^40", who, (long long)n);
  if (!x || !thresholds || !out) VX_FAIL(VX_E_NULL, "%s: null x, thresholds or out", who);
  if (((uintptr_t)x & 7) || ((uintptr_t)out & 3)) VX_FAIL(VX_E_ALIGN, "%s: x or out not aligned to its elements", who);
  toy_thr thr;
  for (int r = 0; r < TOY_SEG_MAX_R; ++r) thr.t[r] = r < R ? thresholds[r] : 0.0;
  const int vec = n % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const int64_t blocks = (n + TOY_THREADS * 4 - 1) / (TOY_THREADS * 4);
  const dim3 grid((unsigned)(blocks < 4 * TOY_MAX_GRID ? blocks : 4 * TOY_MAX_GRID)), wg(TOY_THREADS);
  hipLaunchKernelGGL(toy_segment_kernel, grid, wg, 0, (hipStream_t)stream, x, n, thr, R, out, vec);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// noise

__global__ __launch_bounds__(TOY_THREADS) void toy_noise_kernel(double* __restrict__ x, int64_t n, uint32_t seed, uint32_t stream_index, double noise_prob) {
  const int64_t stride = (int64_t)gridDim.x * TOY_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * TOY_THREADS + threadIdx.x; i < n; i += stride) {
    if (!(x[i] < 0.1)) continue;
    uint32_t h1, h2;
    vx_gauss_words(seed, (uint32_t)i, stream_index, h1, h2);
    const double up = (double)(h1 >> 8) * (1.0 / 16777216.0), un = (double)(h2 >> 8) * (1.0 / 16777216.0);
    x[i] = up <= noise_prob ? 0.0 : un;
  }
}

extern "C" int vx_toy_noise(double* x, int64_t n, uint32_t seed, uint32_t stream_index, double noise_prob, vx_stream_t stream) {
  const char* who = "vx_toy_noise";
  if (n < 0 || n >= ((int64_t)1 << 32)) VX_FAIL(VX_E_SHAPE, "%s: n=%lld outside [0, 2^32): the element index is one hash word", who, (long long)n);
  if (!(noise_prob >= 0.0 && noise_prob <= 1.0)) VX_FAIL(VX_E_SHAPE, "%s: noise_prob %g outside [0, 1]", who, noise_prob);
  if (n == 0) return VX_OK;
  if (!x) VX_FAIL(VX_E_NULL, "%s: null x", who);
  if ((uintptr_t)x & 7) VX_FAIL(VX_E_ALIGN, "%s: x not aligned to its 8-byte elements", who);
  const int64_t blocks = (n + TOY_THREADS - 1) / TOY_THREADS;
  const dim3 grid((unsigned)(blocks < 4 * TOY_MAX_GRID ? blocks : 4 * TOY_MAX_GRID)), wg(TOY_THREADS);
  hipLaunchKernelGGL(toy_noise_kernel, grid, wg, 0, (hipStream_t)stream, x, n, seed, stream_index, noise_prob);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
