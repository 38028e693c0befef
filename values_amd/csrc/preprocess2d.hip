// K43: preprocessing of the GTA / Cityscapes 2D data sets (datasets/gta_cityscapes/preprocess_gta_cityscapes.py:128-174)
// for a batch of decoded images and label files.
//   vx_crop_resize_batched: centre crop, the 1 / k resize and the label tables in one pass from the decoded file to the
//     arrays the reference np.saves.  The OUTPUT of every item is cut into work blocks of 2048 pixels from its first pixel
//     (prep2d_plan.h); the blocks of all items, sizes and modes mixed, are taken in turn by one grid, the way
//     preprocess.hip deals its blocks.  Lanes run along output x: a lane produces four consecutive output pixels per step.
//       IMAGE        cv2.resize(INTER_LINEAR) on uint8 at fx = fy = 1 / k: the taps k d + k/2 - 1 and k d + k/2 on each
//                    axis with weight 1/2 each; OpenCV's fixed point gives exactly (p00 + p01 + p10 + p11 + 2) >> 2.  Only
//                    two source rows of every k are touched, and of those the two pixels of every k.
//       LABEL_IDS    nearest (k y, k x), id -> train id -> colour through two tables in LDS.
//       LABEL_COLOR  nearest in RGB (through the palette for an indexed file), colour -> train id by the lookup of
//                    vx_rgb_to_trainid (trainid_lookup.h), ids as int64; the pixels left at the default are counted into
//                    status[item] with an integer atomic.
//     Source bytes are fetched with aligned dword loads covering the taps, whatever the alignment of the source and of
//     its rows (vx_png_unfilter leaves both at any byte offset), and shifted into place; within 12 bytes of the source's
//     ends the bytes are read singly, so nothing outside [src, src + H W bpp) is read.  A lane's 12 RGB bytes, 4 ids or
//     32 bytes of int64 ids leave in dword / 16-byte stores where the output address allows, else singly.
// Plain C++ stores only.  The item table goes up through the pinned staging buffer of staging.h.
#include "common.h"
#include "prep2d_plan.h"
#include "staging.h"
#include "trainid_lookup.h"

namespace {

struct P2dTablesDev {
  const uint8_t* id2trainid;
  const uint8_t* trainid2color;
  const uint32_t* color2trainid;
  int32_t n_color, default_id;
};

// the last item whose block0 is not after blk (same for every thread of a workgroup)
__device__ __forceinline__ int p2d_find(const p2d_item_dev* __restrict__ items, int n, int64_t blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the NB <= 8 bytes at p (any alignment; all inside [lo, hi)) as a little-endian word; bytes above NB are unspecified.
// Aligned dwords that cover them where those lie inside [lo, hi), single bytes at the buffer's two ends.
template <int NB>
__device__ __forceinline__ uint64_t p2d_load(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if constexpr (NB == 1) return *p;
  constexpr int NW = NB == 1 ? 2 : (NB + 6) / 4;   // dwords that cover NB bytes from any offset 0..3 in the first: 2 or 3
  const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
  const uint32_t sh = 8u * (uint32_t)((uintptr_t)p & 3);
  if (a >= (uintptr_t)lo && a + 4 * NW <= (uintptr_t)hi) {
    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(a);
    const uint32_t w1 = *reinterpret_cast<const uint32_t*>(a + 4);
    uint64_t v = (((uint64_t)w1 << 32) | w0) >> sh;
    if (NW == 3) {
      const uint32_t w2 = *reinterpret_cast<const uint32_t*>(a + 8);
      if (sh) v |= (uint64_t)w2 << (64 - sh);
    }
    return v;
  }
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < NB; ++k)
    if (p + k < hi) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

__device__ __forceinline__ uint32_t p2d_byte(uint64_t v, int i) { return (uint32_t)(v >> (8 * i)) & 0xFFu; }

// channel c of the two horizontally adjacent pixels at p (one pixel where the second tap was clamped onto the first), summed
template <int BPP>
__device__ __forceinline__ void p2d_pair_sum(const uint8_t* p, bool two, const uint8_t* lo, const uint8_t* hi,
                                             const uint8_t* __restrict__ pal, uint32_t (&s)[3]) {
  uint32_t a[3], b[3];
  if (BPP == 1) {
    uint32_t i0, i1;
    if (two) {
      const uint64_t v = p2d_load<2>(p, lo, hi);
      i0 = p2d_byte(v, 0); i1 = p2d_byte(v, 1);
    } else {
      i0 = i1 = *p;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = pal[3 * i0 + c]; b[c] = pal[3 * i1 + c]; }
  } else if (two) {
    const uint64_t v = p2d_load<2 * BPP>(p, lo, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = p2d_byte(v, c); b[c] = p2d_byte(v, BPP + c); }
  } else {
    const uint64_t v = p2d_load<BPP>(p, lo, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = b[c] = p2d_byte(v, c);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c] += a[c] + b[c];
}

// the RGB of the pixel at p
template <int BPP>
__device__ __forceinline__ void p2d_pixel(const uint8_t* p, const uint8_t* lo, const uint8_t* hi, const uint8_t* __restrict__ pal,
                                          uint32_t (&c)[3]) {
  if (BPP == 1) {
    const uint32_t i = *p;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = pal[3 * i + k];
  } else {
    const uint64_t v = p2d_load<BPP>(p, lo, hi);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = p2d_byte(v, k);
  }
}

__device__ __forceinline__ void p2d_put_rgb(uint32_t (&o)[3], int j, const uint32_t (&c)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o[(3 * j + k) >> 2] |= c[k] << (8 * ((3 * j + k) & 3));
}

// a lane's 4 pixels of RGB (12 bytes, pixel p0 first) to out: three dwords where all four exist and out + 3 p0 is aligned
__device__ __forceinline__ void p2d_store_rgb(uint8_t* __restrict__ out, uint32_t p0, int cnt, const uint32_t (&o)[3]) {
  uint8_t* d = out + 3 * (size_t)p0;
  if (cnt == P2D_PER_LANE && ((uintptr_t)d & 3) == 0) {
    uint32_t* w = reinterpret_cast<uint32_t*>(d);
    w[0] = o[0]; w[1] = o[1]; w[2] = o[2];
  } else {
#pragma unroll
    for (int b = 0; b < 12; ++b)
      if (b < 3 * cnt) d[b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
  }
}

template <int MODE, int BPP>
__device__ __forceinline__ void p2d_block(const p2d_item_dev& it, int lb, int tid, const uint8_t* s_id, const uint8_t* s_col,
                                          const uint32_t* s_key, const uint32_t* s_cid, int n_color, uint32_t default_id,
                                          int32_t* __restrict__ status) {
  const uint32_t npix = (uint32_t)it.oh * (uint32_t)it.ow, ow = (uint32_t)it.ow;
  const uint32_t W = (uint32_t)it.W, k = (uint32_t)it.k;
  const uint8_t* lo = it.src;
  const uint8_t* hi = it.src + (size_t)it.H * W * BPP;
  const uint8_t* org = it.src + ((size_t)it.y0 * W + (uint32_t)it.x0) * BPP;   // the crop's first pixel
  const uint8_t* __restrict__ pal = it.palette;
  uint32_t unknown = 0;
#pragma unroll
  for (int u = 0; u < P2D_STEPS; ++u) {
    const uint32_t p0 = (uint32_t)lb * P2D_BLOCK_PIX + (uint32_t)(u * P2D_THREADS + tid) * P2D_PER_LANE;
    if (p0 >= npix) break;
    const int cnt = npix - p0 < P2D_PER_LANE ? (int)(npix - p0) : P2D_PER_LANE;
    uint32_t y = p0 / ow, x = p0 - y * ow;
    uint32_t o[3] = {0, 0, 0};
    uint32_t px[P2D_PER_LANE] = {0, 0, 0, 0}, id[P2D_PER_LANE];
#pragma unroll
    for (int j = 0; j < P2D_PER_LANE; ++j) {
      id[j] = default_id;
      if (j < cnt) {
        uint32_t c[3] = {0, 0, 0};
        if (MODE == VX_P2D_IMAGE) {
          const uint32_t ya = k * y + k / 2 - 1, xa = k * x + k / 2 - 1;
          const uint32_t yb = min(ya + 1, (uint32_t)it.ch - 1);
          const bool two = xa + 1 < (uint32_t)it.cw;   // the second tap is not clamped onto the first
          p2d_pair_sum<BPP>(org + ((size_t)ya * W + xa) * BPP, two, lo, hi, pal, c);
          p2d_pair_sum<BPP>(org + ((size_t)yb * W + xa) * BPP, two, lo, hi, pal, c);
#pragma unroll
          for (int q = 0; q < 3; ++q) c[q] = (c[q] + 2) >> 2;
        } else {
          const uint32_t ys = min(k * y, (uint32_t)it.ch - 1), xs = min(k * x, (uint32_t)it.cw - 1);
          const uint8_t* p = org + ((size_t)ys * W + xs) * BPP;
          if (MODE == VX_P2D_LABEL_IDS) {
            id[j] = s_id[*p];
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q] = s_col[3 * id[j] + q];
          } else {
            p2d_pixel<BPP>(p, lo, hi, pal, c);
            px[j] = (c[0] << 16) | (c[1] << 8) | c[2];
          }
        }
        p2d_put_rgb(o, j, c);
      }
      if (++x == ow) { x = 0; ++y; }
    }
    p2d_store_rgb(it.out_rgb, p0, cnt, o);
    if (MODE == VX_P2D_LABEL_IDS) {
      uint8_t* d = (uint8_t*)it.out_ids + p0;
      if (cnt == P2D_PER_LANE && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < P2D_PER_LANE; ++j)
          if (j < cnt) d[j] = (uint8_t)id[j];
      }
    }
    if (MODE == VX_P2D_LABEL_COLOR) {
      rt_lookup<P2D_PER_LANE>(s_key, s_cid, n_color, px, id);
      long long* d = (long long*)it.out_ids + p0;
      if (cnt == P2D_PER_LANE && ((uintptr_t)d & 15) == 0) {
        typedef long long ll2 __attribute__((ext_vector_type(2)));
        ll2 v0, v1;
        v0.x = id[0]; v0.y = id[1]; v1.x = id[2]; v1.y = id[3];
        reinterpret_cast<ll2*>(d)[0] = v0;
        reinterpret_cast<ll2*>(d)[1] = v1;
      } else {
#pragma unroll
        for (int j = 0; j < P2D_PER_LANE; ++j)
          if (j < cnt) d[j] = (long long)id[j];
      }
#pragma unroll
      for (int j = 0; j < P2D_PER_LANE; ++j) unknown += (j < cnt && id[j] == default_id) ? 1u : 0u;
    }
  }
  if (MODE == VX_P2D_LABEL_COLOR && unknown) atomicAdd(status + it.index, (int)unknown);   // integer: exact in any order
}

__global__ __launch_bounds__(P2D_THREADS) void crop_resize_kernel(const p2d_item_dev* __restrict__ items, int n_items, int64_t n_blocks,
                                                                  P2dTablesDev t, int32_t* __restrict__ status) {
  __shared__ uint8_t s_id[256];
  __shared__ uint8_t s_col[768];
  __shared__ uint32_t s_key[RT_MAX];
  __shared__ uint32_t s_cid[RT_MAX];
  const int tid = threadIdx.x;
  if (t.id2trainid) s_id[tid] = t.id2trainid[tid];
  if (t.trainid2color)
    for (int i = tid; i < 768; i += P2D_THREADS) s_col[i] = t.trainid2color[i];
  rt_stage<P2D_THREADS>(t.color2trainid, t.n_color, s_key, s_cid);   // ends with the workgroup's barrier
  const uint32_t dflt = (uint32_t)t.default_id;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const p2d_item_dev it = items[p2d_find(items, n_items, blk)];
    const int lb = (int)(blk - it.block0);
#define P2D_RUN(M, B) p2d_block<M, B>(it, lb, tid, s_id, s_col, s_key, s_cid, t.n_color, dflt, status)
    if (it.mode == VX_P2D_IMAGE) {
      if (it.bpp == 3) P2D_RUN(VX_P2D_IMAGE, 3);
      else if (it.bpp == 4) P2D_RUN(VX_P2D_IMAGE, 4);
      else P2D_RUN(VX_P2D_IMAGE, 1);
    } else if (it.mode == VX_P2D_LABEL_IDS) {
      P2D_RUN(VX_P2D_LABEL_IDS, 1);
    } else {
      if (it.bpp == 3) P2D_RUN(VX_P2D_LABEL_COLOR, 3);
      else if (it.bpp == 4) P2D_RUN(VX_P2D_LABEL_COLOR, 4);
      else P2D_RUN(VX_P2D_LABEL_COLOR, 1);
    }
#undef P2D_RUN
  }
}

vx_staging g_p2d_stage;

}  // namespace

extern "C" int vx_p2d_out_size(int size, int factor) { return p2d_out_size(size, factor); }

extern "C" int64_t vx_crop_resize_batched_workspace_bytes(const vx_p2d_item* items, int n_items, const vx_p2d_tables* tables) {
  p2d_plan p;
  if (p2d_plan_items(items, n_items, tables, &p) != VX_OK) return 0;
  return (int64_t)p.bytes;
}

extern "C" int vx_crop_resize_batched(const vx_p2d_item* items, int n_items, const vx_p2d_tables* tables, int32_t* status,
                                      void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  const char* who = "vx_crop_resize_batched";
  p2d_plan p;
  const int rc = p2d_plan_items(items, n_items, tables, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  if (n_items == 0) return VX_OK;
  if (!status || !workspace) VX_FAIL(VX_E_NULL, "%s: null status or workspace", who);
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  if (ws_bytes < (int64_t)p.bytes) VX_FAIL(VX_E_WORKSPACE, "%s: workspace needs %lld bytes", who, (long long)p.bytes);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)n_items * sizeof(int32_t), s);
  if (e != hipSuccess) VX_FAIL((int)e, "%s: status: %s", who, hipGetErrorString(e));
  const vx_stage_part up = {p.items.data(), p.items.size() * sizeof(p2d_item_dev), 0};
  const int urc = vx_staged_upload(g_p2d_stage, who, &up, 1, up.bytes, workspace, s);
  if (urc != VX_OK) return urc;
  P2dTablesDev t = {nullptr, nullptr, nullptr, 0, 0};
  if (tables) t = P2dTablesDev{tables->id2trainid, tables->trainid2color, tables->color2trainid, tables->color2trainid ? tables->n_color : 0,
                               tables->default_id};
  if (t.n_color < 0 || t.n_color > RT_MAX) t.n_color = 0;   // (no LABEL_COLOR item: the plan did not look at it)
  const dim3 grid((unsigned)(p.n_blocks < P2D_MAX_GRID ? p.n_blocks : P2D_MAX_GRID)), wg(P2D_THREADS);
  hipLaunchKernelGGL(crop_resize_kernel, grid, wg, 0, s, (const p2d_item_dev*)workspace, n_items, p.n_blocks, t, status);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
