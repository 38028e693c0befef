// LZW-compressed float32 TIFF maps on the device (values_amd/images.py: load_tiff_device) -- Compression 5 with
// Predictor 1, 2 or 3, what libtiff writes (cv2.imwrite, PIL, GDAL).  The host reader (image_io.tiff_decode) walks one
// code after another in Python.
//
//   tiff_lzw_kernel   persistent grid, one wavefront (= one workgroup of 64 lanes) per strip; the waves pull items from
//                     an atomic counter, and the host orders the items by compressed size, largest first.
//     Code walk: every lane runs the same serial decode (lzw_core.h) on the same state, so the walk has no divergence
//       and lane j simply keeps string j of the batch (up to 64 strings).  The table is the 3839 output offsets at
//       which the codes since the last ClearCode began (LDS, 15 KiB): entry 258 + i is out[pos[i], pos[i + 1]].
//     Strings go to a 4 KiB staging buffer in LDS: single bytes lane-parallel, then each longer string copied by the
//       whole wave in code order from the output before it (the KwKwK string overlaps its own first byte: its last byte
//       is its first), a wave barrier between strings orders the LDS reads after the writes they depend on.  A source
//       before the staging buffer is read from dst: the staging buffer is flushed to dst (the item's window) with
//       lane-parallel stores followed by __syncthreads(), whose workgroup release / acquire waits for the stores before
//       any later read of them.  No string is longer than 3839 bytes, so an empty staging buffer holds any one string: a
//       string that does not fit behind the batch ends the batch undecoded and is decoded again after the flush.
//     Input: a 2 KiB window of the compressed bytes in LDS, refilled by the wave (clamped loads) when the reader is
//       less than 1 KiB from its end (a batch consumes at most 64 codes of 12 bits); a read outside the window falls
//       back to clamped global loads (stream_items.h, which also has the item loop and the launcher's window checks,
//       shared with inflate.hip).
//     A strip ends at its window's last byte (whatever follows: many writers omit EndOfInformation, and a string that
//       reaches beyond the window is cut there, as libtiff cuts it), at EndOfInformation (a window not yet full shows in
//       the size), or with a status.
//   LDS per wave: offsets 15 KiB + window 2 KiB + staging 4 KiB (21 KiB): 7 waves per CU.
//
//   tiff_unpredict_kernel   the predictor of tag 317 undone on float32 rows, one workgroup of 256 lanes per row (rows
//                           are independent; the workgroups pull rows from an atomic counter).  A row is walked in
//                           chunks of 1024 samples, 4 per lane: a lane's running values, an exclusive scan of the
//                           lanes' sums (shuffles inside a wave, the four wave sums through LDS) and the
//                           carry of the chunks before.
//     Predictor 2: word[i] += word[i - 1] on uint32: the scan adds words.
//     Predictor 3 (libtiff's fpAcc): byte[i] += byte[i - 1] mod 256 over the row's 4 W bytes, then sample x is put
//       together from the row's four byte planes (plane 0: the most significant bytes).  The running sum over the whole
//       row is each plane's own running sum plus the sums of the planes before it, so a first pass adds up the planes
//       (a workgroup reduction) and the scan then runs over x with the four planes' bytes packed in one word -- plane p
//       in byte 3 - p, the sample's little-endian word -- and an add without carries between the bytes.
//     Bytes: src and dst may have any alignment; words are loaded and stored whole where their address is a multiple
//       of 4 and byte by byte elsewhere.  Predictor 2 may run in place: a lane reads its words before it writes them.
//
// Every store in this file is a plain C++ store of a vector register.
#include "stream_items.h"

#include "lzw_core.h"

namespace {

using namespace vxlzw;

constexpr int LZ_LANES = 64;
constexpr int LZ_STAGE = 4096;   // staged output bytes (>= LZW_MAX_STRING)
constexpr int LZ_WIN = 2048;     // input window bytes
constexpr int LZ_AHEAD = 1024;   // refill when fewer bytes than this lie ahead of the reader in the window
constexpr int LZ_WAVES_PER_CU = 7;

static_assert(LZ_STAGE >= LZW_MAX_STRING, "an empty staging buffer holds any one string");

struct LzShared {
  uint32_t win[LZ_WIN / 4];
  uint32_t pos[LZW_POS + 1];
  uint8_t stage[LZ_STAGE];
};

using LzSrc = vxsi::WinSrc<LZ_WIN>;   // the reader's byte source (stream_items.h)
using vxsi::WinItem;

// one item; *written: bytes in its window
__device__ int lzw_item(LzShared& S, const WinItem& it, uint8_t* dst, int64_t* written) {
  const int lane = threadIdx.x;
  const uint32_t cap = (uint32_t)it.dst_cap;
  LzSrc s{S.win, 0, {it.src, it.src_n}};
  vxsi::win_load<LZ_WIN, LZ_LANES>(S.win, s, 0);
  MBits b = mbits_init(it.src_n);
  Lzw z = lzw_init(S.pos);
  uint32_t sbase = 0;   // output offset of stage[0]
  int fill = 0;         // staged bytes
  int st = VX_LZW_OK;
  bool done = cap == 0;
  while (!done) {
    if (s.stale(b.pos, LZ_AHEAD)) vxsi::win_load<LZ_WIN, LZ_LANES>(S.win, s, b.pos);
    // decode up to 64 strings (every lane the same); lane j keeps string j
    int tlit = -1, tlen = 0, tp = 0;
    uint32_t tfrom = 0;
    int ntok = 0, bo = fill;
    bool full = false;   // the next string needs the staging buffer emptied first
    while (ntok < LZ_LANES && b.pos + 8 <= s.wbase + LZ_WIN) {   // (a run of ClearCodes can use the window up: refill)
      const MBits b0 = b;
      const int k0 = z.k, w0 = z.width;
      int lit = -1;
      uint32_t from = 0, len = 0;
      const uint32_t at = sbase + (uint32_t)bo;
      const int r = lzw_step(z, b, s, at, &lit, &from, &len);
      if (r == LZW_CLEARED) continue;   // consumed 9 to 12 bits
      if (r == LZW_END) { done = true; break; }
      if (r == LZW_TRUNCATED) { st = VX_LZW_TRUNCATED; done = true; break; }
      if (r != LZW_STRING) { st = VX_LZW_BAD_CODE; done = true; break; }
      if (len > cap - at) len = cap - at;   // cut at the window's end (at < cap here)
      if (bo + (int)len > LZ_STAGE) {       // undo the step; it runs again on an empty staging buffer
        b = b0;
        z.k = k0;
        z.width = w0;
        full = true;
        break;
      }
      if (lane == ntok) {
        tlit = lit;
        tlen = (int)len;
        tfrom = from;
        tp = bo;
      }
      bo += (int)len;
      ++ntok;
      if (at + len == cap) { done = true; break; }
    }
    // the batch: single bytes lane-parallel, then the strings in order
    if (tlen == 1 && tlit >= 0) S.stage[tp] = (uint8_t)tlit;
    __syncthreads();
    uint64_t m = __ballot(tlen > 0 && tlit < 0);
    while (m) {
      const int j = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int L = __builtin_amdgcn_readlane(tlen, j);
      const int P = __builtin_amdgcn_readlane(tp, j);
      const uint32_t F = (uint32_t)__builtin_amdgcn_readlane((int)tfrom, j);
      const uint32_t D = sbase + (uint32_t)P - F;   // >= 1; L <= D + 1
      for (int k = lane; k < L; k += LZ_LANES) {
        const uint32_t so = F + ((uint32_t)k < D ? (uint32_t)k : 0u);   // < sbase + P: bytes written before this string
        const uint8_t v = so >= sbase ? S.stage[so - sbase] : dst[so];
        S.stage[P + k] = v;
      }
      __syncthreads();
    }
    fill = bo;
    if (full || done || fill > LZ_STAGE - 1024) {
      // staged bytes to dst; afterwards every lane may read them from dst
      for (int k = lane; k < fill; k += LZ_LANES) dst[sbase + k] = S.stage[k];
      __syncthreads();
      sbase += (uint32_t)fill;
      fill = 0;
    }
  }
  *written = (int64_t)sbase;
  return st;
}

__global__ __launch_bounds__(LZ_LANES) void tiff_lzw_kernel(const WinItem* __restrict__ items, int n_items, int* counter,
                                                            uint8_t* dst, int64_t* __restrict__ out_sizes,
                                                            int32_t* __restrict__ out_status) {
  __shared__ LzShared S;
  vxsi::for_each_item(items, n_items, counter, [&](const WinItem& it) {
    int64_t written = 0;
    const int st = lzw_item(S, it, dst + it.dst_off, &written);
    if (threadIdx.x == 0) {
      out_sizes[it.index] = written;
      out_status[it.index] = st;
    }
  });
}

// ---------------------------------------------------------------------------------------------
constexpr int UP_BLOCK = 256;
constexpr int UP_PER = 4;                        // samples per lane and chunk
constexpr int UP_CHUNK = UP_BLOCK * UP_PER;
constexpr int UP_BLOCKS_PER_CU = 8;

struct UpItemDev {
  const uint8_t* src;
  uint8_t* dst;
  int64_t row0;    // rows of the items before this one
  int32_t rows, W;
  int32_t predictor;
  int32_t index;
};

// predictor 3's element: four bytes added without carries between them
template <int PRED>
__device__ __forceinline__ uint32_t up_add(uint32_t a, uint32_t b) {
  if (PRED == 2) return a + b;
  return (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu) | (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u);
}

// the workgroup's sum of v (every lane gets it) and, in *excl, the sum of the lanes before this one; wsum: 4 words of LDS
template <int PRED>
__device__ __forceinline__ uint32_t up_scan(uint32_t v, uint32_t* wsum, uint32_t* excl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
    if (lane >= d) inc = up_add<PRED>(inc, o);
  }
  uint32_t ex = (uint32_t)__shfl_up((int)inc, 1, 64);
  if (lane == 0) ex = 0;
  __syncthreads();   // the scan before this one no longer reads wsum
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int w = 0; w < UP_BLOCK / 64; ++w) {
    const uint32_t t = wsum[w];
    if (w < wave) ex = up_add<PRED>(t, ex);
    total = up_add<PRED>(total, t);
  }
  *excl = ex;
  return total;
}

__device__ __forceinline__ uint32_t up_load_word(const uint8_t* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void up_store_word(uint8_t* p, uint32_t v, bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
  }
}

// one row of W samples: src / dst are the row's first bytes
template <int PRED>
__device__ void up_row(const uint8_t* src, uint8_t* dst, int W, uint32_t* wsum) {
  const int t = threadIdx.x;
  const bool sal = ((uintptr_t)src & 3) == 0, dal = ((uintptr_t)dst & 3) == 0;
  uint32_t carry = 0;
  if (PRED == 3) {
    // the planes' sums; plane p's running sum starts at the sum of the planes before it
    uint32_t tot = 0;
    for (int x = t; x < W; x += UP_BLOCK) {
      uint32_t e = 0;
#pragma unroll
      for (int p = 0; p < 4; ++p) e |= (uint32_t)src[(int64_t)p * W + x] << (8 * (3 - p));
      tot = up_add<3>(tot, e);
    }
    uint32_t ex = 0;
    tot = up_scan<3>(tot, wsum, &ex);
    const uint32_t s0 = tot >> 24, s1 = (tot >> 16) & 255u, s2 = (tot >> 8) & 255u;
    carry = ((s0 & 255u) << 16) | (((s0 + s1) & 255u) << 8) | ((s0 + s1 + s2) & 255u);
  }
  for (int x0 = 0; x0 < W; x0 += UP_CHUNK) {
    const int x = x0 + UP_PER * t;
    uint32_t v[UP_PER];
#pragma unroll
    for (int j = 0; j < UP_PER; ++j) {
      uint32_t e = 0;
      if (x + j < W) {
        if (PRED == 2) {
          e = up_load_word(src + 4 * (int64_t)(x + j), sal);
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p) e |= (uint32_t)src[(int64_t)p * W + x + j] << (8 * (3 - p));
        }
      }
      v[j] = j ? up_add<PRED>(v[j - 1], e) : e;
    }
    uint32_t ex = 0;
    const uint32_t total = up_scan<PRED>(v[UP_PER - 1], wsum, &ex);
    const uint32_t base = up_add<PRED>(carry, ex);
#pragma unroll
    for (int j = 0; j < UP_PER; ++j)
      if (x + j < W) up_store_word(dst + 4 * (int64_t)(x + j), up_add<PRED>(base, v[j]), dal);
    carry = up_add<PRED>(carry, total);
  }
}

__global__ __launch_bounds__(UP_BLOCK) void tiff_unpredict_kernel(const UpItemDev* __restrict__ items, int n_items, int64_t n_rows,
                                                                  int* counter, int32_t* __restrict__ out_status) {
  __shared__ uint32_t wsum[UP_BLOCK / 64];
  __shared__ int next;
  for (;;) {
    __syncthreads();   // every lane has read the row before
    if (threadIdx.x == 0) next = atomicAdd(counter, 1);
    __syncthreads();
    const int64_t row = next;
    if (row >= n_rows) return;
    // the item of this row: the last one whose row0 <= row
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (items[mid].row0 <= row) lo = mid;
      else hi = mid - 1;
    }
    const UpItemDev it = items[lo];
    const int64_t r = row - it.row0;
    const int64_t off = 4 * r * it.W;
    if (it.predictor == 2) up_row<2>(it.src + off, it.dst + off, it.W, wsum);
    else up_row<3>(it.src + off, it.dst + off, it.W, wsum);
    if (r == 0 && threadIdx.x == 0) out_status[it.index] = VX_LZW_OK;
  }
}

}  // namespace

extern "C" int64_t vx_tiff_lzw_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(WinItem), n_items); }

extern "C" int vx_tiff_lzw(const vx_tiff_lzw_item* items, int n_items, uint8_t* dst, int64_t dst_n, int64_t* out_sizes,
                           int32_t* out_status, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !dst || !out_sizes || !out_status || !workspace) VX_FAIL(VX_E_NULL, "vx_tiff_lzw: null pointer");
  const int64_t need = vx_tiff_lzw_workspace_bytes(n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_tiff_lzw: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<WinItem> di;
  if (int rc = vxsi::win_items("vx_tiff_lzw", items, n_items, dst_n, di, [](int, const vx_tiff_lzw_item&, int32_t*) -> int { return VX_OK; }))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_tiff_lzw", workspace, di, s, n_items, LZ_WAVES_PER_CU, &grid)) return rc;
  hipLaunchKernelGGL(tiff_lzw_kernel, dim3((unsigned)grid), dim3(LZ_LANES), 0, s, vxsi::item_table<WinItem>(workspace), n_items,
                     vxsi::item_counter(workspace), dst, out_sizes, out_status);
  VX_CHECK_LAUNCH("vx_tiff_lzw");
  return VX_OK;
}

extern "C" int64_t vx_tiff_unpredict_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(UpItemDev), n_items); }
extern "C" int vx_tiff_unpredict(const vx_tiff_unpredict_item* items, int n_items, int32_t* out_status, void* workspace,
                                 int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_unpredict: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !out_status || !workspace) VX_FAIL(VX_E_NULL, "vx_tiff_unpredict: null pointer");
  const int64_t need = vx_tiff_unpredict_workspace_bytes(n_items);
  if (ws_bytes < need)
    VX_FAIL(VX_E_WORKSPACE, "vx_tiff_unpredict: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<UpItemDev> di(n_items);
  int64_t n_rows = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_tiff_unpredict_item& g = items[i];
    if (g.predictor != 2 && g.predictor != 3) VX_FAIL(VX_E_DTYPE, "vx_tiff_unpredict: item %d: predictor %d (2 or 3)", i, g.predictor);
    if (g.rows < 1 || g.W < 1) VX_FAIL(VX_E_SHAPE, "vx_tiff_unpredict: item %d: rows=%d W=%d", i, g.rows, g.W);
    if (g.W > 0x7FFFFFFF / 4 - UP_CHUNK) VX_FAIL(VX_E_SHAPE, "vx_tiff_unpredict: item %d: a row of W=%d samples", i, g.W);
    if (!g.src || !g.dst) VX_FAIL(VX_E_NULL, "vx_tiff_unpredict: item %d: null pointer", i);
    const int64_t nb = 4 * (int64_t)g.rows * g.W;
    const bool same = g.src == g.dst;
    if (!(same && g.predictor == 2) && g.src < g.dst + nb && g.dst < g.src + nb)
      VX_FAIL(VX_E_SHAPE, "vx_tiff_unpredict: item %d: src and dst overlap (in place: predictor 2 with src == dst only)", i);
    di[i] = UpItemDev{g.src, g.dst, n_rows, g.rows, g.W, g.predictor, i};
    n_rows += g.rows;
  }
  if (n_rows > 0x7FFFFFFF - 65536) VX_FAIL(VX_E_SHAPE, "vx_tiff_unpredict: %lld rows in one call", (long long)n_rows);
  hipStream_t s = (hipStream_t)stream;
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_tiff_unpredict", workspace, di, s, n_rows, UP_BLOCKS_PER_CU, &grid)) return rc;
  hipLaunchKernelGGL(tiff_unpredict_kernel, dim3((unsigned)grid), dim3(UP_BLOCK), 0, s, vxsi::item_table<UpItemDev>(workspace),
                     n_items, n_rows, vxsi::item_counter(workspace), out_status);
  VX_CHECK_LAUNCH("vx_tiff_unpredict");
  return VX_OK;
}
