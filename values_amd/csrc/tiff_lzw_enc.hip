// LZW-compressed float32 TIFF maps written on the device (values_amd/results2d.py: save_images_device(tiff="lzw")) --
// Compression 5 with Predictor 1, 2 or 3, the file libtiff writes by default (cv2.imwrite) and both readers of this
// project read (image_io.read_tiff_f32; tiff_lzw.hip).  The host writer (image_io.lzw_encode) walks one byte after
// another in Python and writes the same bytes.
//
//   tiff_predict_kernel   the forward predictor of tag 317 on float32 rows: a grid over quads of 4 neighbouring samples
//                         of a row.  No scan: an output word (predictor 2) or byte (predictor 3) is the difference of two
//                         neighbouring inputs.
//     Predictor 2: word[i] -= word[i - 1] mod 2^32 within a row.
//     Predictor 3 (libtiff's fpDiff): the row's four byte planes, the most significant bytes first, then
//       byte[i] -= byte[i - 1] mod 256 over the row's 4 W bytes: the byte before plane p's first is plane p - 1's last.
//     Bytes: src and dst may have any alignment; words are loaded and stored whole where their address is a multiple
//       of 4 and byte by byte elsewhere.
//
//   tiff_lzw_enc_kernel   persistent grid, one wavefront (= one workgroup of 64 lanes) per strip; the waves pull items
//                         from an atomic counter (stream_items.h), and the host orders the items largest first.
//     Walk: every lane runs the same serial encode (lzw_enc_core.h) on the same state, so the walk has no divergence;
//       what the walk loads (the item, an input word, a table slot) is taken from the first lane, so the compiler
//       knows it too and keeps the state in scalar registers, with scalar branches.
//       The dictionary is the core's open-addressing hash table in LDS (8192 slots of one word, 32 KiB); a ClearCode
//       wipes it lane-parallel.
//     Input: a 2 KiB window of the strip's bytes in LDS, loaded by the wave with clamped loads and walked to its end.
//     Output: the packer's whole words go to a 4 KiB staging buffer in LDS (a window's 2048 bytes give at most 2050 codes
//       of 12 bits); after every window the wave stores it to the item's window of dst, whole words where the address
//       allows, and the strip's last bytes one by one: nothing is written at or beyond out_sizes[i].
//     A window smaller than the strip: the bytes that fit are written, the item ends with VX_LZW_NO_ROOM.
//   LDS per wave: table 32 KiB + window 2 KiB + staging 4 KiB (38 KiB): 4 waves per CU.
//
//   lzw_pack_scan_kernel  (one workgroup) exclusive scan of the strips' sizes in table order;
//   lzw_pack_kernel       (workgroups over strips) copies each strip from its window to its place in the packed blob;
//                         scan and copy are pack_copy.h's, shared with gzip.hip and png.hip.
//
// Every store in this file is a plain C++ store of a vector register.
#include "pack_copy.h"
#include "stream_items.h"

#include "lzw_enc_core.h"

namespace {

using namespace vxlzwe;

constexpr int LE_LANES = 64;
constexpr int LE_WIN = 2048;           // input window bytes
constexpr int LE_STAGE_WORDS = 1024;   // staged output words
constexpr int LE_WAVES_PER_CU = 4;

// a window's bytes: one data code each, one ClearCode (3836 insertions lie between two), the strip's first ClearCode,
// the packer's carry of < 32 bits, and the two words of the finish
static_assert(12 * (LE_WIN + 2) + 31 + 64 <= 32 * LE_STAGE_WORDS, "the staging buffer holds what one window produces");
static_assert(LE_WIN < LZWE_MAX_ENTRIES, "at most one ClearCode per window");

struct LeShared {
  uint32_t tab[LZWE_SLOTS];
  uint32_t win[LE_WIN / 4];
  uint32_t stage[LE_STAGE_WORDS];
};

using LeSrc = vxsi::WinSrc<LE_WIN>;
using vxsi::WinItem;

// the packer's words into the staging buffer (every lane the same word to the same place)
struct LeSink {
  uint32_t* stage;
  int n;
  __device__ __forceinline__ void word(uint32_t v) { stage[n++] = v; }
};

__device__ __forceinline__ void le_wipe(uint32_t* tab) {
  __syncthreads();
  uint4* t4 = reinterpret_cast<uint4*>(tab);
  for (int k = threadIdx.x; k < LZWE_SLOTS / 4; k += LE_LANES) t4[k] = make_uint4(LZWE_EMPTY, LZWE_EMPTY, LZWE_EMPTY, LZWE_EMPTY);
  __syncthreads();
}

// the first nb staged bytes to win[base, ...), base a multiple of 4; -> the bytes written: nb, or fewer when the window
// of cap bytes ends first
__device__ int le_flush(const uint32_t* stage, int nb, uint8_t* win, int64_t base, int64_t cap) {
  __syncthreads();   // the staged words are written
  const int64_t room = cap - base;   // >= 0
  const int fit = (int64_t)nb <= room ? nb : (int)room;
  const bool al = ((uintptr_t)win & 3) == 0;
  uint8_t* d = win + base;
  for (int k = threadIdx.x; 4 * k < fit; k += LE_LANES) {
    const uint32_t v = stage[k];
    if (al && 4 * k + 4 <= fit) {
      *reinterpret_cast<uint32_t*>(d + 4 * k) = v;
    } else {
      for (int j = 0; j < 4 && 4 * k + j < fit; ++j) d[4 * k + j] = (uint8_t)(v >> (8 * j));
    }
  }
  __syncthreads();   // the staging buffer may be written again
  return fit;
}

// a value every lane holds, as the first lane's: a scalar to the compiler
__device__ __forceinline__ int64_t le_uniform(int64_t v) {
  return (int64_t)(((uint64_t)VX_LZWE_UNIFORM((uint32_t)((uint64_t)v >> 32)) << 32) | VX_LZWE_UNIFORM((uint32_t)v));
}

// one item; *written: bytes in its window
__device__ int le_item(LeShared& S, const WinItem& it, uint8_t* win, int64_t* written) {
  const int64_t cap = le_uniform(it.dst_cap), n = le_uniform(it.src_n);
  le_wipe(S.tab);
  LeSink sink{S.stage, 0};
  LzwEnc e = lzw_enc_init(S.tab, sink);
  LeSrc s{S.win, 0, {it.src, n}};
  int64_t base = 0;   // bytes of the strip flushed: a multiple of 4 until the finish
  for (int64_t p = 0; p < n; p += LE_WIN) {
    vxsi::win_load<LE_WIN, LE_LANES>(S.win, s, p);
    const int m = n - p < LE_WIN ? (int)(n - p) : LE_WIN;
    for (int i = 0; i < m; i += 4) {
      uint32_t v = VX_LZWE_UNIFORM(S.win[i >> 2]);
      const int mm = m - i < 4 ? m - i : 4;
      for (int j = 0; j < mm; ++j, v >>= 8)
        if (lzw_enc_byte(e, sink, (int)(v & 255u))) le_wipe(S.tab);
    }
    const int nb = 4 * sink.n;
    const int fit = le_flush(S.stage, nb, win, base, cap);
    base += fit;
    sink.n = 0;
    if (fit < nb) {
      *written = base;
      return VX_LZW_NO_ROOM;
    }
  }
  const int tail = lzw_enc_finish(e, sink);
  const int nb = tail ? 4 * (sink.n - 1) + tail : 4 * sink.n;
  const int fit = le_flush(S.stage, nb, win, base, cap);
  *written = base + fit;
  return fit < nb ? VX_LZW_NO_ROOM : VX_LZW_OK;
}

__global__ __launch_bounds__(LE_LANES) void tiff_lzw_enc_kernel(const WinItem* __restrict__ items, int n_items, int* counter,
                                                                uint8_t* dst, int64_t* __restrict__ out_sizes,
                                                                int32_t* __restrict__ out_status) {
  __shared__ LeShared S;
  vxsi::for_each_item(items, n_items, counter, [&](const WinItem& it) {
    int64_t written = 0;
    const int st = le_item(S, it, dst + it.dst_off, &written);
    if (threadIdx.x == 0) {
      out_sizes[it.index] = written;
      out_status[it.index] = st;
    }
  });
}

// ---------------------------------------------------------------------------------------------
constexpr int FP_BLOCK = 256;
constexpr int FP_PER = 4;   // samples per lane
constexpr int FP_BLOCKS_PER_CU = 8;

struct FpItemDev {
  const uint8_t* src;
  uint8_t* dst;
  int64_t unit0;   // quads of the items before this one
  int32_t rows, W;
  int32_t predictor;
  int32_t index;
};

__device__ __forceinline__ uint32_t fp_load_word(const uint8_t* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// nv (1 to 4) bytes of v, the lowest first, to p
__device__ __forceinline__ void fp_store_bytes(uint8_t* p, uint32_t v, int nv) {
  if (nv == 4 && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    for (int j = 0; j < nv; ++j) p[j] = (uint8_t)(v >> (8 * j));
  }
}

__global__ __launch_bounds__(FP_BLOCK) void tiff_predict_kernel(const FpItemDev* __restrict__ items, int n_items, int64_t n_units,
                                                                int32_t* __restrict__ out_status) {
  for (int64_t u = (int64_t)blockIdx.x * FP_BLOCK + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * FP_BLOCK) {
    // the item of this quad: the last one whose unit0 <= u
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (items[mid].unit0 <= u) lo = mid;
      else hi = mid - 1;
    }
    const FpItemDev it = items[lo];
    const int W = it.W;
    const int quads = (W + FP_PER - 1) / FP_PER;
    const int64_t r = (u - it.unit0) / quads;
    const int x0 = FP_PER * (int)((u - it.unit0) % quads);
    const int nv = W - x0 < FP_PER ? W - x0 : FP_PER;
    const uint8_t* src = it.src + 4 * r * W;
    uint8_t* dst = it.dst + 4 * r * W;
    const bool sal = ((uintptr_t)src & 3) == 0;
    uint32_t w[FP_PER];
#pragma unroll
    for (int j = 0; j < FP_PER; ++j) w[j] = j < nv ? fp_load_word(src + 4 * (int64_t)(x0 + j), sal) : 0u;
    if (it.predictor == 2) {
      uint32_t prev = x0 > 0 ? fp_load_word(src + 4 * (int64_t)(x0 - 1), sal) : 0u;
      const bool dal = ((uintptr_t)dst & 3) == 0;
#pragma unroll
      for (int j = 0; j < FP_PER; ++j) {
        if (j < nv) {
          uint8_t* p = dst + 4 * (int64_t)(x0 + j);
          const uint32_t d = w[j] - prev;
          if (dal) *reinterpret_cast<uint32_t*>(p) = d;
          else fp_store_bytes(p, d, 4);
          prev = w[j];
        }
      }
    } else {
      // the sample before the quad; for the row's first quad the row's last sample, whose plane p - 1 byte precedes
      // plane p's first
      const uint32_t before = fp_load_word(src + 4 * (int64_t)(x0 > 0 ? x0 - 1 : W - 1), sal);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int sh = 8 * (3 - p);
        uint32_t prev = x0 > 0 ? (before >> sh) & 255u : p > 0 ? (before >> (sh + 8)) & 255u : 0u;
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < FP_PER; ++j) {
          const uint32_t b = (w[j] >> sh) & 255u;
          out |= ((b - prev) & 255u) << (8 * j);
          prev = b;
        }
        fp_store_bytes(dst + (int64_t)p * W + x0, out, nv);
      }
    }
    if (u == it.unit0) out_status[it.index] = VX_LZW_OK;
  }
}

// ---------------------------------------------------------------------------------------------
constexpr int PK_BLOCK = 256;
constexpr int PK_BLOCKS_PER_CU = 8;

struct PkItemDev {
  int64_t off;   // the strip's window in src
  int64_t cap;
};

// a size as the encoder reports it, kept inside the strip's window whatever the buffer holds
__device__ __forceinline__ int64_t pk_size(const int64_t* sizes, const PkItemDev* items, int i) {
  const int64_t v = sizes[i];
  return v < 0 ? 0 : v > items[i].cap ? items[i].cap : v;
}

// out_offsets[i]: the sum of the sizes before strip i; out_offsets[n]: the blob's size
__global__ __launch_bounds__(PK_BLOCK) void lzw_pack_scan_kernel(const PkItemDev* __restrict__ items, int n, const int64_t* __restrict__ sizes,
                                                                 int64_t* __restrict__ out_offsets) {
  const int64_t total = vxpc::exclusive_scan<PK_BLOCK>(
      n, [&](int64_t i) { return pk_size(sizes, items, (int)i); }, [&](int64_t i, int64_t run) { out_offsets[i] = run; });
  if (threadIdx.x == PK_BLOCK - 1) out_offsets[n] = total;
}

__global__ __launch_bounds__(PK_BLOCK) void lzw_pack_kernel(const PkItemDev* __restrict__ items, int n, const int64_t* __restrict__ sizes,
                                                            const int64_t* __restrict__ offsets, const uint8_t* __restrict__ src,
                                                            uint8_t* __restrict__ out, int64_t out_n) {
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t sz = pk_size(sizes, items, i), o = offsets[i];
    if (o + sz > out_n) continue;   // a blob larger than out: out_offsets[n] tells the caller
    vxpc::copy_bytes<PK_BLOCK>(out + o, src + items[i].off, sz);
  }
}

}  // namespace

extern "C" int64_t vx_tiff_lzw_bound(int64_t n) { return n < 0 ? -1 : lzw_enc_bound(n); }

extern "C" int64_t vx_tiff_lzw_encode_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(WinItem), n_items); }

extern "C" int vx_tiff_lzw_encode(const vx_tiff_lzw_item* items, int n_items, uint8_t* dst, int64_t dst_n, int64_t* out_sizes,
                                  int32_t* out_status, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw_encode: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !dst || !out_sizes || !out_status || !workspace) VX_FAIL(VX_E_NULL, "vx_tiff_lzw_encode: null pointer");
  if (dst_n < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw_encode: dst_n=%lld", (long long)dst_n);
  const int64_t need = vx_tiff_lzw_encode_workspace_bytes(n_items);
  if (ws_bytes < need)
    VX_FAIL(VX_E_WORKSPACE, "vx_tiff_lzw_encode: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<WinItem> di;
  if (int rc = vxsi::win_items("vx_tiff_lzw_encode", items, n_items, dst_n, di,
                               [](int, const vx_tiff_lzw_item&, int32_t*) -> int { return VX_OK; }))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_tiff_lzw_encode", workspace, di, s, n_items, LE_WAVES_PER_CU, &grid)) return rc;
  hipLaunchKernelGGL(tiff_lzw_enc_kernel, dim3((unsigned)grid), dim3(LE_LANES), 0, s, vxsi::item_table<WinItem>(workspace), n_items,
                     vxsi::item_counter(workspace), dst, out_sizes, out_status);
  VX_CHECK_LAUNCH("vx_tiff_lzw_encode");
  return VX_OK;
}

extern "C" int64_t vx_tiff_predict_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(FpItemDev), n_items); }

extern "C" int vx_tiff_predict(const vx_tiff_unpredict_item* items, int n_items, int32_t* out_status, void* workspace,
                               int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_predict: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !out_status || !workspace) VX_FAIL(VX_E_NULL, "vx_tiff_predict: null pointer");
  const int64_t need = vx_tiff_predict_workspace_bytes(n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_tiff_predict: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<FpItemDev> di(n_items);
  int64_t n_units = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_tiff_unpredict_item& g = items[i];
    if (g.predictor != 2 && g.predictor != 3) VX_FAIL(VX_E_DTYPE, "vx_tiff_predict: item %d: predictor %d (2 or 3)", i, g.predictor);
    if (g.rows < 1 || g.W < 1) VX_FAIL(VX_E_SHAPE, "vx_tiff_predict: item %d: rows=%d W=%d", i, g.rows, g.W);
    if (g.W > 0x7FFFFFFF / 4 - FP_PER) VX_FAIL(VX_E_SHAPE, "vx_tiff_predict: item %d: a row of W=%d samples", i, g.W);
    if (!g.src || !g.dst) VX_FAIL(VX_E_NULL, "vx_tiff_predict: item %d: null pointer", i);
    const int64_t nb = 4 * (int64_t)g.rows * g.W;
    if (g.src < g.dst + nb && g.dst < g.src + nb) VX_FAIL(VX_E_SHAPE, "vx_tiff_predict: item %d: src and dst overlap", i);
    di[i] = FpItemDev{g.src, g.dst, n_units, g.rows, g.W, g.predictor, i};
    n_units += (int64_t)g.rows * ((g.W + FP_PER - 1) / FP_PER);
  }
  hipStream_t s = (hipStream_t)stream;
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_tiff_predict", workspace, di, s, (n_units + FP_BLOCK - 1) / FP_BLOCK, FP_BLOCKS_PER_CU, &grid))
    return rc;
  hipLaunchKernelGGL(tiff_predict_kernel, dim3((unsigned)grid), dim3(FP_BLOCK), 0, s, vxsi::item_table<FpItemDev>(workspace), n_items,
                     n_units, out_status);
  VX_CHECK_LAUNCH("vx_tiff_predict");
  return VX_OK;
}

extern "C" int64_t vx_tiff_lzw_pack_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(PkItemDev), n_items); }

extern "C" int vx_tiff_lzw_pack(const vx_tiff_lzw_item* items, int n_items, const uint8_t* src, int64_t src_n, const int64_t* sizes,
                                uint8_t* out, int64_t out_n, int64_t* out_offsets, void* workspace, int64_t ws_bytes,
                                vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw_pack: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !src || !sizes || !out || !out_offsets || !workspace) VX_FAIL(VX_E_NULL, "vx_tiff_lzw_pack: null pointer");
  if (src_n < 0 || out_n < 0) VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw_pack: src_n=%lld out_n=%lld", (long long)src_n, (long long)out_n);
  const int64_t need = vx_tiff_lzw_pack_workspace_bytes(n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_tiff_lzw_pack: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  if (src < out + out_n && out < src + src_n) VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw_pack: src and out overlap");
  std::vector<PkItemDev> di(n_items);
  for (int i = 0; i < n_items; ++i) {
    const vx_tiff_lzw_item& g = items[i];
    if (g.dst_off < 0 || g.dst_cap < 0 || g.dst_off > src_n || g.dst_cap > src_n - g.dst_off)
      VX_FAIL(VX_E_SHAPE, "vx_tiff_lzw_pack: item %d: window [%lld, +%lld) beyond src_n=%lld", i, (long long)g.dst_off,
              (long long)g.dst_cap, (long long)src_n);
    di[i] = PkItemDev{g.dst_off, g.dst_cap};
  }
  hipStream_t s = (hipStream_t)stream;
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_tiff_lzw_pack", workspace, di, s, n_items, PK_BLOCKS_PER_CU, &grid)) return rc;
  const PkItemDev* d_items = vxsi::item_table<PkItemDev>(workspace);
  hipLaunchKernelGGL(lzw_pack_scan_kernel, dim3(1), dim3(PK_BLOCK), 0, s, d_items, n_items, sizes, out_offsets);
  VX_CHECK_LAUNCH("vx_tiff_lzw_pack: scan");
  hipLaunchKernelGGL(lzw_pack_kernel, dim3((unsigned)grid), dim3(PK_BLOCK), 0, s, d_items, n_items, sizes, out_offsets, src, out, out_n);
  VX_CHECK_LAUNCH("vx_tiff_lzw_pack");
  return VX_OK;
}
