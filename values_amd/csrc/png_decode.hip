// What follows the inflate when a 2D results tree is read on the device (values_amd/images.py: load_png_device;
// values_amd/gta.py: pred_seg_loading_device) -- the inverse of png.hip's scanline and colour kernels.  The host reader
// (image_io.read_png) reconstructs one byte after another.
//
//   png_unfilter_kernel   persistent grid, one wavefront (= one workgroup of 64 lanes) per image; the waves pull items
//                         from an atomic counter, and the host orders the items by size, largest first.
//     Pre-pass: the lanes read the item's H filter bytes (one per row) and reduce them with two ballots: a byte above 4
//       ends the item with VX_PNG_BAD_FILTER, an item whose rows all have filter 0 takes the copy below.
//     Filter 0 everywhere (every file this project writes): row by row, the lanes copy the row's W * bpp bytes -- the
//       bytes before dst's first dword boundary singly, then whole dwords (the source, at an odd pitch, is read as two
//       aligned dwords joined by v_alignbyte), then the tail singly.
//     The walk, for any other item: bands of 64 rows, lane r owns row r of the band and at step t reconstructs pixel
//       x = t - r (all bpp bytes, packed in one register), so the three neighbours it needs are already known:
//         a  its own result of the step before;
//         b  what lane r - 1 produced one step earlier: one DPP move (wave_shr:1) of that lane's last result;
//         c  what lane r - 1 produced two steps earlier: the b this lane fetched in the step before.
//       Nothing of this goes through memory.  Lane 0's row above is the last row of the band before: lane 63 leaves its
//       pixels in LDS (W * bpp bytes) and lane 0 of the next band reads them; lane 63 writes pixel t - 63 at step t, lane 0
//       has read it 63 steps earlier.  The filter type is one value per lane, the predictor is chosen by selects: no lane
//       runs a loop of its own.  ceil(H / 64) * (W + 63) steps instead of H * W.
//     Bytes: a lane's row starts at an odd offset and ends at another.  Input: single bytes up to the first dword
//       boundary, then aligned dwords into a 64-bit shift register the pixels are taken from (a dword may reach into the
//       next row -- never beyond src_n; the last bytes of the stream are read singly).  Output the same way round: pixels
//       are appended to a shift register, its bytes go out singly up to the first dword boundary of dst, as dwords after
//       it, and the last (at most 3) singly.
//   rgb_to_trainid_kernel  n pixels at pitch 3 -> the id of the table entry with the pixel's 0x00RRGGBB key, else the
//                          default: one compare loop over the table in LDS (every lane reads the same entry: a broadcast).
//                          Four pixels per lane, three dword loads and one dword store, where rgb and out are aligned.
//
// Every store in this file is a plain C++ store of a vector register.
#include "stream_items.h"   // the [counter | items] table of the launcher
#include "trainid_lookup.h"

namespace {

constexpr int PU_LANES = 64;
constexpr int PU_MAX_ROW = 65536;      // bytes of pixels in a row: the LDS row of the walk
constexpr int PU_WAVES_PER_CU = 16;
constexpr int PU_LDS_PER_CU = 160 * 1024;

struct PuItemDev {
  const uint8_t* src;
  uint8_t* dst;
  int32_t src_n;
  int32_t H, W, bpp;
  int32_t index;   // the item's place in the caller's table (out_status)
  int32_t pad;
};

// four bytes at p (any alignment) of a buffer [lo, hi): two aligned dwords and a byte-align where both lie inside
__device__ __forceinline__ uint32_t pu_load4(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
  if (a >= (uintptr_t)lo && a + 8 <= (uintptr_t)hi) {
    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(a);
    const uint32_t w1 = *reinterpret_cast<const uint32_t*>(a + 4);
    return __builtin_amdgcn_alignbyte(w1, w0, sh);
  }
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k)
    if (p + k < hi) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

// every row has filter 0: dst row r = the W * bpp bytes after the row's filter byte
__device__ void pu_copy(const PuItemDev& it, int wb) {
  const int lane = threadIdx.x;
  const uint8_t* hi = it.src + it.src_n;
  for (int r = 0; r < it.H; ++r) {
    const uint8_t* s = it.src + (int64_t)r * (wb + 1) + 1;
    uint8_t* d = it.dst + (int64_t)r * wb;
    const int head = min(wb, (int)((4 - ((uintptr_t)d & 3)) & 3));
    const int nd = (wb - head) >> 2;
    const int tail = head + 4 * nd;
    if (lane < head) d[lane] = s[lane];
    for (int k = lane; k < nd; k += PU_LANES)
      *reinterpret_cast<uint32_t*>(d + head + 4 * k) = pu_load4(s + head + 4 * k, it.src, hi);
    if (lane < wb - tail) d[tail + lane] = s[tail + lane];
  }
}

__device__ __forceinline__ uint32_t pu_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

// the anti-diagonal walk over one item whose filter bytes are all <= 4; prow: W * BPP bytes of LDS
template <int BPP>
__device__ void pu_walk(const PuItemDev& it, uint8_t* prow) {
  const int lane = threadIdx.x;
  const int W = it.W, H = it.H, wb = W * BPP;
  const uint8_t* send = it.src + it.src_n;
  constexpr uint32_t PMASK = BPP == 4 ? 0xFFFFFFFFu : (1u << (8 * (BPP & 3))) - 1u;
  for (int y0 = 0; y0 < H; y0 += PU_LANES) {
    const int y = y0 + lane;
    const bool row = y < H;
    const int nrows = min(PU_LANES, H - y0);
    const bool keep = y0 + PU_LANES < H;           // a band follows: lane 63 leaves its row in LDS
    const uint8_t* ip = it.src + (int64_t)(row ? y : 0) * (wb + 1);
    const int ft = row ? (int)*ip : 0;
    ++ip;
    uint8_t* op = it.dst + (int64_t)(row ? y : 0) * wb;
    uint64_t ibuf = 0, obuf = 0;
    int in = 0, on = 0;
    uint32_t last = 0, b = 0;
    const int steps = W + nrows - 1;
    for (int t = 0; t < steps; ++t) {
      const int x = t - lane;
      const bool act = row && x >= 0 && x < W;
      const uint32_t c = b;                        // the row above, one pixel to the left: last step's b
      b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)last, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
      if (lane == 0) {
        b = 0;
        if (y0 > 0 && act) {
#pragma unroll
          for (int k = 0; k < BPP; ++k) b |= (uint32_t)prow[x * BPP + k] << (8 * k);
        }
      }
      if (act) {
        // the pixel's raw bytes
        while (in < BPP) {
          if (((uintptr_t)ip & 3) == 0 && ip + 4 <= send) {
            ibuf |= (uint64_t)*reinterpret_cast<const uint32_t*>(ip) << (8 * in);
            ip += 4;
            in += 4;
          } else {
            ibuf |= (uint64_t)*ip << (8 * in);
            ip += 1;
            in += 1;
          }
        }
        const uint32_t raw = (uint32_t)ibuf & PMASK;
        ibuf >>= 8 * BPP;
        in -= BPP;
        const uint32_t a = x > 0 ? last : 0u;
        const uint32_t cc = x > 0 ? c : 0u;
        uint32_t px = 0;
#pragma unroll
        for (int k = 0; k < BPP; ++k) {
          const int ak = (a >> (8 * k)) & 255, bk = (b >> (8 * k)) & 255, ck = (cc >> (8 * k)) & 255;
          uint32_t pred = 0;
          pred = ft == 1 ? (uint32_t)ak : pred;
          pred = ft == 2 ? (uint32_t)bk : pred;
          pred = ft == 3 ? (uint32_t)((ak + bk) >> 1) : pred;
          pred = ft == 4 ? pu_paeth(ak, bk, ck) : pred;
          px |= ((((raw >> (8 * k)) & 255u) + pred) & 255u) << (8 * k);
        }
        last = px;
        if (keep && lane == PU_LANES - 1) {
#pragma unroll
          for (int k = 0; k < BPP; ++k) prow[x * BPP + k] = (uint8_t)(px >> (8 * k));
        }
        // out: single bytes up to dst's dword boundary, dwords after it
        obuf |= (uint64_t)px << (8 * on);
        on += BPP;
        while (on > 0 && ((uintptr_t)op & 3)) {
          *op++ = (uint8_t)obuf;
          obuf >>= 8;
          --on;
        }
        if (on >= 4) {
          *reinterpret_cast<uint32_t*>(op) = (uint32_t)obuf;
          op += 4;
          obuf >>= 32;
          on -= 4;
        }
        if (x == W - 1) {
          while (on > 0) {
            *op++ = (uint8_t)obuf;
            obuf >>= 8;
            --on;
          }
        }
      }
    }
    __syncthreads();   // the band's last row is in LDS before the next band's lane 0 reads it
  }
}

__global__ __launch_bounds__(PU_LANES) void png_unfilter_kernel(const PuItemDev* __restrict__ items, int n_items, int* counter,
                                                                int32_t* __restrict__ out_status) {
  extern __shared__ uint8_t pu_row[];
  const int lane = threadIdx.x;
  vxsi::for_each_item(items, n_items, counter, [&](const PuItemDev& it) {
    const int wb = it.W * it.bpp;
    int st = VX_PNG_OK;
    if ((int64_t)it.src_n != (int64_t)it.H * (wb + 1)) {
      st = VX_PNG_BAD_SIZE;
    } else {
      // the H filter bytes: any above 4, any other than 0
      bool bad = false, some = false;
      for (int r = lane; r < it.H; r += PU_LANES) {
        const int f = it.src[(int64_t)r * (wb + 1)];
        bad |= f > 4;
        some |= f != 0;
      }
      if (__ballot(bad)) {
        st = VX_PNG_BAD_FILTER;
      } else if (!__ballot(some)) {
        pu_copy(it, wb);
      } else if (it.bpp == 1) {
        pu_walk<1>(it, pu_row);
      } else if (it.bpp == 3) {
        pu_walk<3>(it, pu_row);
      } else {
        pu_walk<4>(it, pu_row);
      }
    }
    if (lane == 0) out_status[it.index] = st;
  });
}

constexpr int RT_BLOCK = 256;

__global__ __launch_bounds__(RT_BLOCK) void rgb_to_trainid_kernel(const uint8_t* __restrict__ rgb, int64_t n,
                                                                  const uint32_t* __restrict__ table, int n_table, int default_id,
                                                                  uint8_t* __restrict__ out, int aligned) {
  __shared__ uint32_t key[RT_MAX];
  __shared__ uint32_t id[RT_MAX];
  rt_stage<RT_BLOCK>(table, n_table, key, id);
  const int64_t groups = (n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * RT_BLOCK + threadIdx.x; g < groups; g += (int64_t)gridDim.x * RT_BLOCK) {
    const int64_t p0 = 4 * g;
    const int cnt = n - p0 < 4 ? (int)(n - p0) : 4;
    uint32_t px[4] = {0, 0, 0, 0};
    if (aligned && cnt == 4) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(rgb + 3 * p0);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
      const uint32_t q1 = (w0 >> 24) | (w1 << 8), q2 = (w1 >> 16) | (w2 << 16), q3 = w2 >> 8;
      px[0] = __builtin_bswap32(w0) >> 8;
      px[1] = __builtin_bswap32(q1) >> 8;
      px[2] = __builtin_bswap32(q2) >> 8;
      px[3] = __builtin_bswap32(q3) >> 8;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) {
          const uint8_t* p = rgb + 3 * (p0 + k);
          px[k] = ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
        }
    }
    uint32_t r[4] = {(uint32_t)default_id, (uint32_t)default_id, (uint32_t)default_id, (uint32_t)default_id};
    rt_lookup<4>(key, id, n_table, px, r);
    if (aligned && cnt == 4) {
      *reinterpret_cast<uint32_t*>(out + p0) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) out[p0 + k] = (uint8_t)r[k];
    }
  }
}

}  // namespace

extern "C" int64_t vx_png_unfilter_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(PuItemDev), n_items); }

extern "C" int vx_png_unfilter(const vx_png_unfilter_item* items, int n_items, int32_t* out_status, void* workspace,
                               int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_png_unfilter: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !out_status || !workspace) VX_FAIL(VX_E_NULL, "vx_png_unfilter: null pointer");
  const int64_t need = vx_png_unfilter_workspace_bytes(n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_png_unfilter: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<PuItemDev> di(n_items);
  int row_max = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_png_unfilter_item& g = items[i];
    if (g.bpp != 1 && g.bpp != 3 && g.bpp != 4) VX_FAIL(VX_E_DTYPE, "vx_png_unfilter: item %d: bpp %d (1, 3 or 4)", i, g.bpp);
    if (g.H < 1 || g.W < 1) VX_FAIL(VX_E_SHAPE, "vx_png_unfilter: item %d: H=%d W=%d", i, g.H, g.W);
    if ((int64_t)g.W * g.bpp > PU_MAX_ROW)
      VX_FAIL(VX_E_SHAPE, "vx_png_unfilter: item %d: a row of %lld bytes (at most %d)", i, (long long)g.W * g.bpp, PU_MAX_ROW);
    if ((int64_t)g.H * ((int64_t)g.W * g.bpp + 1) > 0x7FFFFFFF) VX_FAIL(VX_E_SHAPE, "vx_png_unfilter: item %d: H (W bpp + 1) >= 2^31", i);
    if (g.src_n < 0) VX_FAIL(VX_E_SHAPE, "vx_png_unfilter: item %d: src_n=%lld", i, (long long)g.src_n);
    if (!g.src || !g.dst) VX_FAIL(VX_E_NULL, "vx_png_unfilter: item %d: null pointer", i);
    // a stream of another size is the item's VX_PNG_BAD_SIZE: any such src_n compares unequal in 32 bits too
    const int32_t sn = g.src_n > 0x7FFFFFFF ? -1 : (int32_t)g.src_n;
    di[i] = PuItemDev{g.src, g.dst, sn, g.H, g.W, g.bpp, i, 0};
    row_max = std::max(row_max, g.W * g.bpp);
  }
  // largest images first: a batch with one large file does not end with one wave working
  std::stable_sort(di.begin(), di.end(), [](const PuItemDev& a, const PuItemDev& b) {
    return (int64_t)a.H * a.W * a.bpp > (int64_t)b.H * b.W * b.bpp;
  });
  hipStream_t s = (hipStream_t)stream;
  const int lds = (int)vx_align256((size_t)row_max);   // <= 64 KiB: the default limit of a launch
  const int per_cu = std::max(1, std::min(PU_WAVES_PER_CU, PU_LDS_PER_CU / lds));
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_png_unfilter", workspace, di, s, n_items, per_cu, &grid)) return rc;
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)grid), dim3(PU_LANES), (size_t)lds, s, vxsi::item_table<PuItemDev>(workspace),
                     n_items, vxsi::item_counter(workspace), out_status);
  VX_CHECK_LAUNCH("vx_png_unfilter");
  return VX_OK;
}

extern "C" int vx_rgb_to_trainid(const uint8_t* rgb, int64_t n, const uint32_t* table, int n_table, int default_id,
                                 uint8_t* out, vx_stream_t stream) {
  if (n < 0) VX_FAIL(VX_E_SHAPE, "vx_rgb_to_trainid: n=%lld", (long long)n);
  if (n_table < 0 || n_table > RT_MAX) VX_FAIL(VX_E_SHAPE, "vx_rgb_to_trainid: n_table=%d (0..%d)", n_table, RT_MAX);
  if (default_id < 0 || default_id > 255) VX_FAIL(VX_E_DTYPE, "vx_rgb_to_trainid: default_id=%d", default_id);
  if (n == 0) return VX_OK;
  if (!rgb || !out || (n_table > 0 && !table)) VX_FAIL(VX_E_NULL, "vx_rgb_to_trainid: null pointer");
  const int aligned = (((uintptr_t)rgb | (uintptr_t)out) & 3) == 0;
  const int64_t groups = (n + 3) >> 2;
  const int64_t blocks = std::min<int64_t>((groups + RT_BLOCK - 1) / RT_BLOCK, (int64_t)vx_cu_count() * 8);
  hipLaunchKernelGGL(rgb_to_trainid_kernel, dim3((unsigned)blocks), dim3(RT_BLOCK), 0, (hipStream_t)stream, rgb, n, table, n_table,
                     default_id, out, aligned);
  VX_CHECK_LAUNCH("vx_rgb_to_trainid");
  return VX_OK;
}
