// Batched PNG encoder for label masks -- the compression half of the 2D device results writer
// (values_amd/results2d.py: save_images_device).  The reference writes every colour arg-max mask with cv2.imwrite
// (test_2D.py:116-141); the host mirror (image_io.write_png) deflates one file after another on one core.  Here one
// vx_png_encode call turns a batch of (H, W) uint8 label masks into complete RGB PNG files, back to back in dst:
//
//   png_scanline_kernel (grid-stride over each item's scanline bytes, one dword per lane step)
//     the raw PNG image data: per row filter byte 0, then lut[label] as R, G, B (label := unlabeled where ignore != 0);
//     exactly the bytes write_png hands to zlib.  HBM-bound.
//   png_adler_kernel    (one workgroup per 32 KiB chunk): Adler-32 of the chunk's raw bytes -- 128-byte lane slices,
//     then a tree join with adler_combine.
//   gz_chunk_kernel     (deflate_chunk.hip, shared with gzip.hip): one byte-aligned raw DEFLATE fragment per
//     chunk, stride hints (3, 3W + 1, 0): the previous pixel and the previous scanline.
//   png_scan_kernel     (one workgroup): exclusive scan (pack_copy.h) of the fragments' sizes over the whole batch.  File i starts at
//     the sum of the streams before it plus 63 bytes of framing per earlier file; out_offsets / out_sizes are written.
//   png_pack_kernel     (one workgroup per chunk): copies its fragment behind the file's zlib header (pack_copy.h).
//   png_frame_kernel    (one workgroup per file): signature, IHDR, the IDAT length, the zlib header 78 01, the
//     big-endian Adler-32 (chunk Adlers joined in order), IEND; then the IDAT CRC-32 over "IDAT" + the zlib stream,
//     which covers the packed bytes: lane slices, crc_join_block.
//
// File layout (63 bytes of framing around the DEFLATE stream of L bytes):
//   [0, 8) signature  [8, 33) IHDR  [33, 41) IDAT length, "IDAT"  [41, 43) 78 01  [43, 43 + L) stream
//   [43 + L, 47 + L) Adler-32  [47 + L, 51 + L) IDAT CRC  [51 + L, 63 + L) IEND
//
// Every store in this file is a plain C++ store of a vector register.
#include <type_traits>
#include <vector>

#include "deflate_chunk.h"
#include "pack_copy.h"

namespace {

constexpr int PNG_FRAME = 63;     // bytes of a file outside its DEFLATE stream
constexpr int PNG_STREAM0 = 43;   // offset of the DEFLATE stream in the file
constexpr int PNG_FRAME_LANES = 1024;
constexpr int PNG_SCAN_LANES = 1024;

struct PngItemDev {
  const uint8_t* labels;
  const uint8_t* ignore;   // null: none
  uint8_t* raw;            // scanline bytes in the workspace (256-byte aligned, padded to a multiple of 16)
  int32_t H, W;
  int32_t n;               // H * (3 W + 1) < 2^31
  int32_t first_chunk, nchunks, pad;
};

// RGB: `labels` holds the item's RGB bytes and a scanline byte is that byte (vx_png_encode_rgb; lut is not looked at)
template <bool RGB>
__global__ __launch_bounds__(256) void png_scanline_kernel(const PngItemDev* __restrict__ items, int n_items,
                                                           const uint8_t* __restrict__ lut, int unlabeled) {
  __shared__ uint8_t s_lut[768];
  if (!RGB) {
    for (int i = threadIdx.x; i < 768; i += 256) s_lut[i] = lut[i];
    __syncthreads();
  }
  for (int item = blockIdx.y; item < n_items; item += gridDim.y) {
    const PngItemDev it = items[item];
    const uint32_t row = 3u * (uint32_t)it.W + 1u;
    const uint32_t n = (uint32_t)it.n;
    const uint32_t nw = (n + 3) / 4;
    uint32_t* out = reinterpret_cast<uint32_t*>(it.raw);
    for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < nw; w += gridDim.x * 256) {
      const uint32_t k = 4 * w;
      uint32_t y = k / row;
      uint32_t c = k - y * row;
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k + j < n && c != 0) {
          const uint32_t p = (c - 1) / 3;
          const uint32_t ch = c - 1 - 3 * p;
          const size_t pix = (size_t)y * (uint32_t)it.W + p;
          if (RGB) {
            v |= (uint32_t)it.labels[3 * pix + ch] << (8 * j);
          } else {
            int l = it.labels[pix];
            if (it.ignore && it.ignore[pix]) l = unlabeled;
            v |= (uint32_t)s_lut[3 * l + ch] << (8 * j);
          }
        }
        if (++c == row) { c = 0; ++y; }
      }
      out[w] = v;   // the pad bytes of the last dword are zero and lie inside the item's raw buffer
    }
  }
}

__global__ __launch_bounds__(GZ_LANES) void png_adler_kernel(const GzItemDev* __restrict__ items,
                                                             const GzChunkDev* __restrict__ chunks,
                                                             uint32_t* __restrict__ adler) {
  __shared__ uint32_t a[GZ_LANES];
  __shared__ uint32_t len[GZ_LANES];
  const int tid = threadIdx.x;
  const GzChunkDev ch = chunks[blockIdx.x];
  const GzItemDev it = items[ch.item];
  const int64_t cstart = (int64_t)ch.index * GZ_CHUNK;
  const int clen = (int)min64(GZ_CHUNK, it.n - cstart);
  const int s0 = tid * GZ_SLICE;
  const int s1 = min(s0 + GZ_SLICE, clen);
  uint32_t x1 = 1, x2 = 0;   // 128 bytes: x1 <= 32641, x2 < 2^23, no reduction needed inside the slice
  if (s1 > s0) {
    // 16-byte loads: the raw buffer is 256-byte aligned and padded to 16 bytes, slices start on 128-byte boundaries
    const uint4* g = reinterpret_cast<const uint4*>(it.src + cstart + s0);
    const int nb = s1 - s0;
    for (int q = 0; q < (nb + 15) / 16; ++q) {
      const uint4 v = g[q];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (q * 16 + j < nb) {
          x1 += (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
          x2 += x1;
        }
      }
    }
  }
  a[tid] = ((x2 % ADLER_BASE) << 16) | (x1 % ADLER_BASE);
  len[tid] = s1 > s0 ? (uint32_t)(s1 - s0) : 0u;
  for (int stride = 1; stride < GZ_LANES; stride <<= 1) {
    __syncthreads();
    if ((tid % (2 * stride)) == 0 && tid + stride < GZ_LANES) {
      a[tid] = adler_combine(a[tid], a[tid + stride], len[tid + stride]);
      len[tid] += len[tid + stride];
    }
  }
  __syncthreads();
  if (tid == 0) adler[blockIdx.x] = a[0];
}

// exclusive scan of the fragment sizes over the whole batch: chunk_off[c] = file offset of chunk c's fragment in dst
__global__ __launch_bounds__(PNG_SCAN_LANES) void png_scan_kernel(const PngItemDev* __restrict__ items, int n_items,
                                                                  const GzChunkDev* __restrict__ chunks,
                                                                  const GzChunkMeta* __restrict__ meta, int64_t nch,
                                                                  int64_t* __restrict__ chunk_off,
                                                                  int64_t* __restrict__ out_offsets,
                                                                  int64_t* __restrict__ out_sizes) {
  vxpc::exclusive_scan<PNG_SCAN_LANES>(
      nch, [&](int64_t c) { return (int64_t)meta[c].bytes; },
      [&](int64_t c, int64_t run) { chunk_off[c] = run + (int64_t)PNG_FRAME * chunks[c].item + PNG_STREAM0; });
  __syncthreads();   // workgroup-scope fence: the chunk offsets written above are visible to every lane below
  for (int i = threadIdx.x; i < n_items; i += PNG_SCAN_LANES) {
    const PngItemDev it = items[i];
    const int last = it.first_chunk + it.nchunks - 1;
    const int64_t start = chunk_off[it.first_chunk] - PNG_STREAM0;
    out_offsets[i] = start;
    out_sizes[i] = chunk_off[last] + (int64_t)meta[last].bytes - start + (PNG_FRAME - PNG_STREAM0);
  }
}

__global__ __launch_bounds__(256) void png_pack_kernel(const GzChunkMeta* __restrict__ meta, const int64_t* __restrict__ chunk_off,
                                                       const uint8_t* __restrict__ slots, uint8_t* __restrict__ dst) {
  vxpc::copy_bytes<256>(dst + chunk_off[blockIdx.x], slots + (size_t)blockIdx.x * GZ_SLOT, meta[blockIdx.x].bytes);
}

__device__ __forceinline__ uint32_t crc_bytes(uint32_t c, const uint8_t* p, int n) {
  for (int i = 0; i < n; ++i) c = kCrc.byte[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return c;
}
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

__global__ __launch_bounds__(PNG_FRAME_LANES) void png_frame_kernel(const PngItemDev* __restrict__ items,
                                                                    const uint32_t* __restrict__ adler,
                                                                    const int64_t* __restrict__ out_offsets,
                                                                    const int64_t* __restrict__ out_sizes,
                                                                    uint8_t* __restrict__ dst) {
  __shared__ uint32_t crc[PNG_FRAME_LANES];
  __shared__ uint32_t len[PNG_FRAME_LANES];
  const int tid = threadIdx.x;
  const PngItemDev it = items[blockIdx.x];
  uint8_t* f = dst + out_offsets[blockIdx.x];
  const int64_t size = out_sizes[blockIdx.x];
  const int64_t idat = size - (PNG_FRAME - 6);   // zlib header + stream + Adler-32
  if (tid == 0) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; ++i) f[i] = sig[i];
    // IHDR: W, H, bit depth 8, colour type 2 (RGB), deflate, filter method 0, no interlace
    uint8_t ih[17] = {'I', 'H', 'D', 'R', 0, 0, 0, 0, 0, 0, 0, 0, 8, 2, 0, 0, 0};
    put_be32(ih + 4, (uint32_t)it.W);
    put_be32(ih + 8, (uint32_t)it.H);
    put_be32(f + 8, 13u);
    for (int i = 0; i < 17; ++i) f[12 + i] = ih[i];
    put_be32(f + 29, crc_bytes(0xFFFFFFFFu, ih, 17) ^ 0xFFFFFFFFu);
    put_be32(f + 33, (uint32_t)idat);
    f[37] = 'I'; f[38] = 'D'; f[39] = 'A'; f[40] = 'T';
    f[41] = 0x78;   // CM 8 (deflate), CINFO 7 (32 KiB window)
    f[42] = 0x01;   // FLEVEL 0, no dictionary, FCHECK: 0x7801 % 31 == 0
    uint32_t ad = adler[it.first_chunk];
    for (int k = 1; k < it.nchunks; ++k) {
      const int64_t l = min64(GZ_CHUNK, (int64_t)it.n - (int64_t)k * GZ_CHUNK);
      ad = adler_combine(ad, adler[it.first_chunk + k], (uint64_t)l);
    }
    put_be32(f + 41 + idat - 4, ad);
    uint8_t* e = f + size - 12;   // IEND: length 0, "IEND", CRC
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) e[i] = iend[i];
  }
  __syncthreads();   // workgroup-scope fence: the zlib header and the Adler-32 above are read back below
  // IDAT CRC over "IDAT" + zlib stream: lane slices, tree join
  const int64_t n = 4 + idat;
  const uint8_t* x = f + 37;
  const int64_t per = (n + PNG_FRAME_LANES - 1) / PNG_FRAME_LANES;
  const int64_t a = min64(n, per * tid), b = min64(n, a + per);
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = a; i < b; ++i) c = kCrc.byte[(c ^ x[i]) & 0xFF] ^ (c >> 8);
  crc[tid] = c ^ 0xFFFFFFFFu;
  len[tid] = (uint32_t)(b - a);
  crc_join_block<PNG_FRAME_LANES>(crc, len);
  if (tid == 0) put_be32(f + 41 + idat, crc[0]);
}

int64_t png_raw_bytes(int H, int W) { return (int64_t)H * (3 * (int64_t)W + 1); }
constexpr int64_t PNG_RAW_MAX = 0x7FFFFFFF;

struct PngLayout {
  size_t items, gz_items, chunks, meta, adler, chunk_off, slots, raw, total, head;
};

template <typename Item>
PngLayout png_layout(const Item* items, int n, int64_t nch) {
  PngLayout L{};
  size_t o = 0;
  L.items = o; o += vx_align256(sizeof(PngItemDev) * n);
  L.gz_items = o; o += vx_align256(sizeof(GzItemDev) * n);
  L.chunks = o; o += vx_align256(sizeof(GzChunkDev) * nch);
  L.head = o;
  L.meta = o; o += vx_align256(sizeof(GzChunkMeta) * nch);
  L.adler = o; o += vx_align256(sizeof(uint32_t) * nch);
  L.chunk_off = o; o += vx_align256(sizeof(int64_t) * nch);
  L.slots = o; o += (size_t)nch * GZ_SLOT;
  L.raw = o;
  for (int i = 0; i < n; ++i) o += vx_align256((size_t)png_raw_bytes(items[i].H, items[i].W));
  L.total = o;
  return L;
}

}  // namespace

extern "C" int64_t vx_png_bound(int H, int W) {
  if (H < 1 || W < 1) return -1;
  const int64_t n = png_raw_bytes(H, W);
  return n + 5 * gz_nchunks(n) + PNG_FRAME;
}

namespace {

template <typename Item>
size_t png_workspace_bytes(const Item* items, int n) {
  if (!items || n < 1) return 0;
  int64_t nch = 0;
  for (int i = 0; i < n; ++i) {
    if (items[i].H < 1 || items[i].W < 1) return 0;
    nch += gz_nchunks(png_raw_bytes(items[i].H, items[i].W));
  }
  return png_layout(items, n, nch).total;
}

inline const uint8_t* png_src(const vx_png_item& g) { return g.labels; }
inline const uint8_t* png_src(const vx_png_rgb_item& g) { return g.rgb; }
inline const uint8_t* png_ignore(const vx_png_item& g) { return g.ignore; }
inline const uint8_t* png_ignore(const vx_png_rgb_item&) { return nullptr; }

// vx_png_encode (Item = vx_png_item: labels through lut) and vx_png_encode_rgb (Item = vx_png_rgb_item: RGB bytes)
template <typename Item>
int png_encode(const char* who, const Item* items, int n, const uint8_t* lut, int unlabeled, uint8_t* dst, int64_t dst_bytes,
               int64_t* out_offsets, int64_t* out_sizes, void* workspace, size_t ws_bytes, vx_stream_t stream) {
  constexpr bool RGB = std::is_same<Item, vx_png_rgb_item>::value;
  if (n < 1) VX_FAIL(VX_E_SHAPE, "%s: n=%d", who, n);
  if (!items || (!RGB && !lut) || !dst || !out_offsets || !out_sizes || !workspace) VX_FAIL(VX_E_NULL, "%s: null pointer", who);
  if (!vx_aligned16(workspace)) VX_FAIL(VX_E_ALIGN, "%s: workspace not 16-byte aligned", who);
  if (unlabeled < 0 || unlabeled > 255) VX_FAIL(VX_E_SHAPE, "%s: unlabeled=%d outside 0..255", who, unlabeled);
  int64_t need = 0, nch = 0;
  for (int i = 0; i < n; ++i) {
    const Item& g = items[i];
    if (g.H < 1 || g.W < 1) VX_FAIL(VX_E_SHAPE, "%s: item %d: H=%d W=%d", who, i, g.H, g.W);
    if (png_raw_bytes(g.H, g.W) > PNG_RAW_MAX)
      VX_FAIL(VX_E_SHAPE, "%s: item %d: %d x %d has 2^31 or more scanline bytes", who, i, g.H, g.W);
    if (!png_src(g)) VX_FAIL(VX_E_NULL, "%s: item %d: null %s", who, i, RGB ? "rgb" : "labels");
    need += vx_png_bound(g.H, g.W);
    nch += gz_nchunks(png_raw_bytes(g.H, g.W));
  }
  if (dst_bytes < need) VX_FAIL(VX_E_SHAPE, "%s: dst_bytes=%lld < %lld (sum of vx_png_bound)", who, (long long)dst_bytes,
                                (long long)need);
  if (nch > 0x7FFFFFFF) VX_FAIL(VX_E_SHAPE, "%s: %lld chunks", who, (long long)nch);
  const PngLayout L = png_layout(items, n, nch);
  if (ws_bytes < L.total) VX_FAIL(VX_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, L.total);

  // descriptor tables, built in one host block laid out like the head of the workspace and uploaded in one copy
  uint8_t* ws = (uint8_t*)workspace;
  std::vector<uint8_t> head(L.head, 0);
  PngItemDev* pi = reinterpret_cast<PngItemDev*>(head.data() + L.items);
  std::vector<vx_gz_item> recs(n);   // each item's scanline buffer as the chunk kernel's input
  size_t raw = L.raw;
  int32_t c = 0, max_words = 1;
  for (int i = 0; i < n; ++i) {
    const Item& g = items[i];
    const int32_t nb = (int32_t)png_raw_bytes(g.H, g.W);
    const int32_t k = (int32_t)gz_nchunks(nb);
    pi[i] = PngItemDev{png_src(g), png_ignore(g), ws + raw, g.H, g.W, nb, c, k, 0};
    const int64_t row = 3 * (int64_t)g.W + 1;
    // stride hints: the previous pixel and, while within the window, the previous scanline
    recs[i] = vx_gz_item{ws + raw, nb, 0, {3, row <= GZ_CHUNK ? (int32_t)row : 0, 0}, 0};
    c += k;
    raw += vx_align256((size_t)nb);
    max_words = max(max_words, (nb + 3) / 4);
  }
  gz_fill_tables(recs.data(), n, reinterpret_cast<GzItemDev*>(head.data() + L.gz_items),
                 reinterpret_cast<GzChunkDev*>(head.data() + L.chunks));
  hipStream_t s = (hipStream_t)stream;
  if (int rc = vx_upload_table(who, "descriptor upload", ws, head.data(), L.head, s)) return rc;
  const PngItemDev* d_items = (const PngItemDev*)(ws + L.items);
  const GzItemDev* d_gz = (const GzItemDev*)(ws + L.gz_items);
  const GzChunkDev* d_chunks = (const GzChunkDev*)(ws + L.chunks);
  GzChunkMeta* d_meta = (GzChunkMeta*)(ws + L.meta);
  uint32_t* d_adler = (uint32_t*)(ws + L.adler);
  int64_t* d_off = (int64_t*)(ws + L.chunk_off);
  uint8_t* d_slots = ws + L.slots;
  const unsigned bx = (unsigned)min(1024, (max_words + 255) / 256);
  const unsigned by = (unsigned)min(n, 65535);
  hipLaunchKernelGGL(png_scanline_kernel<RGB>, dim3(bx, by), dim3(256), 0, s, d_items, n, lut, unlabeled);
  VX_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(png_adler_kernel, dim3((unsigned)nch), dim3(GZ_LANES), 0, s, d_gz, d_chunks, d_adler);
  VX_CHECK_LAUNCH(who);
  if (int rc = gz_launch_chunks(who, d_gz, d_chunks, d_meta, d_slots, nch, s)) return rc;
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(PNG_SCAN_LANES), 0, s, d_items, n, d_chunks, d_meta, nch, d_off,
                     out_offsets, out_sizes);
  VX_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)nch), dim3(256), 0, s, d_meta, d_off, d_slots, dst);
  VX_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(png_frame_kernel, dim3((unsigned)n), dim3(PNG_FRAME_LANES), 0, s, d_items, d_adler, out_offsets,
                     out_sizes, dst);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

}  // namespace

extern "C" size_t vx_png_workspace_bytes(const vx_png_item* items, int n) { return png_workspace_bytes(items, n); }
extern "C" size_t vx_png_encode_rgb_workspace_bytes(const vx_png_rgb_item* items, int n) { return png_workspace_bytes(items, n); }

extern "C" int vx_png_encode(const vx_png_item* items, int n, const uint8_t* lut, int unlabeled, uint8_t* dst,
                             int64_t dst_bytes, int64_t* out_offsets, int64_t* out_sizes, void* workspace,
                             size_t ws_bytes, vx_stream_t stream) {
  return png_encode("vx_png_encode", items, n, lut, unlabeled, dst, dst_bytes, out_offsets, out_sizes, workspace, ws_bytes, stream);
}

extern "C" int vx_png_encode_rgb(const vx_png_rgb_item* items, int n, uint8_t* dst, int64_t dst_bytes, int64_t* out_offsets,
                                 int64_t* out_sizes, void* workspace, size_t ws_bytes, vx_stream_t stream) {
  return png_encode("vx_png_encode_rgb", items, n, nullptr, 0, dst, dst_bytes, out_offsets, out_sizes, workspace, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Colour rendering of an arg-max mask (Tester.save_prediction, test_2D.py:124-134): label -> RGB through a 256-entry
// table, pixels of the ignore map first set to `unlabeled`.  Byte gather, HBM-bound.
__global__ __launch_bounds__(256) void colorize_u8_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ ignore,
                                                          int64_t n, const uint8_t* __restrict__ lut, int unlabeled,
                                                          uint8_t* __restrict__ rgb) {
  __shared__ uint8_t s_lut[768];
  for (int i = threadIdx.x; i < 768; i += 256) s_lut[i] = lut[i];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int l = labels[i];
    if (ignore && ignore[i]) l = unlabeled;
    rgb[3 * i + 0] = s_lut[3 * l + 0];
    rgb[3 * i + 1] = s_lut[3 * l + 1];
    rgb[3 * i + 2] = s_lut[3 * l + 2];
  }
}

extern "C" int vx_colorize_u8(const uint8_t* labels, const uint8_t* ignore, int64_t n, const uint8_t* lut, int unlabeled,
                              uint8_t* rgb, vx_stream_t stream) {
  if (n < 0 || unlabeled < 0 || unlabeled > 255) VX_FAIL(VX_E_SHAPE, "vx_colorize_u8: n=%lld unlabeled=%d", (long long)n, unlabeled);
  if (n == 0) return VX_OK;
  if (!labels || !lut || !rgb) VX_FAIL(VX_E_NULL, "vx_colorize_u8: null pointer");
  int bx = (int)((n + 255) / 256);
  if (bx > 4096) bx = 4096;
  hipLaunchKernelGGL(colorize_u8_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, labels, ignore, n, lut, unlabeled, rgb);
  VX_CHECK_LAUNCH("vx_colorize_u8");
  return VX_OK;
}
