// Batched gzip encoder (RFC 1951 DEFLATE inside RFC 1952 gzip members) and CRC-32 -- the compression half of the
// device results writer (values_amd/results.py: save_case_device).  The reference writes each NIfTI volume of the
// results tree through SimpleITK's gzip (data_carrier_3D.py:208-371); on the host that is one zlib stream per file on
// one core.  Here every item is cut into 32 KiB chunks and every chunk is one workgroup:
//
//   gz_chunk_kernel   (one workgroup of 256 lanes per chunk)
//     1. the chunk and the 32 KiB before it (same item only) are loaded into LDS: matches reach back across chunks;
//     2. LZ77: each lane greedily parses its own 128-byte slice.  Candidates are the previous byte (runs), the item's
//        stride hints (previous voxel, row, slice of a volume) and one hash-table entry.  The table is filled with the window's positions first, then
//        in lock step with the parse (step r inserts every lane's position slice + r), and atomicMax keeps the latest
//        position per bucket, so every run sees the same table: the output does not depend on scheduling.  A candidate
//        from a later position, outside the window or out of reach is rejected by bounds, a wrong one by the compare;
//     3. symbol histograms with LDS atomics, Huffman lengths (in-place minimum-redundancy construction on the sorted
//        frequencies, limited to 15 bits; the code-length code to 7), canonical codes;
//     4. the block is whichever of stored / fixed / dynamic costs the fewest bytes (exact bit counts from the histograms);
//     5. bit packing: exclusive scan of the lanes' bit counts, then every lane ORs its codes into LDS words;
//     6. a non-final chunk ends byte aligned (an empty stored block after a Huffman block, as pigz does), so chunks
//        concatenate without shifting; the chunk's CRC-32 is the slice CRCs joined with the GF(2) shift operator.
//   gz_pack_kernel    (one workgroup per chunk): the chunk's offset in its member is the sum of the sizes of the chunks
//     before it; it copies its bytes behind the 10-byte header (pack_copy.h), the first chunk writes the header and the last the
//     CRC-32 / ISIZE trailer and the member's size.
//
// The chunk kernel is compiled in deflate_chunk.hip and launched through deflate_chunk.h (shared with png.hip), the CRC-32
// helpers live in checksum.h; this file keeps the gzip framing: the pack kernel, vx_crc32 and the launchers.
//
// Every store in this file is a plain C++ store of a vector register.
#include <vector>

#include "deflate_chunk.h"
#include "pack_copy.h"

namespace {

__global__ __launch_bounds__(256) void gz_pack_kernel(const GzItemDev* __restrict__ items, const GzChunkDev* __restrict__ chunks,
                                                      const GzChunkMeta* __restrict__ meta, const uint8_t* __restrict__ slots,
                                                      uint8_t* __restrict__ dst, int64_t* __restrict__ out_sizes) {
  __shared__ uint32_t part[256];
  __shared__ uint32_t crcs[256];
  const int tid = threadIdx.x;
  const GzChunkDev ch = chunks[blockIdx.x];
  const GzItemDev it = items[ch.item];
  const int c0 = it.first_chunk;
  uint32_t s = 0;
  for (int k = tid; k < ch.index; k += 256) s += meta[c0 + k].bytes;
  part[tid] = s;
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (tid < stride) part[tid] += part[tid + stride];
    __syncthreads();
  }
  const uint64_t off = part[0];
  uint8_t* m = dst + it.dst_off;
  const uint32_t nb = meta[blockIdx.x].bytes;
  vxpc::copy_bytes<256>(m + 10 + off, slots + (size_t)blockIdx.x * GZ_SLOT, nb);
  if (ch.index == 0 && tid < 10) {
    // ID1 ID2 CM=deflate FLG=0 MTIME=0 XFL=0 OS=255
    m[tid] = tid == 0 ? 0x1f : tid == 1 ? 0x8b : tid == 2 ? 8 : tid == 9 ? 255 : 0;
  }
  if (ch.index == it.nchunks - 1) {
    // CRC of the item: chunk CRCs joined in order (all full chunks but the last)
    __syncthreads();
    if (tid == 0) {
      const uint32_t full = crc_shift_op(GZ_CHUNK);
      uint32_t crc = meta[c0].crc;
      for (int k = 1; k < it.nchunks; ++k) {
        const int64_t len = min64(GZ_CHUNK, it.n - (int64_t)k * GZ_CHUNK);
        const uint32_t op = len == GZ_CHUNK ? full : crc_shift_op((uint64_t)len);
        crc = crc_multmodp(op, crc) ^ meta[c0 + k].crc;
      }
      crcs[0] = crc;
    }
    __syncthreads();
    const uint64_t end = 10 + off + nb;
    if (tid < 8) {
      const uint32_t crc = crcs[0];
      const uint32_t isz = (uint32_t)(it.n & 0xFFFFFFFFu);
      const uint32_t v = tid < 4 ? crc : isz;
      m[end + tid] = (uint8_t)(v >> (8 * (tid & 3)));
    }
    if (tid == 0) out_sizes[ch.item] = (int64_t)(end + 8);
  }
}

// CRC-32 of one byte range by one workgroup: lane slices, tree join
__global__ __launch_bounds__(1024) void crc32_kernel(const uint8_t* __restrict__ x, int64_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t crc[1024];
  __shared__ uint32_t len[1024];
  const int tid = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t a = min64(n, per * tid), b = min64(n, a + per);
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = a; i < b; ++i) c = kCrc.byte[(c ^ x[i]) & 0xFF] ^ (c >> 8);
  crc[tid] = c ^ 0xFFFFFFFFu;
  len[tid] = (uint32_t)(b - a);
  crc_join_block<1024>(crc, len);
  if (tid == 0) out[0] = crc[0];
}

}  // namespace

extern "C" int64_t vx_gzip_bound(int64_t n) {
  if (n < 0) return -1;
  return n + 5 * gz_nchunks(n) + 18;
}

extern "C" size_t vx_gzip_workspace_bytes(const int64_t* sizes, int n_items) {
  if (n_items <= 0 || !sizes) return 0;
  int64_t nch = 0;
  for (int i = 0; i < n_items; ++i) {
    if (sizes[i] < 0) return 0;
    nch += gz_nchunks(sizes[i]);
  }
  return vx_align256(sizeof(GzItemDev) * n_items) + vx_align256(sizeof(GzChunkDev) * nch) + vx_align256(sizeof(GzChunkMeta) * nch) +
         (size_t)nch * GZ_SLOT;
}

extern "C" int vx_gzip_encode(const vx_gz_item* items, int n_items, uint8_t* dst, int64_t dst_bytes, int64_t* out_sizes,
                              void* workspace, size_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_gzip_encode: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !dst || !out_sizes || !workspace) VX_FAIL(VX_E_NULL, "vx_gzip_encode: null pointer");
  std::vector<int64_t> sizes(n_items);
  for (int i = 0; i < n_items; ++i) {
    const vx_gz_item& g = items[i];
    if (g.n < 0 || g.dst_off < 0) VX_FAIL(VX_E_SHAPE, "vx_gzip_encode: item %d: n=%lld dst_off=%lld", i, (long long)g.n, (long long)g.dst_off);
    if (g.n > 0 && !g.src) VX_FAIL(VX_E_NULL, "vx_gzip_encode: item %d: null source", i);
    if (g.dst_off + vx_gzip_bound(g.n) > dst_bytes)
      VX_FAIL(VX_E_SHAPE, "vx_gzip_encode: item %d: slot [%lld, +%lld) beyond dst_bytes=%lld", i, (long long)g.dst_off,
              (long long)vx_gzip_bound(g.n), (long long)dst_bytes);
    for (int k = 0; k < 3; ++k)
      if (g.stride_hint[k] < 0 || g.stride_hint[k] > GZ_CHUNK)
        VX_FAIL(VX_E_SHAPE, "vx_gzip_encode: item %d: stride_hint[%d]=%d outside 0..32768", i, k, g.stride_hint[k]);
    sizes[i] = g.n;
  }
  const size_t need = vx_gzip_workspace_bytes(sizes.data(), n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_gzip_encode: workspace %zu < %zu bytes", ws_bytes, need);
  // descriptor tables, built in one host block laid out like the head of the workspace and uploaded in one copy
  int64_t nch = 0;
  for (int i = 0; i < n_items; ++i) nch += gz_nchunks(items[i].n);
  const size_t chunks_at = vx_align256(sizeof(GzItemDev) * n_items);
  std::vector<uint8_t> head(chunks_at + sizeof(GzChunkDev) * nch, 0);
  gz_fill_tables(items, n_items, (GzItemDev*)head.data(), (GzChunkDev*)(head.data() + chunks_at));
  uint8_t* ws = (uint8_t*)workspace;
  GzItemDev* d_items = (GzItemDev*)ws;
  GzChunkDev* d_chunks = (GzChunkDev*)(ws + chunks_at);
  ws += chunks_at + vx_align256(sizeof(GzChunkDev) * nch);
  GzChunkMeta* d_meta = (GzChunkMeta*)ws;
  uint8_t* d_slots = ws + vx_align256(sizeof(GzChunkMeta) * nch);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = vx_upload_table("vx_gzip_encode", "descriptor upload", workspace, head.data(), head.size(), s)) return rc;
  if (int rc = gz_launch_chunks("vx_gzip_encode", d_items, d_chunks, d_meta, d_slots, nch, s)) return rc;
  hipLaunchKernelGGL(gz_pack_kernel, dim3((unsigned)nch), dim3(256), 0, s, d_items, d_chunks, d_meta, d_slots, dst, out_sizes);
  VX_CHECK_LAUNCH("vx_gzip_encode: pack");
  return VX_OK;
}

extern "C" int vx_crc32(const void* x, int64_t n, uint32_t* out, vx_stream_t stream) {
  if (n < 0) VX_FAIL(VX_E_SHAPE, "vx_crc32: n=%lld", (long long)n);
  if (!out || (n > 0 && !x)) VX_FAIL(VX_E_NULL, "vx_crc32: null pointer");
  hipLaunchKernelGGL(crc32_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const uint8_t*)x, n, out);
  VX_CHECK_LAUNCH("vx_crc32");
  return VX_OK;
}
