// The container-independent half of the DEFLATE encoder, shared by gzip.hip (gzip members) and png.hip (zlib streams
// inside PNG files): the sizes and descriptor structs of the chunk kernel and the two host functions through which the
// launchers reach it.  The kernel itself (gz_chunk_kernel: 32 KiB of an item in, a byte-aligned raw DEFLATE fragment
// out) is compiled once, in deflate_chunk.hip; the CRC-32 tables and joins are in checksum.h.  gzip.hip's header comment
// describes the chunk kernel step by step.
#pragma once
#include "checksum.h"

constexpr int GZ_CHUNK = 32768;          // bytes of input per chunk (and the DEFLATE window)
constexpr int GZ_LANES = 256;
constexpr int GZ_SLICE = GZ_CHUNK / GZ_LANES;   // 128 bytes parsed by each lane
constexpr int GZ_HBITS = 12;
constexpr int GZ_HSIZE = 1 << GZ_HBITS;
constexpr int GZ_SLOT = GZ_CHUNK + 256;   // workspace bytes per chunk output (stored worst case: 5 + 32768)

struct GzItemDev {
  const uint8_t* src;
  int64_t n;
  int64_t dst_off;
  int32_t hint[3];
  int32_t first_chunk;
  int32_t nchunks;
  int32_t pad;
};
struct GzChunkDev {
  int32_t item;
  int32_t index;   // chunk number within the item
};
struct GzChunkMeta {
  uint32_t bytes;
  uint32_t crc;
};

static inline int64_t gz_nchunks(int64_t n) { return n <= 0 ? 1 : (n + GZ_CHUNK - 1) / GZ_CHUNK; }

// Host tables of a batch from its (src, n, dst_off, stride_hint) records: items[i] with its first chunk and chunk count,
// and one chunks[] entry per chunk, item after item (the sum of gz_nchunks(recs[i].n) entries).
void gz_fill_tables(const vx_gz_item* recs, int n, GzItemDev* items, GzChunkDev* chunks);

// One workgroup per chunk on the stream: chunk c's fragment goes to slots + c * GZ_SLOT, its size and CRC-32 to meta[c]
// (all four device pointers).  Sets the kernel's dynamic-LDS attribute on first use.  `who` is the calling launcher's
// name, for the error text; -> VX_OK or the HIP error.
int gz_launch_chunks(const char* who, const GzItemDev* items, const GzChunkDev* chunks, GzChunkMeta* meta, uint8_t* slots,
                     int64_t nch, hipStream_t s);
