// Host reference decoder built from values_amd/csrc/lzw_core.h: the CPU tests compile it with g++ (and the sanitizers)
// and compare it with the bytes the streams were made from; the GPU tests compare the device decoder with the same
// bytes.  Test-only: the package's host reader (image_io.tiff_decode) is Python.
//
//   lzw_host IN OUT
// IN:  records {int64 capacity, int64 n, n bytes}
// OUT: records {int32 status, int32 pad, int64 size, size bytes}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../values_amd/csrc/lzw_core.h"
#include "../values_amd/csrc/stream_items.h"

using namespace vxlzw;

namespace {

using HostSrc = vxsi::Bytes;   // the clamped loads the device decoder falls back to outside its window

int lzw_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap64, int64_t* out_size) {
  std::vector<uint32_t> pos(LZW_POS);   // exact size: the sanitizers see any index beyond it
  const HostSrc s{src, n};
  MBits b = mbits_init(n);
  Lzw z = lzw_init(pos.data());
  const uint32_t cap = (uint32_t)cap64;
  uint32_t at = 0;
  int st = VX_LZW_OK;
  while (at < cap) {   // every step consumes >= 9 bits of the input
    int lit = -1;
    uint32_t from = 0, len = 0;
    const int r = lzw_step(z, b, s, at, &lit, &from, &len);
    if (r == LZW_CLEARED) continue;
    if (r == LZW_END) break;
    if (r == LZW_TRUNCATED) { st = VX_LZW_TRUNCATED; break; }
    if (r != LZW_STRING) { st = VX_LZW_BAD_CODE; break; }
    if (len > cap - at) len = cap - at;
    if (lit >= 0) {
      dst[at] = (uint8_t)lit;
    } else {
      for (uint32_t k = 0; k < len; ++k) dst[at + k] = dst[from + k];   // the KwKwK byte reads the one just written
    }
    at += len;
  }
  *out_size = at;
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: lzw_host IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) { perror("lzw_host"); return 2; }
  for (;;) {
    int64_t cap, n;
    if (fread(&cap, 8, 1, f) != 1) break;
    if (fread(&n, 8, 1, f) != 1 || cap < 0 || n < 0 || cap > (int64_t)0xFFFFFFFF) return 3;
    // exact-size buffers (one byte for an empty one): the sanitizers see any access past the input or the capacity
    std::vector<uint8_t> src((size_t)(n ? n : 1)), dst((size_t)(cap ? cap : 1));
    if (n && fread(src.data(), 1, (size_t)n, f) != (size_t)n) return 3;
    int64_t size = 0;
    const int st = lzw_host(src.data(), n, dst.data(), cap, &size);
    if (size < 0 || size > cap) return 4;
    const int32_t oh[2] = {st, 0};
    fwrite(oh, sizeof oh, 1, g);
    fwrite(&size, 8, 1, g);
    if (size) fwrite(dst.data(), 1, (size_t)size, g);
  }
  fclose(f);
  fclose(g);
  return 0;
}
