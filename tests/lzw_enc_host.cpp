// Host encoder built from values_amd/csrc/lzw_enc_core.h: the CPU tests compile it with g++ (and the sanitizers), run
// it as a program and compare its strips with tests/lzw_build.lzw_encode; the GPU tests compare the device encoder
// with the same bytes.  Test-only: the package's host writer (image_io.lzw_encode) is Python.
//
//   lzw_enc_host IN OUT
// IN:  records {int64 capacity, int64 n, n bytes}
// OUT: records {int32 status, int32 pad, int64 size, size bytes}
// A strip longer than the capacity: status VX_LZW_NO_ROOM, the first `capacity` bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../values_amd/csrc/lzw_enc_core.h"

using namespace vxlzwe;

namespace {

// the strip's words into a window of cap bytes: what does not fit is dropped and counted
struct HostSink {
  uint8_t* dst;
  int64_t cap;
  int64_t n;   // bytes handed out, also those dropped
  void word(uint32_t v) {
    for (int k = 0; k < 4; ++k, ++n)
      if (n < cap) dst[n] = (uint8_t)(v >> (8 * k));
  }
};

void wipe(std::vector<uint32_t>& tab) {
  for (uint32_t& s : tab) s = LZWE_EMPTY;
}

int lzw_enc_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_size) {
  std::vector<uint32_t> tab(LZWE_SLOTS);   // exact size: the sanitizers see any index beyond it
  // a window of whole words the sink may fill, exact to the byte afterwards: the last word's padding stays out of dst
  std::vector<uint8_t> stage((size_t)(cap + 4));
  HostSink sink{stage.data(), cap + 4, 0};
  wipe(tab);
  LzwEnc e = lzw_enc_init(tab.data(), sink);
  for (int64_t i = 0; i < n; ++i) {
    if (lzw_enc_byte(e, sink, src[i])) wipe(tab);
    if (e.width != lzw_enc_width(e.k)) abort();   // the width kept as state is the schedule's
  }
  const int64_t before = sink.n;
  const int tail = lzw_enc_finish(e, sink);
  const int64_t size = tail ? sink.n - 4 + tail : sink.n;
  if (sink.n - before > 8 || size > lzw_enc_bound(n)) abort();   // the core's contract
  const int64_t fit = size < cap ? size : cap;
  if (fit) memcpy(dst, stage.data(), (size_t)fit);
  *out_size = fit;
  return size > cap ? VX_LZW_NO_ROOM : VX_LZW_OK;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: lzw_enc_host IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) { perror("lzw_enc_host"); return 2; }
  for (;;) {
    int64_t cap, n;
    if (fread(&cap, 8, 1, f) != 1) break;
    if (fread(&n, 8, 1, f) != 1 || cap < 0 || n < 0) return 3;
    // exact-size buffers (one byte for an empty one): the sanitizers see any access past the input or the capacity
    std::vector<uint8_t> src((size_t)(n ? n : 1)), dst((size_t)(cap ? cap : 1));
    if (n && fread(src.data(), 1, (size_t)n, f) != (size_t)n) return 3;
    int64_t size = 0;
    const int st = lzw_enc_host(src.data(), n, dst.data(), cap, &size);
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
