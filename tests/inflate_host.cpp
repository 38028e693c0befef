// Host reference decoder built from values_amd/csrc/inflate_core.h: the CPU tests compile it with g++ (and the
// sanitizers) and compare it with zlib; the GPU tests compare the device decoder's statuses with it.  Test-only: the
// package has no CPU decode path.
//
//   inflate_host IN OUT
// IN:  records {int32 format, int32 pad, int64 capacity, int64 n, n bytes}
// OUT: records {int32 status, int32 pad, int64 size, size bytes}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../values_amd/csrc/inflate_core.h"
#include "../values_amd/csrc/stream_items.h"

using namespace vxinf;

namespace {

using HostSrc = vxsi::Bytes;   // the clamped loads the device decoder falls back to outside its window

uint32_t crc32_of(const uint8_t* p, int64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return c ^ 0xFFFFFFFFu;
}

uint32_t adler32_of(const uint8_t* p, int64_t n) {
  uint32_t a = 1, b = 0;
  for (int64_t i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}

// one Huffman block (BTYPE 1 or 2) after its tables are built
int huffman_block(Bits& b, const HostSrc& s, Tables& t, uint8_t* dst, int64_t cap, int64_t mstart, int64_t& out) {
  const Huff lit = lit_huff(t), dist = dist_huff(t);
  for (;;) {
    bits_fill(b, s);
    const int sym = huff_decode(b, lit);
    if (sym < 0 || sym > 285) return bits_truncated(b) ? VX_INFLATE_TRUNCATED : VX_INFLATE_BAD_SYMBOL;
    if (sym < 256) {
      if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
      if (out + 1 > cap) return VX_INFLATE_CAPACITY;
      dst[out++] = (uint8_t)sym;
      continue;
    }
    if (sym == 256) return bits_truncated(b) ? VX_INFLATE_TRUNCATED : 0;
    const int len = len_base(sym) + (int)bits_get(b, s, len_extra(sym));
    bits_fill(b, s);
    const int ds = huff_decode(b, dist);
    if (ds < 0 || ds > 29) return bits_truncated(b) ? VX_INFLATE_TRUNCATED : VX_INFLATE_BAD_SYMBOL;
    const int d = dist_base(ds) + (int)bits_get(b, s, dist_extra(ds));
    if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
    if (d > out - mstart) return VX_INFLATE_BAD_DISTANCE;
    if (out + len > cap) return VX_INFLATE_CAPACITY;
    for (int k = 0; k < len; ++k, ++out) dst[out] = dst[out - d];
  }
}

int inflate_host(const uint8_t* src, int64_t n, int fmt, uint8_t* dst, int64_t cap, int64_t* out_size) {
  static Tables t;
  const HostSrc s{src, n};
  Bits b = bits_init(n);
  int64_t out = 0;
  int st = 0;
  for (;;) {   // members: each one consumes its header, so the loop ends with the input
    const int64_t mstart = out;
    if (fmt == VX_INFLATE_GZIP) st = gzip_header(b, s);
    else if (fmt == VX_INFLATE_ZLIB) st = zlib_header(b, s);
    if (st) break;
    int final = 0;
    do {
      final = (int)bits_get(b, s, 1);
      const int type = (int)bits_get(b, s, 2);
      if (bits_truncated(b)) { st = VX_INFLATE_TRUNCATED; break; }
      if (type == 0) {
        int len = 0;
        int64_t data = 0;
        st = stored_header(b, s, &len, &data);
        if (st) break;
        if (out + len > cap) { st = VX_INFLATE_CAPACITY; break; }
        if (len) memcpy(dst + out, src + data, (size_t)len);
        out += len;
        bits_seek(b, s, data + len);
      } else if (type == 3) {
        st = VX_INFLATE_BAD_BLOCK;
      } else {
        if (type == 1) fixed_lens(t);
        else st = dynamic_lens(b, s, t);
        if (!st) st = prepare_block(t);
        if (st) break;
        huff_build(lit_huff(t));
        huff_build(dist_huff(t));
        st = huffman_block(b, s, t, dst, cap, mstart, out);
      }
    } while (!final && !st);
    if (st) break;
    bits_align(b);
    if (fmt == VX_INFLATE_RAW) {
      if (bits_bytepos(b) < n) st = VX_INFLATE_TRAILING;
      break;
    }
    if (fmt == VX_INFLATE_ZLIB) {
      const uint32_t ad = trailer_u32(b, s, true);
      if (bits_truncated(b)) st = VX_INFLATE_TRUNCATED;
      else if (ad != adler32_of(dst + mstart, out - mstart)) st = VX_INFLATE_BAD_CHECK;
      else if (bits_bytepos(b) < n) st = VX_INFLATE_TRAILING;
      break;
    }
    const uint32_t crc = trailer_u32(b, s, false);
    const uint32_t isz = trailer_u32(b, s, false);
    if (bits_truncated(b)) { st = VX_INFLATE_TRUNCATED; break; }
    if (crc != crc32_of(dst + mstart, out - mstart)) { st = VX_INFLATE_BAD_CHECK; break; }
    if (isz != (uint32_t)(out - mstart)) { st = VX_INFLATE_BAD_ISIZE; break; }
    const int nx = gzip_next(b, s);
    if (nx == 1) continue;
    st = nx;
    break;
  }
  *out_size = out;
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: inflate_host IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) { perror("inflate_host"); return 2; }
  for (;;) {
    int32_t hdr[2];
    int64_t cap, n;
    if (fread(hdr, sizeof hdr, 1, f) != 1) break;
    if (fread(&cap, 8, 1, f) != 1 || fread(&n, 8, 1, f) != 1 || cap < 0 || n < 0) return 3;
    // exact-size buffers (one byte for an empty one): the sanitizers see any access past the input or the capacity
    std::vector<uint8_t> src((size_t)(n ? n : 1)), dst((size_t)(cap ? cap : 1));
    if (n && fread(src.data(), 1, (size_t)n, f) != (size_t)n) return 3;
    int64_t size = 0;
    const int st = inflate_host(src.data(), n, hdr[0], dst.data(), cap, &size);
    const int32_t oh[2] = {st, 0};
    fwrite(oh, sizeof oh, 1, g);
    fwrite(&size, 8, 1, g);
    if (size) fwrite(dst.data(), 1, (size_t)size, g);
  }
  fclose(f);
  fclose(g);
  return 0;
}
