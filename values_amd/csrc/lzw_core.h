// The serial core of the TIFF LZW decoder (TIFF 6.0 section 13, Compression 5), shared by the batched device decoder
// (tiff_lzw.hip) and the host reference decoder the CPU tests build with g++ (tests/lzw_host.cpp).  Plain C++: every
// function compiles as device code under hipcc and as host code under g++.
//
// The format: codes packed MSB first, 9 bits wide at the start; ClearCode 256, EndOfInformation 257, first free entry
// 258.  "Early change": the width grows when the next free entry reaches 511, 1023 and 2047, never beyond 12 bits.  With
// a full table (4096 entries) and no ClearCode the decode goes on at 12 bits without adding entries, as libtiff's does.
// A code equal to the next free entry is the KwKwK string.  The old LSB-first variant is not decoded (its first code is
// not ClearCode: LZW_BAD).
//
// The table.  The string of entry 258 + i is the output that begins where the i-th code since the last ClearCode began,
// one byte longer than that code's string -- so the table is the output offsets pos[i] of those codes alone: entry
// 258 + i is out[pos[i], pos[i + 1]] (both ends included), and emitting a code is a copy from earlier output.  The copy
// of the KwKwK string overlaps its own first byte: it is written at pos[i + 1], one byte before its end.  pos[] has
// LZW_POS entries: i + 1 <= 3838 for every entry a 12-bit code can name.
//
// Safety contract (the decoder runs on shared machines): lzw_step reads the input through the bit reader only (the
// source clamps: bytes beyond the end read as 0, and a code whose bits reach beyond the end is LZW_TRUNCATED, never
// acted on), indexes pos[] below LZW_POS only, and returns strings that lie wholly before `at` except for the KwKwK
// byte; every call consumes at least 9 bits, so a loop over it makes progress on the input.
#pragma once
#include <stdint.h>

#include "../../include/values_amd.h"

#if defined(__HIPCC__)
#define VX_LZW_HD __host__ __device__ __forceinline__
#else
#define VX_LZW_HD inline
#endif

namespace vxlzw {

constexpr int LZW_CLEAR = 256;
constexpr int LZW_EOI = 257;
constexpr int LZW_FIRST = 258;
constexpr int LZW_MAX_K = 4096 - LZW_FIRST + 1;   // 3839: the table is full once this many codes followed a ClearCode
constexpr int LZW_POS = LZW_MAX_K;                // pos[0 .. 3838]
constexpr int LZW_MAX_STRING = LZW_MAX_K;         // no string is longer (each entry is one byte longer than an earlier one)

// what lzw_step found
enum { LZW_STRING = 0, LZW_CLEARED = 1, LZW_END = 2, LZW_TRUNCATED = 3, LZW_BAD = 4 };

// ---------------------------------------------------------------------------------------------
// Bit reader, MSB first.  pos: next byte to load, a multiple of 4 from the stream start; the source's u32(pos) returns
// the 4 bytes at pos as a little-endian word with every byte at or beyond n read as 0.  The low cnt bits of buf are the
// bits not yet handed out, the oldest highest.
struct MBits {
  uint64_t buf;
  int cnt;
  int64_t pos;
  int64_t n;
};

VX_LZW_HD MBits mbits_init(int64_t n) { return MBits{0, 0, 0, n}; }
VX_LZW_HD bool mbits_truncated(const MBits& b) { return b.pos * 8 - b.cnt > b.n * 8; }
VX_LZW_HD uint32_t lzw_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}
// k in [1, 32] bits
template <class S>
VX_LZW_HD uint32_t mbits_get(MBits& b, const S& s, int k) {
  if (b.cnt <= 32) {
    b.buf = (b.buf << 32) | lzw_bswap(s.u32(b.pos));
    b.pos += 4;
    b.cnt += 32;
  }
  b.cnt -= k;
  return (uint32_t)(b.buf >> b.cnt) & (uint32_t)((1ull << k) - 1);
}

// ---------------------------------------------------------------------------------------------
// The state machine.  k: codes since the last ClearCode (saturating at LZW_MAX_K), -1 before the strip's first code.
struct Lzw {
  uint32_t* pos;   // LZW_POS entries
  int k;
  int width;
};

VX_LZW_HD Lzw lzw_init(uint32_t* pos) { return Lzw{pos, -1, 9}; }

// Decodes the next code; `at` is the output offset it begins at.  LZW_STRING: *lit >= 0 is a single byte, else the
// string is the *len bytes at output offset *from (*from < at, *from + *len <= at + 1).
template <class S>
VX_LZW_HD int lzw_step(Lzw& z, MBits& b, const S& s, uint32_t at, int* lit, uint32_t* from, uint32_t* len) {
  const int code = (int)mbits_get(b, s, z.width);
  if (mbits_truncated(b)) return LZW_TRUNCATED;
  if (code == LZW_CLEAR) {
    z.k = 0;
    z.width = 9;
    return LZW_CLEARED;
  }
  if (z.k < 0) return LZW_BAD;          // a strip begins with ClearCode
  if (code == LZW_EOI) return LZW_END;
  const int k = z.k;
  if (k < LZW_POS) z.pos[k] = at;
  if (code < 256) {
    *lit = code;
    *from = 0;
    *len = 1;
  } else {
    const int i = code - LZW_FIRST;     // <= 3837
    if (i >= k) return LZW_BAD;         // above the next free entry (258 + k - 1), or no string before it
    *lit = -1;
    *from = z.pos[i];
    *len = z.pos[i + 1] - z.pos[i] + 1;
    if (*len > (uint32_t)LZW_MAX_STRING || *from >= at) return LZW_BAD;   // not reachable: offsets rise by >= 1 per code
  }
  if (k < LZW_MAX_K) z.k = k + 1;
  // the next free entry is now 258 + k (one entry per code after the first)
  const int nfree = LZW_FIRST + k;
  z.width = 9 + (nfree >= 511) + (nfree >= 1023) + (nfree >= 2047);
  return LZW_STRING;
}

}  // namespace vxlzw
