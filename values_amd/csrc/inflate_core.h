// The serial core of the DEFLATE decoder (RFC 1951) and its gzip (RFC 1952) / zlib (RFC 1950) framing, shared by the
// batched device decoder (inflate.hip) and the host reference decoder the CPU tests build with g++
// (tests/inflate_host.cpp).  Plain C++: every function compiles as device code under hipcc and as host code under g++.
//
// The pieces: a 64-bit little-endian bit reader over a byte source that returns 0 beyond the end (the source decides
// where the bytes live: host memory, or an LDS window in front of device memory), the gzip / zlib header parsers, the
// stored-block header, the dynamic-block header (code-length code, then the literal/length and distance lengths), and
// canonical Huffman tables.
//
// Safety contract (the decoder runs on shared machines): no input makes these functions read or write outside the
// arrays they are given, and every loop is bounded.  The reader never reads past the source's end (the source clamps);
// it reports truncation when the bits it handed out reach past the end (bits_truncated), and every caller checks that
// BEFORE it acts on what it read, so a truncated stream is reported as truncated, not as whatever the zero fill decodes
// to.  A code-length set is validated (over-subscribed refused, incomplete refused except where zlib allows it: a
// literal/length or distance code with a single code of length 1, or a distance code with no codes) before any table
// built from it is used, and a table lookup that finds no code is VX_INFLATE_BAD_SYMBOL.
//
// Tables: a primary lookup of FB bits (entry = symbol << 4 | code length, 0 = no code of <= FB bits starts with these
// bits) and, for the longer codes, the canonical (count, sorted symbols) walk of puff.c, at most 15 steps.
#pragma once
#include <stdint.h>

#include "../../include/values_amd.h"

#if defined(__HIPCC__)
#define VX_HD __host__ __device__ __forceinline__
#else
#define VX_HD inline
#endif

namespace vxinf {

constexpr int LIT_FB = 10;     // primary lookup bits, literal/length code
constexpr int DIST_FB = 8;     // primary lookup bits, distance code
constexpr int CL_FB = 7;       // the code-length code has codes of at most 7 bits: one lookup
constexpr int MAX_BITS = 15;

struct Tables {
  uint16_t lit_fast[1 << LIT_FB];
  uint16_t dist_fast[1 << DIST_FB];
  uint16_t lit_count[16];
  uint16_t dist_count[16];
  uint16_t lit_sym[288];
  uint16_t dist_sym[32];
  uint16_t offs[16];           // huff_prepare's running offsets
  uint8_t lens[320];           // literal/length lengths [0, 288), distance lengths [288, 320)
};

struct Huff {
  uint16_t* fast;
  uint16_t* count;
  uint16_t* sym;
  uint16_t* offs;
  int fb;
};

VX_HD Huff lit_huff(Tables& t) { return Huff{t.lit_fast, t.lit_count, t.lit_sym, t.offs, LIT_FB}; }
VX_HD Huff dist_huff(Tables& t) { return Huff{t.dist_fast, t.dist_count, t.dist_sym, t.offs, DIST_FB}; }
VX_HD Huff cl_huff(Tables& t) { return Huff{t.lit_fast, t.lit_count, t.lit_sym, t.offs, CL_FB}; }   // reuses the literal slots

// ---------------------------------------------------------------------------------------------
// Bit reader.  pos: next byte to load, always a multiple of 4 from the stream start; the source's u32(pos) returns the
// 4 little-endian bytes at pos with every byte at or beyond n read as 0.
struct Bits {
  uint64_t buf;
  int cnt;
  int64_t pos;
  int64_t n;
};

VX_HD Bits bits_init(int64_t n) { return Bits{0, 0, 0, n}; }
// bits handed out so far
VX_HD int64_t bits_used(const Bits& b) { return b.pos * 8 - b.cnt; }
VX_HD bool bits_truncated(const Bits& b) { return bits_used(b) > b.n * 8; }
template <class S>
VX_HD void bits_fill(Bits& b, const S& s) {
  if (b.cnt <= 32) {
    b.buf |= (uint64_t)s.u32(b.pos) << b.cnt;
    b.pos += 4;
    b.cnt += 32;
  }
}
// k <= 32 bits, LSB first, from a filled reader
VX_HD uint32_t bits_peek(const Bits& b, int k) { return (uint32_t)(b.buf & ((k >= 32) ? 0xFFFFFFFFull : ((1ull << k) - 1))); }
VX_HD void bits_drop(Bits& b, int k) {
  b.buf >>= k;
  b.cnt -= k;
}
template <class S>
VX_HD uint32_t bits_get(Bits& b, const S& s, int k) {
  bits_fill(b, s);
  const uint32_t v = bits_peek(b, k);
  bits_drop(b, k);
  return v;
}
VX_HD void bits_align(Bits& b) { bits_drop(b, b.cnt & 7); }
// byte position of a byte-aligned reader
VX_HD int64_t bits_bytepos(const Bits& b) { return b.pos - (b.cnt >> 3); }
// restart the reader at byte p (>= 0)
template <class S>
VX_HD void bits_seek(Bits& b, const S& s, int64_t p) {
  b.pos = p & ~(int64_t)3;
  b.buf = 0;
  b.cnt = 0;
  bits_fill(b, s);
  bits_drop(b, (int)(p & 3) * 8);
}

// ---------------------------------------------------------------------------------------------
// Symbol values.  lit/len: 257 + (0..28) lengths, 285 = 258; distance: 30 codes.
VX_HD int len_base(int sym) {   // sym in [257, 285]
  if (sym < 265) return sym - 254;
  if (sym == 285) return 258;
  const int e = (sym - 261) >> 2;
  return ((4 + ((sym - 265) & 3)) << e) + 3;
}
VX_HD int len_extra(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
VX_HD int dist_base(int sym) {  // sym in [0, 29]
  if (sym < 4) return sym + 1;
  const int e = (sym >> 1) - 1;
  return ((2 + (sym & 1)) << e) + 1;
}
VX_HD int dist_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// the order in which the code-length code's lengths are stored: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, packed
// 5 bits per entry into two words (an indexed local array would live in scratch on the device)
constexpr uint64_t cl_pack(int from, int to) {
  const int ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint64_t v = 0;
  for (int i = from; i < to; ++i) v |= (uint64_t)ord[i] << (5 * (i - from));
  return v;
}
VX_HD int cl_order(int i) {
  constexpr uint64_t A = cl_pack(0, 12), B = cl_pack(12, 19);
  return i < 12 ? (int)((A >> (5 * i)) & 31) : (int)((B >> (5 * (i - 12))) & 31);
}

enum { CODE_CL = 0, CODE_LIT = 1, CODE_DIST = 2 };

// counts, sorted symbols and validation of the lengths lens[0, n) (n <= 288).  0 or VX_INFLATE_BAD_LENGTHS.
VX_HD int huff_prepare(const uint8_t* lens, int n, Huff h, int kind) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int s = 0; s < n; ++s) h.count[lens[s] & 15]++;
  int left = 1, maxlen = 0;
  for (int l = 1; l <= MAX_BITS; ++l) {
    left <<= 1;
    left -= h.count[l];
    if (left < 0) return VX_INFLATE_BAD_LENGTHS;   // over-subscribed
    if (h.count[l]) maxlen = l;
  }
  if (left > 0) {
    // incomplete: zlib accepts it for a literal/length or distance code whose only code has length 1, and for a
    // distance code without codes (a block of literals only); the code-length code must be complete
    const bool single = maxlen == 1 && h.count[1] == 1;
    if (kind == CODE_CL || !(single || (kind == CODE_DIST && maxlen == 0))) return VX_INFLATE_BAD_LENGTHS;
  }
  // sorted symbols: by length, then by symbol
  h.offs[1] = 0;
  for (int l = 1; l < MAX_BITS; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
  for (int s = 0; s < n; ++s) {
    const int l = lens[s] & 15;
    if (l) h.sym[h.offs[l]++] = (uint16_t)s;
  }
  h.count[0] = 0;
  return 0;
}

VX_HD uint32_t bit_reverse(uint32_t v, int k) {
  uint32_t r = 0;
  for (int i = 0; i < k; ++i) {
    r = (r << 1) | (v & 1);
    v >>= 1;
  }
  return r;
}

// the primary lookup: entries [first, 1 << fb) step stride cleared, then the codes of sorted index [first, total) step
// stride written (the device decoder spreads both over its 64 lanes; the host calls them with 0, 1).  Only after
// huff_prepare accepted the lengths: a code's entries never overlap another code's.
VX_HD void huff_clear(Huff h, int first, int stride) {
  for (int i = first; i < (1 << h.fb); i += stride) h.fast[i] = 0;
}
VX_HD void huff_fill(Huff h, int first, int stride) {
  int total = 0;
  for (int l = 1; l <= h.fb; ++l) total += h.count[l];
  for (int idx = first; idx < total; idx += stride) {
    // length and canonical code of sorted index idx (idx < total: the walk ends by l = fb)
    int l = 1, base = 0, code = 0;
    for (; l < h.fb; ++l) {
      if (idx < base + h.count[l]) break;
      base += h.count[l];
      code = (code + h.count[l]) << 1;
    }
    code += idx - base;
    const uint32_t r = bit_reverse((uint32_t)code, l);
    const uint16_t e = (uint16_t)((h.sym[idx] << 4) | l);
    for (uint32_t k = r; k < (1u << h.fb); k += (1u << l)) h.fast[k] = e;
  }
}
VX_HD void huff_build(Huff h) {
  huff_clear(h, 0, 1);
  huff_fill(h, 0, 1);
}

// decode one symbol from a filled reader (>= 15 bits).  -1: no code (an incomplete set's missing codes).
VX_HD int huff_decode(Bits& b, Huff h) {
  const uint16_t e = h.fast[b.buf & ((1u << h.fb) - 1)];
  if (e & 15) {
    bits_drop(b, e & 15);
    return e >> 4;
  }
  // canonical walk (puff.c decode) for the codes longer than the primary lookup
  int code = 0, first = 0, index = 0;
  uint64_t v = b.buf;
  for (int l = 1; l <= MAX_BITS; ++l) {
    code |= (int)(v & 1);
    v >>= 1;
    const int count = h.count[l];
    if (code - count < first) {
      bits_drop(b, l);
      return h.sym[index + (code - first)];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// ---------------------------------------------------------------------------------------------
// Block headers.

// the fixed code (BTYPE 1): lengths into t.lens
VX_HD void fixed_lens(Tables& t) {
  for (int s = 0; s < 288; ++s) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  for (int s = 0; s < 32; ++s) t.lens[288 + s] = 5;
}

// the dynamic header (BTYPE 2) after the 3 block-header bits: lens[0, hlit) and lens[288, 288 + hdist), the rest 0.
// The code-length code's table is built here (serially) into the literal slots.  0 or a status.
template <class S>
VX_HD int dynamic_lens(Bits& b, const S& s, Tables& t) {
  const int hlit = (int)bits_get(b, s, 5) + 257;
  const int hdist = (int)bits_get(b, s, 5) + 1;
  const int hclen = (int)bits_get(b, s, 4) + 4;
  if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
  if (hlit > 286 || hdist > 30) return VX_INFLATE_BAD_LENGTHS;
  for (int i = 0; i < 320; ++i) t.lens[i] = 0;
  // the code-length code's 19 lengths go to lens[300, 319) (outside both codes' ranges until the loop below)
  uint8_t* cl = t.lens + 300;
  for (int i = 0; i < hclen; ++i) cl[cl_order(i)] = (uint8_t)bits_get(b, s, 3);
  if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
  Huff ch = cl_huff(t);
  if (huff_prepare(cl, 19, ch, CODE_CL)) return VX_INFLATE_BAD_LENGTHS;
  huff_build(ch);
  for (int i = 300; i < 320; ++i) t.lens[i] = 0;
  // hlit + hdist lengths in one run-length alphabet: every step writes >= 1 length or fails
  int i = 0;
  const int total = hlit + hdist;
  while (i < total) {
    bits_fill(b, s);
    const int sym = huff_decode(b, ch);
    if (sym < 0) return bits_truncated(b) ? VX_INFLATE_TRUNCATED : VX_INFLATE_BAD_LENGTHS;
    int len = 0, rep = 1;
    if (sym < 16) {
      len = sym;
    } else if (sym == 16) {
      if (i == 0) return bits_truncated(b) ? VX_INFLATE_TRUNCATED : VX_INFLATE_BAD_LENGTHS;
      len = t.lens[(i - 1) < hlit ? (i - 1) : 288 + (i - 1 - hlit)];
      rep = 3 + (int)bits_get(b, s, 2);
    } else if (sym == 17) {
      rep = 3 + (int)bits_get(b, s, 3);
    } else {
      rep = 11 + (int)bits_get(b, s, 7);
    }
    if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
    if (i + rep > total) return VX_INFLATE_BAD_LENGTHS;
    for (int k = 0; k < rep; ++k, ++i) t.lens[i < hlit ? i : 288 + (i - hlit)] = (uint8_t)len;
  }
  if (t.lens[256] == 0) return VX_INFLATE_BAD_LENGTHS;   // no end-of-block code
  return 0;
}

// validation and sorted symbols of both codes from t.lens (the caller then builds the primary lookups)
VX_HD int prepare_block(Tables& t) {
  if (huff_prepare(t.lens, 288, lit_huff(t), CODE_LIT)) return VX_INFLATE_BAD_LENGTHS;
  if (huff_prepare(t.lens + 288, 32, dist_huff(t), CODE_DIST)) return VX_INFLATE_BAD_LENGTHS;
  return 0;
}

// stored block (BTYPE 0) after the 3 block-header bits: *len and the byte position of its data.  0 or a status.
template <class S>
VX_HD int stored_header(Bits& b, const S& s, int* len, int64_t* data) {
  bits_align(b);
  const uint32_t l = bits_get(b, s, 16);
  const uint32_t nl = bits_get(b, s, 16);
  if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
  if ((l ^ 0xFFFFu) != nl) return VX_INFLATE_BAD_STORED;
  *len = (int)l;
  *data = bits_bytepos(b);
  if (*data + (int64_t)l > b.n) return VX_INFLATE_TRUNCATED;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Framing.

// gzip member header (RFC 1952) at the byte-aligned reader; FEXTRA / FNAME / FCOMMENT / FHCRC are skipped (the header
// CRC is not checked, as Python's gzip does not).  Every name / comment byte consumes 8 bits: bounded by n.
template <class S>
VX_HD int gzip_header(Bits& b, const S& s) {
  const uint32_t id = bits_get(b, s, 16);
  const uint32_t cm = bits_get(b, s, 8);
  const uint32_t flg = bits_get(b, s, 8);
  bits_get(b, s, 32);   // MTIME
  bits_get(b, s, 16);   // XFL, OS
  if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
  if (id != 0x8B1Fu || cm != 8 || (flg & 0xE0u)) return VX_INFLATE_BAD_HEADER;
  if (flg & 4u) {       // FEXTRA
    const uint32_t xlen = bits_get(b, s, 16);
    if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
    const int64_t p = bits_bytepos(b) + xlen;
    if (p > b.n) return VX_INFLATE_TRUNCATED;
    bits_seek(b, s, p);
  }
  for (uint32_t f = 8; f <= 16; f <<= 1) {   // FNAME, FCOMMENT: zero-terminated
    if (!(flg & f)) continue;
    for (;;) {
      const uint32_t c = bits_get(b, s, 8);
      if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
      if (c == 0) break;
    }
  }
  if (flg & 2u) {       // FHCRC
    bits_get(b, s, 16);
    if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
  }
  return 0;
}

// zlib header (RFC 1950)
template <class S>
VX_HD int zlib_header(Bits& b, const S& s) {
  const uint32_t cmf = bits_get(b, s, 8);
  const uint32_t flg = bits_get(b, s, 8);
  if (bits_truncated(b)) return VX_INFLATE_TRUNCATED;
  if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u) return VX_INFLATE_BAD_HEADER;
  if (flg & 0x20u) return VX_INFLATE_DICT;
  return 0;
}

// a 32-bit trailer word at the byte-aligned reader (little endian: gzip CRC-32 / ISIZE; big endian: zlib Adler-32)
template <class S>
VX_HD uint32_t trailer_u32(Bits& b, const S& s, bool big_endian) {
  const uint32_t v = bits_get(b, s, 32);
  return big_endian ? ((v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24)) : v;
}

// after a gzip member's trailer: skip zero padding (Python's gzip.decompress does), then 1 = another member follows,
// 0 = the end, VX_INFLATE_TRAILING = other bytes
template <class S>
VX_HD int gzip_next(Bits& b, const S& s) {
  while (bits_bytepos(b) < b.n) {
    bits_fill(b, s);
    const uint32_t c = bits_peek(b, 8);
    if (c == 0x1F) return bits_bytepos(b) + 1 < b.n && ((b.buf >> 8) & 0xFF) == 0x8B ? 1 : VX_INFLATE_TRAILING;
    if (c != 0) return VX_INFLATE_TRAILING;
    bits_drop(b, 8);
  }
  return 0;
}

}  // namespace vxinf
