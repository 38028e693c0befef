// The serial core of the TIFF LZW encoder (TIFF 6.0 section 13, Compression 5, with libtiff's policy), shared by the
// batched device encoder (tiff_lzw_enc.hip) and the host program the CPU tests build with g++ (tests/lzw_enc_host.cpp).
// Plain C++: every function compiles as device code under hipcc and as host code under g++.
//
// The strip: ClearCode 256 first; greedy longest match; codes packed MSB first, 9 bits wide at the start, "early
// change" (lzw_enc_width); a ClearCode when the next free entry would be 4094 (LZWE_CLEAR_AT), after which the match
// goes on from the byte that ended the last one; EndOfInformation 257 last, the last byte zero-padded.  Greedy matching
// with a fixed reset rule has one output per input: the strip is the one libtiff's encoder policy gives.
//
// The dictionary is an open-addressing hash table of LZWE_SLOTS 32-bit slots, keyed by (prefix code, byte): a slot is
// key << 12 | code with key = prefix << 8 | byte (20 bits) and code the entry (12 bits); LZWE_EMPTY is no entry (it
// would be entry 4095 under prefix 4095, and no entry above 4093 is ever made).  Linear probing from a multiplicative
// hash.  Probing ends: between two ClearCodes at most 4094 - 258 = 3836 entries are made, so at least
// LZWE_SLOTS - 3836 slots are empty and a probe sequence meets one.
//
// The caller owns the table's memory and wipes it (all LZWE_EMPTY) at the start and whenever lzw_enc_byte returns true
// (a ClearCode went out): on the device the wave wipes it lane-parallel.  Codes go out through a sink of whole
// big-endian 32-bit words (sink.word(v): v holds the strip's next 4 bytes as they lie in memory on a little-endian
// machine); lzw_enc_finish pads the last word with zero bits and returns how many of its bytes belong to the strip.
//
// On the device every lane of the wave runs the core on the same state, so a slot loaded from the table is the same
// in all lanes.  The device build says so to the compiler (VX_LZWE_UNIFORM: the first lane's value), which then keeps the
// whole state in scalar registers and branches on it without lane masks; the caller does the same for the input byte.
//
// Safety contract: the core reads and writes the table at indices below LZWE_SLOTS only and hands out at most one word
// per byte taken (two codes of at most 12 bits each), at most two at the finish.
#pragma once
#include <stdint.h>

#include "../../include/values_amd.h"

#if defined(__HIPCC__)
#define VX_LZWE_HD __host__ __device__ __forceinline__
#else
#define VX_LZWE_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define VX_LZWE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define VX_LZWE_UNIFORM(x) ((uint32_t)(x))
#endif

namespace vxlzwe {

constexpr int LZWE_CLEAR = 256;
constexpr int LZWE_EOI = 257;
constexpr int LZWE_FIRST = 258;
constexpr int LZWE_CLEAR_AT = 4094;                          // a ClearCode once the next free entry would be this
constexpr int LZWE_MAX_ENTRIES = LZWE_CLEAR_AT - LZWE_FIRST;   // 3836 entries between two ClearCodes
constexpr int LZWE_SLOT_BITS = 13;
constexpr int LZWE_SLOTS = 1 << LZWE_SLOT_BITS;              // 8192 slots: 32 KiB
constexpr uint32_t LZWE_EMPTY = 0xFFFFFFFFu;

static_assert(LZWE_MAX_ENTRIES < LZWE_SLOTS, "probing ends at an empty slot");

// The largest strip n >= 0 input bytes can produce.  Every data code stands for at least one input byte: at most n
// data codes.  ClearCodes: one at the start, and one more after every LZWE_MAX_ENTRIES insertions; an insertion follows
// a data code that is not the last, so there are fewer than n insertions and at most n / 3836 further ClearCodes.  One
// EndOfInformation.  Each code is at most 12 bits wide, and the last byte is padded:
//   bytes <= (12 * (n + n / 3836 + 2) + 7) / 8.
VX_LZWE_HD int64_t lzw_enc_bound(int64_t n) { return (12 * (n + n / LZWE_MAX_ENTRIES + 2) + 7) / 8; }

// the width of the code that follows k codes since the last ClearCode: the decoder's next free entry is then
// 258 + k - 1 (one entry per code after the first), and the width grows when that reaches 511, 1023, 2047
VX_LZWE_HD int lzw_enc_width(int k) {
  const int nfree = LZWE_FIRST + (k > 1 ? k : 1) - 1;
  return 9 + (nfree >= 511) + (nfree >= 1023) + (nfree >= 2047);
}

VX_LZWE_HD uint32_t lzw_enc_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}

// lzw_enc_width kept as state: the width grows when k reaches 254, 766 and 1790 (each 2 g + 258 after the last); the 3838
// that follows is never reached: a ClearCode goes out at k = 3836
constexpr int LZWE_FIRST_GROW = 254;

struct LzwEnc {
  uint32_t* tab;   // LZWE_SLOTS slots
  int w;           // the code of the match so far, -1: none
  int k;           // codes since the last ClearCode
  int nxt;         // the next free entry
  int width;       // lzw_enc_width(k)
  int grow;        // the k at which the width grows next
  uint64_t acc;    // the low nbits bits are not yet handed out, the oldest highest
  int nbits;       // < 32 between calls
};

// one code into the packer, e.width bits wide
template <class Sink>
VX_LZWE_HD void lzw_enc_put(LzwEnc& e, Sink& sink, int code) {
  e.acc = (e.acc << e.width) | (uint32_t)code;
  e.nbits += e.width;
  if (e.nbits >= 32) {
    e.nbits -= 32;
    sink.word(lzw_enc_bswap((uint32_t)(e.acc >> e.nbits)));
  }
}

// a data code: one more code since the last ClearCode
template <class Sink>
VX_LZWE_HD void lzw_enc_put_data(LzwEnc& e, Sink& sink, int code) {
  lzw_enc_put(e, sink, code);
  if (++e.k == e.grow) {
    ++e.width;
    e.grow = 2 * e.grow + LZWE_FIRST;
  }
}

// ClearCode: the state of a strip's start (the table is the caller's to wipe)
template <class Sink>
VX_LZWE_HD void lzw_enc_put_clear(LzwEnc& e, Sink& sink) {
  lzw_enc_put(e, sink, LZWE_CLEAR);
  e.k = 0;
  e.nxt = LZWE_FIRST;
  e.width = 9;
  e.grow = LZWE_FIRST_GROW;
}

// the strip's first code; the table must be wiped
template <class Sink>
VX_LZWE_HD LzwEnc lzw_enc_init(uint32_t* tab, Sink& sink) {
  LzwEnc e{tab, -1, 0, LZWE_FIRST, 9, LZWE_FIRST_GROW, 0, 0};
  lzw_enc_put_clear(e, sink);
  return e;
}

VX_LZWE_HD uint32_t lzw_enc_hash(uint32_t key) { return (key * 2654435761u) >> (32 - LZWE_SLOT_BITS); }

// Takes the next input byte.  true: a ClearCode went out and the state is reset -- the caller wipes the table before
// the next call.
template <class Sink>
VX_LZWE_HD bool lzw_enc_byte(LzwEnc& e, Sink& sink, int c) {
  if (e.w < 0) {
    e.w = c;
    return false;
  }
  const uint32_t key = ((uint32_t)e.w << 8) | (uint32_t)c;
  uint32_t h = lzw_enc_hash(key);
  uint32_t slot = VX_LZWE_UNIFORM(e.tab[h]);
  while (slot != LZWE_EMPTY && (slot >> 12) != key) {
    h = (h + 1) & (LZWE_SLOTS - 1);
    slot = VX_LZWE_UNIFORM(e.tab[h]);
  }
  if (slot != LZWE_EMPTY) {
    e.w = (int)(slot & 0xFFFu);
    return false;
  }
  lzw_enc_put_data(e, sink, e.w);
  e.tab[h] = (key << 12) | (uint32_t)e.nxt;
  ++e.nxt;
  e.w = c;
  if (e.nxt >= LZWE_CLEAR_AT) {
    lzw_enc_put_clear(e, sink);
    return true;
  }
  return false;
}

// The pending match and EndOfInformation; -> the bytes of the last word handed out that belong to the strip (1 to 4), or
// 0 when the strip ended on a word boundary and no partial word was handed out.
template <class Sink>
VX_LZWE_HD int lzw_enc_finish(LzwEnc& e, Sink& sink) {
  if (e.w >= 0) {
    lzw_enc_put_data(e, sink, e.w);
    e.w = -1;
  }
  lzw_enc_put(e, sink, LZWE_EOI);
  if (e.nbits == 0) return 0;
  const int tail = (e.nbits + 7) / 8;
  sink.word(lzw_enc_bswap((uint32_t)(e.acc << (32 - e.nbits))));
  e.nbits = 0;
  return tail;
}

}  // namespace vxlzwe
