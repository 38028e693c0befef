// The DEFLATE chunk kernel: 32 KiB of an item in, one byte-aligned raw DEFLATE fragment out.  gzip.hip (gzip members) and
// png.hip (zlib streams inside PNG files) both run it; it is compiled here, once, and they reach it through the two host
// functions at the end of this file (declared in deflate_chunk.h).  gzip.hip's header comment describes the kernel step
// by step.
//
// Every store in this file is a plain C++ store of a vector register.
#include "deflate_chunk.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Huffman code lengths.  sortkey/sortsym: scratch for n symbols.  Called by one whole wave (64 lanes): the rank sort is
// lane-parallel, the minimum-redundancy construction and the length limit are serial on lane 0.
__device__ void huff_lengths(const uint32_t* freq, int n, int limit, uint8_t* len_out, uint32_t* sortkey, uint16_t* sortsym,
                             int* num) {
  const int lane = threadIdx.x & 63;
  int used = 0;
  for (int i = lane; i < n; i += 64) {
    const uint32_t f = freq[i];
    len_out[i] = 0;
    if (f) {
      int r = 0;
      for (int j = 0; j < n; ++j) {
        const uint32_t g = freq[j];
        r += g && (g < f || (g == f && j < i));
      }
      sortkey[r] = f;
      sortsym[r] = (uint16_t)i;
    }
  }
  for (int i = lane; i < n; i += 64) used += freq[i] != 0;
  for (int off = 32; off > 0; off >>= 1) used += __shfl_xor(used, off, 64);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (lane == 0 && used > 0) {
    uint32_t* A = sortkey;
    if (used == 1) {
      len_out[sortsym[0]] = 1;
    } else {
      // in-place minimum-redundancy code lengths of ascending frequencies (Moffat & Katajainen)
      const int m = used;
      A[0] += A[1];
      int root = 0, leaf = 2;
      for (int next = 1; next < m - 1; ++next) {
        if (leaf >= m || A[root] < A[leaf]) {
          A[next] = A[root];
          A[root++] = (uint32_t)next;
        } else {
          A[next] = A[leaf++];
        }
        if (leaf >= m || (root < next && A[root] < A[leaf])) {
          A[next] += A[root];
          A[root++] = (uint32_t)next;
        } else {
          A[next] += A[leaf++];
        }
      }
      A[m - 2] = 0;
      for (int next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
      int avbl = 1, usedn = 0, dpth = 0, root2 = m - 2, next2 = m - 1;
      while (avbl > 0) {
        while (root2 >= 0 && (int)A[root2] == dpth) { ++usedn; --root2; }
        while (avbl > usedn) { A[next2--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * usedn;
        ++dpth;
        usedn = 0;
      }
      // length histogram, limited to `limit` bits (Kraft sum brought back to exactly 1)
      for (int i = 0; i <= 32; ++i) num[i] = 0;
      for (int i = 0; i < m; ++i) num[A[i] > 32 ? 32 : A[i]]++;
      for (int i = limit + 1; i <= 32; ++i) { num[limit] += num[i]; num[i] = 0; }
      uint32_t total = 0;
      for (int i = limit; i > 0; --i) total += (uint32_t)num[i] << (limit - i);
      while (total != (1u << limit)) {
        num[limit]--;
        for (int i = limit - 1; i > 0; --i) {
          if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        }
        total--;
      }
      // the most frequent symbols (end of the ascending order) get the shortest codes
      int j = m;
      for (int i = 1; i <= limit; ++i)
        for (int k = num[i]; k > 0; --k) len_out[sortsym[--j]] = (uint8_t)i;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for LSB-first emission; one lane.  tmp: 32 ints of LDS
__device__ void huff_codes(const uint8_t* len, int n, uint16_t* code, int* tmp) {
  int* bl_count = tmp;
  int* next_code = tmp + 16;
  for (int i = 0; i < 16; ++i) bl_count[i] = 0;
  for (int i = 0; i < n; ++i) bl_count[len[i]]++;
  bl_count[0] = 0;
  int c = 0;
  for (int b = 1; b < 16; ++b) {
    c = (c + bl_count[b - 1]) << 1;
    next_code[b] = c;
  }
  for (int i = 0; i < n; ++i) {
    const int l = len[i];
    if (l) {
      const uint32_t v = (uint32_t)next_code[l]++;
      code[i] = (uint16_t)(__builtin_bitreverse32(v) >> (32 - l));
    } else {
      code[i] = 0;
    }
  }
}

__device__ __forceinline__ void len_sym(int L, int& sym, int& ebits, int& evalue) {
  if (L == 258) { sym = 285; ebits = 0; evalue = 0; return; }
  const int v = L - 3;
  if (v < 8) { sym = 257 + v; ebits = 0; evalue = 0; return; }
  const int hb = 31 - __builtin_clz((unsigned)v);
  sym = 257 + 4 * (hb - 1) + ((v >> (hb - 2)) & 3);
  ebits = hb - 2;
  evalue = v & ((1 << ebits) - 1);
}
__device__ __forceinline__ void dist_sym(int D, int& sym, int& ebits, int& evalue) {
  const int v = D - 1;
  if (v < 4) { sym = v; ebits = 0; evalue = 0; return; }
  const int hb = 31 - __builtin_clz((unsigned)v);
  sym = 2 * hb + ((v >> (hb - 1)) & 1);
  ebits = hb - 1;
  evalue = v & ((1 << ebits) - 1);
}
__device__ __forceinline__ int fixed_lit_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }
__device__ __forceinline__ uint32_t fixed_lit_code(int s) {
  uint32_t c;
  int l;
  if (s < 144) { c = 0x30 + s; l = 8; }
  else if (s < 256) { c = 0x190 + (s - 144); l = 9; }
  else if (s < 280) { c = s - 256; l = 7; }
  else { c = 0xC0 + (s - 280); l = 8; }
  return __builtin_bitreverse32(c) >> (32 - l);
}

// OR `n` (<= 32) bits of v into the LDS bit stream at bit position pos
__device__ __forceinline__ void put_bits(uint32_t* o, uint32_t pos, uint32_t v, int n) {
  if (n == 0) return;
  const uint32_t w = pos >> 5, s = pos & 31;
  atomicOr(&o[w], v << s);
  if (s + n > 32) atomicOr(&o[w + 1], v >> (32 - s));
}

__constant__ uint8_t kClenOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct GzShared {
  uint8_t buf[2 * GZ_CHUNK + 16];        // window (32 KiB before the chunk) + chunk; after the parse: the output bit stream
  int32_t head[GZ_HSIZE];                // hash table; after the parse: Huffman scratch
  uint16_t tok[GZ_SLICE * GZ_LANES];     // token stream of each lane, interleaved: entry k of lane l at k * 256 + l
  uint32_t lfreq[288];
  uint32_t dfreq[32];
  uint32_t cfreq[20];
  uint16_t lcode[288];
  uint16_t dcode[32];
  uint16_t ccode[20];
  uint8_t llen[288];
  uint8_t dlen[32];
  uint8_t clen[20];
  uint16_t rle[320];                     // code-length sequence: symbol | extra << 5
  uint32_t lane_bits[GZ_LANES];
  uint32_t crc[GZ_LANES];
  uint32_t crc_len[GZ_LANES];
  int32_t ntok[GZ_LANES];
  int32_t hlit, hdist, hclen, nrle;
  int32_t mode;                          // 0 stored, 1 fixed, 2 dynamic
  uint32_t hdr_bits, total_bits, out_bytes;
};

__device__ __forceinline__ uint32_t gz_hash(const uint8_t* b, int p) {
  const uint32_t v = (uint32_t)b[p] | ((uint32_t)b[p + 1] << 8) | ((uint32_t)b[p + 2] << 16);
  return (v * 2654435761u) >> (32 - GZ_HBITS);
}

__global__ __launch_bounds__(GZ_LANES) void gz_chunk_kernel(const GzItemDev* __restrict__ items,
                                                            const GzChunkDev* __restrict__ chunks,
                                                            GzChunkMeta* __restrict__ meta, uint8_t* __restrict__ slots) {
  extern __shared__ __align__(16) uint8_t smem_raw[];
  GzShared& S = *reinterpret_cast<GzShared*>(smem_raw);
  const int tid = threadIdx.x;
  const GzChunkDev ch = chunks[blockIdx.x];
  const GzItemDev it = items[ch.item];
  const int64_t cstart = (int64_t)ch.index * GZ_CHUNK;
  const int clen = (int)min64(GZ_CHUNK, it.n - cstart);
  const int wlen = (int)min64(GZ_CHUNK, cstart);
  const bool final_chunk = ch.index == it.nchunks - 1;
  const int base = GZ_CHUNK;          // LDS position of the chunk's first byte
  const int lo = base - wlen;         // first valid history position
  const int dend = base + clen;

  // 1. load window + chunk
  const uint8_t* g = it.src + (cstart - wlen);
  const int nload = wlen + clen;
  if ((((uintptr_t)g) & 3) == 0) {
    const uint32_t* g4 = reinterpret_cast<const uint32_t*>(g);
    uint32_t* b4 = reinterpret_cast<uint32_t*>(S.buf + lo);
    for (int i = tid; i < nload / 4; i += GZ_LANES) b4[i] = g4[i];
    for (int i = (nload & ~3) + tid; i < nload; i += GZ_LANES) S.buf[lo + i] = g[i];
  } else {
    for (int i = tid; i < nload; i += GZ_LANES) S.buf[lo + i] = g[i];
  }
  for (int i = tid; i < GZ_HSIZE; i += GZ_LANES) S.head[i] = -1;
  for (int i = tid; i < 288; i += GZ_LANES) S.lfreq[i] = 0;
  if (tid < 32) S.dfreq[tid] = 0;
  if (tid < 20) S.cfreq[tid] = 0;
  if (tid < 16) S.buf[dend + tid] = 0;
  __syncthreads();
  for (int p = lo + tid; p < base; p += GZ_LANES)
    if (p + 2 < dend) atomicMax(&S.head[gz_hash(S.buf, p)], p);

  // CRC of the lane's slice
  const int s0 = base + tid * GZ_SLICE;
  const int s1 = min(s0 + GZ_SLICE, dend);
  {
    uint32_t c = 0xFFFFFFFFu;
    for (int p = s0; p < s1; ++p) c = kCrc.byte[(c ^ S.buf[p]) & 0xFF] ^ (c >> 8);
    S.crc[tid] = c ^ 0xFFFFFFFFu;
    S.crc_len[tid] = s1 > s0 ? (uint32_t)(s1 - s0) : 0u;
  }
  __syncthreads();

  // 2. lock-step greedy parse of the lane's slice
  const int h0 = it.hint[0], h1 = it.hint[1], h2 = it.hint[2];
  int cursor = s0, nt = 0;
  for (int r = 0; r < GZ_SLICE; ++r) {
    const int p = s0 + r;
    if (p < s1 && cursor == p) {
      int best = 0, bestd = 0;
      const int maxl = min(258, s1 - p);
      if (maxl >= 3) {
        // nearest first: a later candidate replaces the choice only with a longer match (runs take distance 1)
        int cand[5] = {p - 1, h0 ? p - h0 : -1, h1 ? p - h1 : -1, h2 ? p - h2 : -1, S.head[gz_hash(S.buf, p)]};
        const uint8_t b0 = S.buf[p], b1 = S.buf[p + 1], b2 = S.buf[p + 2];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int q = cand[k];
          if (best >= maxl) break;
          if (q < lo || q >= p || p - q > GZ_CHUNK) continue;
          if (S.buf[q] != b0 || S.buf[q + 1] != b1 || S.buf[q + 2] != b2) continue;
          if (best >= 3 && S.buf[q + best] != S.buf[p + best]) continue;
          int L = 3;
          while (L < maxl && S.buf[q + L] == S.buf[p + L]) ++L;
          if (L > best) { best = L; bestd = p - q; }
        }
      }
      if (best >= 3) {
        S.tok[nt * GZ_LANES + tid] = (uint16_t)(0x8000u | (uint32_t)(best - 3));
        S.tok[(nt + 1) * GZ_LANES + tid] = (uint16_t)(bestd - 1);
        nt += 2;
        cursor += best;
      } else {
        S.tok[nt * GZ_LANES + tid] = S.buf[p];
        nt += 1;
        cursor += 1;
      }
    }
    __syncthreads();
    if (p < s1 && p + 2 < dend) atomicMax(&S.head[gz_hash(S.buf, p)], p);
    __syncthreads();
  }
  S.ntok[tid] = nt;

  // 3. histograms
  for (int k = 0; k < nt; ++k) {
    const uint32_t t = S.tok[k * GZ_LANES + tid];
    if (t & 0x8000u) {
      int sym, eb, ev;
      len_sym((int)(t & 0xFF) + 3, sym, eb, ev);
      atomicAdd(&S.lfreq[sym], 1u);
      dist_sym((int)S.tok[(k + 1) * GZ_LANES + tid] + 1, sym, eb, ev);
      atomicAdd(&S.dfreq[sym], 1u);
      ++k;
    } else {
      atomicAdd(&S.lfreq[t], 1u);
    }
  }
  __syncthreads();
  if (tid == 0) S.lfreq[256] = 1;   // end of block
  __syncthreads();

  // Huffman scratch lives in the hash table (no longer needed): [0, 288) keys + syms of the literal tree, [512, ...) distance
  uint32_t* scr = reinterpret_cast<uint32_t*>(S.head);
  uint32_t* dfreq_t = scr + 1536;    // distance frequencies with at least two symbols present
  if (tid < 30) dfreq_t[tid] = S.dfreq[tid] + (tid < 2 && S.dfreq[tid] == 0 ? 1u : 0u);
  __syncthreads();
  const int wave = tid >> 6;
  if (wave == 0) huff_lengths(S.lfreq, 286, 15, S.llen, scr, reinterpret_cast<uint16_t*>(scr + 300), reinterpret_cast<int*>(scr + 1800));
  else if (wave == 1) huff_lengths(dfreq_t, 30, 15, S.dlen, scr + 512, reinterpret_cast<uint16_t*>(scr + 560), reinterpret_cast<int*>(scr + 1850));
  __syncthreads();

  // code-length sequence (RLE 16 / 17 / 18) and its code
  uint32_t* cfreq_t = scr + 1600;
  if (tid == 0) {
    int hlit = 286, hdist = 30;
    while (hlit > 257 && S.llen[hlit - 1] == 0) --hlit;
    while (hdist > 1 && S.dlen[hdist - 1] == 0) --hdist;
    const int tot = hlit + hdist;
    int nr = 0, i = 0;
    while (i < tot) {
      const int v = i < hlit ? S.llen[i] : S.dlen[i - hlit];
      int run = 1;
      while (i + run < tot && (i + run < hlit ? S.llen[i + run] : S.dlen[i + run - hlit]) == v) ++run;
      if (v == 0) {
        int rr = run;
        while (rr >= 11) { const int k = min(rr, 138); S.rle[nr++] = (uint16_t)(18 | ((k - 11) << 5)); S.cfreq[18]++; rr -= k; }
        if (rr >= 3) { S.rle[nr++] = (uint16_t)(17 | ((rr - 3) << 5)); S.cfreq[17]++; rr = 0; }
        while (rr > 0) { S.rle[nr++] = 0; S.cfreq[0]++; --rr; }
      } else {
        S.rle[nr++] = (uint16_t)v;
        S.cfreq[v]++;
        int rr = run - 1;
        while (rr >= 3) { const int k = min(rr, 6); S.rle[nr++] = (uint16_t)(16 | ((k - 3) << 5)); S.cfreq[16]++; rr -= k; }
        while (rr > 0) { S.rle[nr++] = (uint16_t)v; S.cfreq[v]++; --rr; }
      }
      i += run;
    }
    S.hlit = hlit;
    S.hdist = hdist;
    S.nrle = nr;
    // the code-length code must be complete: at least two symbols
    int nz = 0;
    for (int k = 0; k < 19; ++k) { cfreq_t[k] = S.cfreq[k]; nz += S.cfreq[k] != 0; }
    for (int k = 0; k < 19 && nz < 2; ++k) if (!cfreq_t[k]) { cfreq_t[k] = 1; ++nz; }
  }
  __syncthreads();
  if (wave == 0) huff_lengths(cfreq_t, 19, 7, S.clen, scr + 1664, reinterpret_cast<uint16_t*>(scr + 1700), reinterpret_cast<int*>(scr + 1800));
  __syncthreads();

  // codes + block choice
  if (tid == 0) {
    int* tmp = reinterpret_cast<int*>(scr + 1900);
    huff_codes(S.llen, 286, S.lcode, tmp);
    huff_codes(S.dlen, 30, S.dcode, tmp);
    huff_codes(S.clen, 19, S.ccode, tmp);
    int hclen = 19;
    while (hclen > 4 && S.clen[kClenOrder[hclen - 1]] == 0) --hclen;
    S.hclen = hclen;
    uint64_t extra = 0, dyn = 0, fix = 0;
    for (int s = 0; s < 286; ++s) {
      const uint64_t f = S.lfreq[s];
      if (!f) continue;
      dyn += f * S.llen[s];
      fix += f * fixed_lit_len(s);
      if (s >= 265 && s < 285) extra += f * (uint64_t)((s - 261) / 4);
    }
    for (int s = 0; s < 30; ++s) {
      const uint64_t f = S.dfreq[s];
      if (!f) continue;
      dyn += f * S.dlen[s];
      fix += f * 5;
      if (s >= 4) extra += f * (uint64_t)((s - 2) / 2);
    }
    uint64_t hdr = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen;
    for (int k = 0; k < 19; ++k) hdr += (uint64_t)S.cfreq[k] * S.clen[k];
    hdr += 2ull * S.cfreq[16] + 3ull * S.cfreq[17] + 7ull * S.cfreq[18];
    dyn += hdr + extra;
    fix += 3 + extra;
    auto huff_bytes = [&](uint64_t bits) -> uint64_t { return final_chunk ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; };
    const uint64_t sb = 5 + (uint64_t)clen, fb = huff_bytes(fix), db = huff_bytes(dyn);
    int mode = 0;
    uint64_t bytes = sb;
    if (fb < bytes) { mode = 1; bytes = fb; }
    if (db < bytes) { mode = 2; bytes = db; }
    S.mode = mode;
    S.out_bytes = (uint32_t)bytes;
    S.hdr_bits = mode == 2 ? (uint32_t)hdr : 3u;
    S.total_bits = (uint32_t)(mode == 2 ? dyn : fix);
  }
  __syncthreads();
  const int mode = S.mode;
  uint8_t* slot = slots + (size_t)blockIdx.x * GZ_SLOT;

  // CRC of the chunk (every lane takes part)
  crc_join_block<GZ_LANES>(S.crc, S.crc_len);
  if (tid == 0) {
    meta[blockIdx.x].bytes = S.out_bytes;
    meta[blockIdx.x].crc = S.crc[0];
  }

  if (mode == 0) {
    // stored block: straight from the source
    if (tid == 0) {
      slot[0] = final_chunk ? 1 : 0;
      slot[1] = (uint8_t)(clen & 0xFF);
      slot[2] = (uint8_t)(clen >> 8);
      slot[3] = (uint8_t)(~clen & 0xFF);
      slot[4] = (uint8_t)((~clen >> 8) & 0xFF);
    }
    const uint8_t* c = it.src + cstart;
    for (int i = tid; i < clen; i += GZ_LANES) slot[5 + i] = c[i];
    return;
  }

  // 4. bit counts of the lanes' tokens under the chosen code, exclusive scan
  uint32_t bits = 0;
  for (int k = 0; k < nt; ++k) {
    const uint32_t t = S.tok[k * GZ_LANES + tid];
    if (t & 0x8000u) {
      int sym, eb, ev;
      len_sym((int)(t & 0xFF) + 3, sym, eb, ev);
      bits += (mode == 2 ? S.llen[sym] : fixed_lit_len(sym)) + eb;
      dist_sym((int)S.tok[(k + 1) * GZ_LANES + tid] + 1, sym, eb, ev);
      bits += (mode == 2 ? S.dlen[sym] : 5) + eb;
      ++k;
    } else {
      bits += mode == 2 ? S.llen[t] : fixed_lit_len((int)t);
    }
  }
  S.lane_bits[tid] = bits;
  // the bit stream goes where the input was: clear it
  uint32_t* o = reinterpret_cast<uint32_t*>(S.buf);
  const int nwords = (int)((S.out_bytes + 3) / 4) + 2;
  __syncthreads();
  for (int i = tid; i < nwords; i += GZ_LANES) o[i] = 0;
  if (tid == 0) {
    uint32_t acc = S.hdr_bits;
    for (int l = 0; l < GZ_LANES; ++l) {
      const uint32_t b = S.lane_bits[l];
      S.lane_bits[l] = acc;
      acc += b;
    }
  }
  __syncthreads();

  // 5. block header, tokens, end of block, byte alignment
  if (tid == 0) {
    uint32_t pos = 0;
    put_bits(o, pos, (final_chunk ? 1u : 0u) | ((uint32_t)mode << 1), 3);
    pos += 3;
    if (mode == 2) {
      put_bits(o, pos, (uint32_t)(S.hlit - 257), 5); pos += 5;
      put_bits(o, pos, (uint32_t)(S.hdist - 1), 5); pos += 5;
      put_bits(o, pos, (uint32_t)(S.hclen - 4), 4); pos += 4;
      for (int k = 0; k < S.hclen; ++k) { put_bits(o, pos, S.clen[kClenOrder[k]], 3); pos += 3; }
      for (int k = 0; k < S.nrle; ++k) {
        const int sym = S.rle[k] & 31, ex = S.rle[k] >> 5;
        put_bits(o, pos, S.ccode[sym], S.clen[sym]);
        pos += S.clen[sym];
        const int eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        put_bits(o, pos, (uint32_t)ex, eb);
        pos += eb;
      }
    }
  }
  {
    uint32_t pos = S.lane_bits[tid];
    for (int k = 0; k < nt; ++k) {
      const uint32_t t = S.tok[k * GZ_LANES + tid];
      if (t & 0x8000u) {
        int sym, eb, ev;
        len_sym((int)(t & 0xFF) + 3, sym, eb, ev);
        const int cl = mode == 2 ? S.llen[sym] : fixed_lit_len(sym);
        put_bits(o, pos, mode == 2 ? S.lcode[sym] : fixed_lit_code(sym), cl);
        pos += cl;
        put_bits(o, pos, (uint32_t)ev, eb);
        pos += eb;
        dist_sym((int)S.tok[(k + 1) * GZ_LANES + tid] + 1, sym, eb, ev);
        const int dl = mode == 2 ? S.dlen[sym] : 5;
        put_bits(o, pos, mode == 2 ? S.dcode[sym] : (__builtin_bitreverse32((uint32_t)sym) >> 27), dl);
        pos += dl;
        put_bits(o, pos, (uint32_t)ev, eb);
        pos += eb;
        ++k;
      } else {
        const int cl = mode == 2 ? S.llen[t] : fixed_lit_len((int)t);
        put_bits(o, pos, mode == 2 ? S.lcode[t] : fixed_lit_code((int)t), cl);
        pos += cl;
      }
    }
  }
  if (tid == GZ_LANES - 1) {
    uint32_t pos = S.total_bits - (mode == 2 ? S.llen[256] : 7u);
    put_bits(o, pos, mode == 2 ? S.lcode[256] : 0u, mode == 2 ? S.llen[256] : 7);
    if (!final_chunk) {
      // empty stored block: BFINAL 0, BTYPE 00, pad to the byte, LEN 0x0000, NLEN 0xFFFF
      pos = S.total_bits + 3;
      const uint32_t byte = (pos + 7) / 8;
      put_bits(o, byte * 8 + 16, 0xFFFFu, 16);
    }
  }
  __syncthreads();
  const uint8_t* ob = S.buf;
  const int nb = (int)S.out_bytes;
  for (int i = tid; i < nb; i += GZ_LANES) slot[i] = ob[i];
}

}  // namespace

void gz_fill_tables(const vx_gz_item* recs, int n, GzItemDev* items, GzChunkDev* chunks) {
  int32_t c = 0;
  for (int i = 0; i < n; ++i) {
    const vx_gz_item& g = recs[i];
    const int32_t k = (int32_t)gz_nchunks(g.n);
    items[i] = GzItemDev{(const uint8_t*)g.src, g.n, g.dst_off, {g.stride_hint[0], g.stride_hint[1], g.stride_hint[2]}, c, k, 0};
    for (int32_t j = 0; j < k; ++j) chunks[c + j] = GzChunkDev{i, j};
    c += k;
  }
}

int gz_launch_chunks(const char* who, const GzItemDev* items, const GzChunkDev* chunks, GzChunkMeta* meta, uint8_t* slots,
                     int64_t nch, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute((const void*)gz_chunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GzShared));
    if (e != hipSuccess) VX_FAIL((int)e, "%s: LDS attribute: %s", who, hipGetErrorString(e));
    attr_set = true;
  }
  hipLaunchKernelGGL(gz_chunk_kernel, dim3((unsigned)nch), dim3(GZ_LANES), sizeof(GzShared), s, items, chunks, meta, slots);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) VX_FAIL((int)e, "%s: chunks: %s", who, hipGetErrorString(e));
  return VX_OK;
}
