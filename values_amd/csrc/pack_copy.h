// What the pack steps of the device writers share (gzip.hip, png.hip, tiff_lzw_enc.hip): every encoder leaves its
// fragments (DEFLATE chunks, LZW strips) in windows of a workspace, one workgroup scans their sizes into places, and
// workgroups copy each fragment to its place.  The framing each format puts around the places stays in its own file.
//
// Every store in this file is a plain C++ store of a vector register.
#pragma once
#include "common.h"

namespace vxpc {

// The workgroup of LANES lanes copies n bytes from s to d, both of any alignment: the bytes up to d's first whole word,
// whole-word stores, the bytes after the last whole word.  A stored word is cut from the one or two aligned source words
// that hold its bytes.  Nothing is written outside [d, d + n); of the source only aligned words that hold at least one
// of the n bytes are read, so no read goes beyond n rounded up to a word of a word-aligned window.
template <int LANES>
__device__ __forceinline__ void copy_bytes(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, int64_t n) {
  const int t = threadIdx.x;
  int64_t head = (4 - (int64_t)((uintptr_t)d & 3)) & 3;
  if (head > n) head = n;
  if (t < head) d[t] = s[t];
  const int64_t nw = (n - head) >> 2;
  const uint32_t sh = 8 * (uint32_t)((uintptr_t)(s + head) & 3);   // where the first word's bytes begin in their aligned word
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(s + head - (sh >> 3));
  uint32_t* dw = reinterpret_cast<uint32_t*>(d + head);
#pragma unroll 4
  for (int64_t k = t; k < nw; k += LANES) dw[k] = sh ? __builtin_amdgcn_alignbit(sw[k + 1], sw[k], sh) : sw[k];
  const int64_t k = head + 4 * nw + t;
  if (k < n) d[k] = s[k];
}

// Exclusive scan of value(0) ... value(n - 1) by one workgroup of LANES lanes (a power of two): every lane sums its own
// range of the indices, a Hillis-Steele scan runs over the lanes' sums, and the lane walks its range again calling
// emit(i, the sum of the values before i); -> the sum of all values, in every lane.
template <int LANES, class Value, class Emit>
__device__ __forceinline__ int64_t exclusive_scan(int64_t n, Value value, Emit emit) {
  __shared__ int64_t part[LANES];
  const int t = threadIdx.x;
  const int64_t per = (n + LANES - 1) / LANES;
  const int64_t lo = per * t < n ? per * t : n, hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += value(i);
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < LANES; d <<= 1) {
    const int64_t o = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += o;
    __syncthreads();
  }
  int64_t run = part[t] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    emit(i, run);
    run += value(i);
  }
  return part[LANES - 1];
}

}  // namespace vxpc
