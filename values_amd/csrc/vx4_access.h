// Four consecutive elements per lane: the access helpers of the batched 3D streaming passes (patches3d.hip,
// train_patches3d.hip).  One access of up to 16 bytes where the four elements lie inside the row and the address is
// aligned to the access, element by element elsewhere.
#pragma once
#include "common.h"

template <typename S>
struct alignas((sizeof(S) * 4 < 16) ? sizeof(S) * 4 : 16) vx4_pack { S v[4]; };

// n (1..4) elements from p into v; one access of min(16, 4 * sizeof(S)) bytes (two for 8-byte elements) when n == 4 and p
// is aligned to it, else n element loads
template <typename S>
__device__ __forceinline__ void vx4_load(const S* p, int n, S v[4]) {
  typedef vx4_pack<S> pack;
  if (n == 4 && ((uintptr_t)p & (alignof(pack) - 1)) == 0) {
    const pack q = *reinterpret_cast<const pack*>(p);
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = q.v[u];
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = u < n ? p[u] : S(0);
  }
}

template <typename S>
__device__ __forceinline__ void vx4_store(S* p, int n, const S v[4]) {
  typedef vx4_pack<S> pack;
  if (n == 4 && ((uintptr_t)p & (alignof(pack) - 1)) == 0) {
    pack q;
#pragma unroll
    for (int u = 0; u < 4; ++u) q.v[u] = v[u];
    *reinterpret_cast<pack*>(p) = q;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < n) p[u] = v[u];
  }
}

template <typename S>
__device__ __forceinline__ void vx4_load_as_double(const void* base, int64_t e, int n, double d[4]) {
  S v[4];
  vx4_load<S>(reinterpret_cast<const S*>(base) + e, n, v);
#pragma unroll
  for (int u = 0; u < 4; ++u) d[u] = (double)v[u];
}

// elements [e, e + n) of an array of kind VX_PREP_* as doubles: every kind's values are exact in a double
__device__ __forceinline__ void vx4_load_kind(const void* base, int kind, int64_t e, int n, double d[4]) {
  switch (kind) {
    case VX_PREP_U8: vx4_load_as_double<uint8_t>(base, e, n, d); break;
    case VX_PREP_I8: vx4_load_as_double<int8_t>(base, e, n, d); break;
    case VX_PREP_U16: vx4_load_as_double<uint16_t>(base, e, n, d); break;
    case VX_PREP_I16: vx4_load_as_double<int16_t>(base, e, n, d); break;
    case VX_PREP_U32: vx4_load_as_double<uint32_t>(base, e, n, d); break;
    case VX_PREP_I32: vx4_load_as_double<int32_t>(base, e, n, d); break;
    case VX_PREP_F32: vx4_load_as_double<float>(base, e, n, d); break;
    default: vx4_load_as_double<double>(base, e, n, d); break;
  }
}

// labels [e, e + n) of 1 << esl bytes each, signed when sgn, as (the value numpy's astype(intc) gives: the low 32 bits of
// the sign- or zero-extended element; anything outside 0..255)
template <typename S>
__device__ __forceinline__ void vx4_load_label_t(const void* base, int64_t e, int n, int32_t lab[4], bool bad[4]) {
  S v[4];
  vx4_load<S>(reinterpret_cast<const S*>(base) + e, n, v);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const unsigned long long w = (unsigned long long)(long long)v[u];   // a negative value extends to one above 255
    lab[u] = (int32_t)(uint32_t)w;
    bad[u] = u < n && w > 255ull;
  }
}

__device__ __forceinline__ void vx4_load_label(const void* base, int esl, int sgn, int64_t e, int n, int32_t lab[4], bool bad[4]) {
  switch (esl | (sgn << 2)) {
    case 0: vx4_load_label_t<uint8_t>(base, e, n, lab, bad); break;
    case 1: vx4_load_label_t<uint16_t>(base, e, n, lab, bad); break;
    case 2: vx4_load_label_t<uint32_t>(base, e, n, lab, bad); break;
    case 3: vx4_load_label_t<unsigned long long>(base, e, n, lab, bad); break;
    case 4: vx4_load_label_t<int8_t>(base, e, n, lab, bad); break;
    case 5: vx4_load_label_t<int16_t>(base, e, n, lab, bad); break;
    case 6: vx4_load_label_t<int32_t>(base, e, n, lab, bad); break;
    default: vx4_load_label_t<long long>(base, e, n, lab, bad); break;
  }
}
