// The scaffold the batched stream decoders share (inflate.hip, tiff_lzw.hip; the item table also png_decode.hip's and
// tiff_unpredict's): the clamped byte source in front of a compressed stream, the persistent wave-per-item loop, and
// the launcher's half -- validating the items' windows, ordering them and putting the [counter | items] table into the
// workspace.  What a decoder does with an item (token and string batches, flushes, checksums) stays in its own file.
//
// The first part is plain C++: the host reference decoders the CPU tests build with g++ (tests/inflate_host.cpp,
// tests/lzw_host.cpp) read their input through it.  The rest is for hipcc alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "common.h"
#define VX_SI_HD __host__ __device__ __forceinline__
#else
#define VX_SI_HD inline
#endif

namespace vxsi {

// A stream's n bytes at g, read with clamped loads.  u32(pos): the 4 bytes at pos as a little-endian word, every byte at
// or beyond n read as 0 -- what the bit readers of inflate_core.h and lzw_core.h ask of a source; never reads outside
// [g, g + n).  The host reference decoders read their input through this alone.
struct Bytes {
  const uint8_t* g;
  int64_t n;
  VX_SI_HD uint32_t u32(int64_t pos) const {
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
      if (pos + k < n) v |= (uint32_t)g[pos + k] << (8 * k);
    return v;
  }
};

}  // namespace vxsi

#if defined(__HIPCC__)
#include <string.h>

#include <algorithm>
#include <vector>

namespace vxsi {

// ---------------------------------------------------------------------------------------------
// Device: the reader's byte source and the item loop.

// the LDS window of WIN bytes in front of the stream, else the stream's clamped loads
template <int WIN>
struct WinSrc {
  const uint32_t* win;
  int64_t wbase;
  Bytes all;
  __device__ uint32_t u32(int64_t pos) const {
    if (pos >= wbase && pos + 4 <= wbase + WIN) return win[(pos - wbase) >> 2];
    return all.u32(pos);
  }
  // the reader at pos has left the window, or fewer than `ahead` bytes of it lie before the reader
  __device__ bool stale(int64_t pos, int ahead) const { return pos < wbase || pos + ahead > wbase + WIN; }
};

// load the window (win: the WIN / 4 words s.win points at) at base (a multiple of 4), zeros beyond n; the whole
// workgroup of LANES lanes calls it
template <int WIN, int LANES>
static __device__ void win_load(uint32_t* win, WinSrc<WIN>& s, int64_t base) {
  __syncthreads();   // every lane is done with the old window
  s.wbase = base;
  const bool al = ((uintptr_t)(s.all.g + base) & 3) == 0;
  for (int w = threadIdx.x; w < WIN / 4; w += LANES) {
    const int64_t p = base + 4 * w;
    win[w] = al && p + 4 <= s.all.n ? *reinterpret_cast<const uint32_t*>(s.all.g + p) : s.all.u32(p);
  }
  __syncthreads();
}

// The body of a persistent wave-per-item kernel (one workgroup = one wavefront): the waves pull items from the atomic
// counter until the table is used up; body(item) is run by all lanes.
template <class Item, class Body>
static __device__ __forceinline__ void for_each_item(const Item* __restrict__ items, int n_items, int* counter, Body body) {
  for (;;) {
    int idx = 0;
    if (threadIdx.x == 0) idx = atomicAdd(counter, 1);
    idx = __shfl(idx, 0);
    if (idx >= n_items) return;
    const Item it = items[idx];
    body(it);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Host: the launchers' item tables.

// an item of a decoder that writes windows of one dst buffer
struct WinItem {
  const uint8_t* src;
  int64_t src_n;
  int64_t dst_off;
  int64_t dst_cap;
  int32_t index;   // the item's place in the caller's table (out_sizes / out_status)
  int32_t spare;   // the decoder's own word (inflate: the format)
};

// The caller's items (src, src_n, dst_off, dst_cap) as the table of a launch: every window inside [0, dst_n) and
// shorter than 4 GiB, no two overlapping, the largest streams first (a batch with one large stream does not end with
// one wave working).  own(i, item, &spare) is the launcher's own check of item i, run before the shared ones; a
// refusal names the item by the caller's index.
template <class Item, class Own>
static inline int win_items(const char* who, const Item* items, int n_items, int64_t dst_n, std::vector<WinItem>& di, Own own) {
  di.resize(n_items);
  for (int i = 0; i < n_items; ++i) {
    const Item& g = items[i];
    int32_t spare = 0;
    if (int rc = own(i, g, &spare)) return rc;
    if (g.src_n < 0 || g.dst_off < 0 || g.dst_cap < 0 || g.dst_cap > (int64_t)0xFFFFFFFF)
      VX_FAIL(VX_E_SHAPE, "%s: item %d: src_n=%lld dst_off=%lld dst_cap=%lld", who, i, (long long)g.src_n, (long long)g.dst_off,
              (long long)g.dst_cap);
    if (g.src_n > 0 && !g.src) VX_FAIL(VX_E_NULL, "%s: item %d: null source", who, i);
    if (g.dst_off > dst_n || g.dst_cap > dst_n - g.dst_off)   // (dst_off + dst_cap may not be formed: it can overflow)
      VX_FAIL(VX_E_SHAPE, "%s: item %d: window [%lld, +%lld) beyond dst_n=%lld", who, i, (long long)g.dst_off, (long long)g.dst_cap,
              (long long)dst_n);
    di[i] = WinItem{g.src, g.src_n, g.dst_off, g.dst_cap, i, spare};
  }
  // the windows may not overlap
  std::vector<int> byoff(n_items);
  for (int i = 0; i < n_items; ++i) byoff[i] = i;
  std::sort(byoff.begin(), byoff.end(), [&](int a, int b) { return di[a].dst_off < di[b].dst_off; });
  int64_t end = 0;
  for (int k = 0; k < n_items; ++k) {
    const WinItem& d = di[byoff[k]];
    if (d.dst_cap == 0) continue;
    if (d.dst_off < end) VX_FAIL(VX_E_SHAPE, "%s: item %d: window overlaps another", who, d.index);
    end = d.dst_off + d.dst_cap;
  }
  std::stable_sort(di.begin(), di.end(), [](const WinItem& a, const WinItem& b) { return a.src_n > b.src_n; });
  return VX_OK;
}

// bytes of the [counter | items] table of n_items items of item_bytes each (the *_workspace_bytes of its launcher)
static inline int64_t item_table_bytes(size_t item_bytes, int n_items) {
  if (n_items < 0) return -1;
  return 256 + (int64_t)vx_align256(item_bytes * (size_t)(n_items > 0 ? n_items : 1));
}
static inline int* item_counter(void* workspace) { return (int*)workspace; }
template <class Item>
static inline const Item* item_table(void* workspace) {
  return (const Item*)((uint8_t*)workspace + 256);
}

// the table [counter = 0 | di] into the workspace; *grid: one workgroup per unit of work, at most per_cu on every CU
template <class Item>
static inline int item_table_upload(const char* who, void* workspace, const std::vector<Item>& di, hipStream_t s, int64_t work,
                                    int per_cu, int* grid) {
  std::vector<uint8_t> table(256 + sizeof(Item) * di.size(), 0);
  memcpy(table.data() + 256, di.data(), sizeof(Item) * di.size());
  if (int rc = vx_upload_table(who, "table upload", workspace, table.data(), table.size(), s)) return rc;
  *grid = (int)std::min<int64_t>(work, (int64_t)vx_cu_count() * per_cu);
  return VX_OK;
}

}  // namespace vxsi
#endif  // __HIPCC__
