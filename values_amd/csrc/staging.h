// Descriptor upload without a wait on the stream, for the batched entry points that build a small table on the host
// (vx_aggregate_batched, vx_ncc_batched, vx_platt_sums_batched, vx_calib_bins_batched, vx_count_nonzero_batched,
// vx_select_segments): the table goes through one pinned
// staging buffer, and a call waits only for the event behind the PREVIOUS call's upload (long complete unless calls are
// issued back to back).  Not capturable into a hipGraph.
#pragma once
#include <string.h>

#include <mutex>

#include "common.h"

struct vx_staging {
  std::mutex mu;
  void* host = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  int dev = -1;
  bool pending = false;
};

// one piece of a table: `bytes` from `src` at `offset` of the uploaded block
struct vx_stage_part {
  const void* src;
  size_t bytes, offset;
};

// copies the parts into the staging buffer and uploads its first `bytes` bytes to `dst` on stream s
static inline int vx_staged_upload(vx_staging& st, const char* who, const vx_stage_part* parts, int n_parts, size_t bytes, void* dst,
                                   hipStream_t s) {
  std::lock_guard<std::mutex> lock(st.mu);
  hipError_t e = hipSuccess;
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess) VX_FAIL((int)e, "%s: hipGetDevice: %s", who, hipGetErrorString(e));
  if (st.pending && (e = hipEventSynchronize(st.ev)) != hipSuccess)
    VX_FAIL((int)e, "%s: descriptor upload: %s", who, hipGetErrorString(e));
  st.pending = false;
  if (st.ev && st.dev != dev) { (void)hipEventDestroy(st.ev); st.ev = nullptr; }
  if (!st.ev) {
    if ((e = hipEventCreateWithFlags(&st.ev, hipEventDisableTiming)) != hipSuccess)
      VX_FAIL((int)e, "%s: hipEventCreate: %s", who, hipGetErrorString(e));
    st.dev = dev;
  }
  if (bytes > st.cap) {
    if (st.host) (void)hipHostFree(st.host);
    st.host = nullptr; st.cap = 0;
    const size_t cap = bytes < (64 << 10) ? (64 << 10) : bytes * 2;
    if ((e = hipHostMalloc(&st.host, cap, hipHostMallocDefault)) != hipSuccess)
      VX_FAIL((int)e, "%s: %zu bytes of pinned staging: %s", who, cap, hipGetErrorString(e));
    st.cap = cap;
  }
  for (int i = 0; i < n_parts; ++i) memcpy((char*)st.host + parts[i].offset, parts[i].src, parts[i].bytes);
  if ((e = hipMemcpyAsync(dst, st.host, bytes, hipMemcpyHostToDevice, s)) != hipSuccess ||
      (e = hipEventRecord(st.ev, s)) != hipSuccess)
    VX_FAIL((int)e, "%s: descriptor upload: %s", who, hipGetErrorString(e));
  st.pending = true;
  return VX_OK;
}
