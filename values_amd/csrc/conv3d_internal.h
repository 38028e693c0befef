// Internal interface of the 3x3x3 convolution files: conv3d_k3.hip (entry points: route, then launch), one file per kernel family
// (kernel, pack kernel, launch_X<...>, vx_conv3d_X_launch) and unet3d_forward.hip.  The routing itself is conv3d_route.h.
#pragma once
#include <stdlib.h>

#include "common.h"
#include "conv3d_route.h"

// ---- launchers: copy the descriptor into the kernel's argument struct, switch on the instance --------------------------------
int vx_conv3d_mfma_launch(const Conv3dRoute& r, const vx_conv3d_args& a, hipStream_t s);   // conv3d_mfma.hip: native fp32 tile kernel
int vx_conv3d_c8_launch(const Conv3dRoute& r, const vx_conv3d_args& a, hipStream_t s);     // conv3d_c8.hip: fp32 4x4x1, Cout = 8
int vx_conv3d_s16_launch(const Conv3dRoute& r, const vx_conv3d_args& a, hipStream_t s);    // conv3d_s16.hip: split-fp16 tile kernel
int vx_conv3d_xp8w_launch(const Conv3dRoute& r, const vx_conv3d_args& a, hipStream_t s);   // conv3d_xp8w.hip: full-resolution z-column kernel
int vx_conv3d_zc16_launch(const Conv3dRoute& r, const vx_conv3d_args& a, const float* w_block, hipStream_t s);   // conv3d_zc16.hip
int vx_conv3d_deep_launch(const Conv3dRoute& r, const vx_conv3d_args& a, const float* w_block, hipStream_t s);   // conv3d_deep.hip

// ---- weight packing, one per packed block (sizes: conv3d_route.h) ------------------------------------------------------------
int vx_pack_conv3d_k3_mfma(const float* w_torch, float* w_packed, int Cin, int Cout, int64_t total, hipStream_t s);
int vx_pack_conv3d_k3_c8(const float* w_torch, float* w_packed, int Cin, hipStream_t s);
int vx_pack_conv3d_k3_s16(const float* w_torch, float* w_packed, int Cin, int Cout, hipStream_t s);
int vx_pack_conv3d_zc16(const float* w_torch, float* w_packed, int Cin, int Cout, hipStream_t s);
int vx_pack_conv3d_deep(const float* w_torch, float* w_packed, int Cin, int Cout, hipStream_t s);

// conv3d_c1.hip
extern "C" int vx_conv3d_k3_c1_tiles(int D, int H, int W);

// the instance's name, formatted once per launch_X<...> instantiation (a function-local static there) and kept for the process
static inline const char* vx_conv3d_kname(const Conv3dRoute& r) {
  char buf[128];
  conv3d_route_name(r, buf, (int)sizeof(buf));
  return vx_kname("%s", buf);
}

// Phase stamps of the kernels' item loops (diagnostic build -DVX_CONV_STAMPS, tools/build_stamps.sh): s_memtime deltas summed per wave
// into st_sum[phase]; the values go to a buffer of their own, never into an output.  VX_DIAG(x): a phase-ablation word of the
// argument struct (wrong results by design) -- the product library compiles it to 0.
#ifdef VX_CONV_STAMPS
#define VX_STAMP(i)                                                                      \
  do {                                                                                   \
    unsigned long long t_;                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");           \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    st_sum[i] += t_ - st_last;                                                           \
    st_last = t_;                                                                        \
  } while (0)
#define VX_STAMP_WAIT_LOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define VX_DIAG(x) (x)
#else
#define VX_STAMP(i) do {} while (0)
#define VX_STAMP_WAIT_LOADS() do {} while (0)
#define VX_DIAG(x) 0
#endif

// Diagnostic build only (-DVX_CONV_STAMPS, tools/build_stamps.sh): the phase-stamp buffer and the family's phase-ablation word come
// from the environment; the product library does not contain the variable names (tests/test_abi.py).
enum { VX_DIAG_NONE = 0, VX_DIAG_XP_ABL, VX_DIAG_S16_DBG, VX_DIAG_C8_DBG };
static inline void vx_conv_diag(int which, unsigned long long** stamps, int* dbg) {
  *stamps = nullptr;
  *dbg = 0;
#ifdef VX_CONV_STAMPS
  static const char* const env[] = {nullptr, "VX_XP_ABL", "VX_S16_DBG", "VX_C8_DBG"};
  if (const char* e = getenv("VX_CONV_DBG_PTR")) *stamps = (unsigned long long*)strtoull(e, nullptr, 0);
  if (env[which])
    if (const char* e = getenv(env[which])) *dbg = atoi(e);
#endif
}
