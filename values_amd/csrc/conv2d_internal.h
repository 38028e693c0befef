// Internal interface of the 2D convolution files: conv2d.hip (entry points: route, then launch) and one file per kernel family
// (kernel, pack kernel, launch_X<...>, vx_conv2d_X_launch).  The routing itself is conv2d_route.h.
#pragma once
#include "common.h"
#include "conv2d_route.h"

// ---- launchers: copy the descriptor into the kernel's argument struct, switch on the instance --------------------------------
int vx_conv2d_mfma_launch(const Conv2dRoute& r, const vx_conv2d_args& a, hipStream_t s);   // conv2d_mfma.hip: native fp32
int vx_conv2d_s16_launch(const Conv2dRoute& r, const vx_conv2d_args& a, hipStream_t s);    // conv2d_s16.hip: split-fp16

// ---- weight packing, one per schedule (sizes: conv2d_route.h) ----------------------------------------------------------------
int vx_pack_conv2d_mfma(const float* w_torch, float* w_packed, int Cin, int Cout, int KS, int64_t total, hipStream_t s);
int vx_pack_conv2d_s16(const float* w_torch, float* w_packed, int Cin, int Cout, int KS, const C2SPack& k, hipStream_t s);

// the instance's name, formatted once per launch_X<...> instantiation (a function-local static there) and kept for the process
static inline const char* vx_conv2d_kname(const Conv2dRoute& r) {
  char buf[128];
  conv2d_route_name(r, buf, (int)sizeof(buf));
  return vx_kname("%s", buf);
}
