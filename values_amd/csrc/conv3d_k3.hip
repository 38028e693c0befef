// vx_conv3d_k3 and its public queries: validate -> route -> launch.  Everything that decides is conv3d_route.h (a pure function
// of the arguments and the configuration); everything that runs on the device is in the family's own file.
#include <string.h>

#include "conv3d_internal.h"

extern "C" int vx_conv3d_k3_route(const vx_conv3d_args* ap, char* kernel_name, int cap) {
  if (!ap) VX_FAIL(VX_E_NULL, "vx_conv3d_k3: null args");
  Conv3dRoute r;
  const int rc = conv3d_route(*ap, vx_cfg(), &r);
  if (rc != VX_OK) VX_FAIL(rc, "%s", r.err);
  if (kernel_name && cap > 0) conv3d_route_name(r, kernel_name, cap);
  return VX_OK;
}

extern "C" int vx_conv3d_k3(const vx_conv3d_args* ap, vx_stream_t stream) {
  if (!ap) VX_FAIL(VX_E_NULL, "vx_conv3d_k3: null args");
  const vx_conv3d_args& a = *ap;
  Conv3dRoute r;
  const int rc = conv3d_route(a, vx_cfg(), &r);
  if (rc != VX_OK) VX_FAIL(rc, "%s", r.err);
  hipStream_t s = (hipStream_t)stream;
  switch (r.kernel) {
    case CONV3D_C8: return vx_conv3d_c8_launch(r, a, s);
    case CONV3D_XP8W: return vx_conv3d_xp8w_launch(r, a, s);
    case CONV3D_ZC16: return vx_conv3d_zc16_launch(r, a, a.w_packed + r.w_off, s);
    case CONV3D_DEEP: return vx_conv3d_deep_launch(r, a, a.w_packed + r.w_off, s);
    case CONV3D_S16: return vx_conv3d_s16_launch(r, a, s);
    default: return vx_conv3d_mfma_launch(r, a, s);
  }
}

// ---- weight packing -----------------------------------------------------------------------------------------------------------
extern "C" int vx_conv3d_k3_family(int Cin, int Cout) { return conv3d_family(Cin, Cout, vx_cfg()); }
extern "C" int64_t vx_conv3d_k3_packed_floats(int Cin, int Cout) { return conv3d_packed_floats(Cin, Cout, vx_cfg()); }

extern "C" int vx_pack_conv3d_k3(const float* w_torch, float* w_packed, int Cin, int Cout, vx_stream_t stream) {
  if (!w_torch || !w_packed) VX_FAIL(VX_E_NULL, "vx_pack_conv3d_k3: null pointer");
  const int64_t total = vx_conv3d_k3_packed_floats(Cin, Cout);
  if (total < 0) VX_FAIL(VX_E_SHAPE, "vx_pack_conv3d_k3: Cin=%d Cout=%d must be positive multiples of 8", Cin, Cout);
  const ConvCfg c = conv_config(Cin, Cout, vx_cfg());
  hipStream_t s = (hipStream_t)stream;
  if (c.C8) return vx_pack_conv3d_k3_c8(w_torch, w_packed, Cin, s);
  if (!c.S16) return vx_pack_conv3d_k3_mfma(w_torch, w_packed, Cin, Cout, total, s);
  const int rc = vx_pack_conv3d_k3_s16(w_torch, w_packed, Cin, Cout, s);
  if (rc != VX_OK) return rc;
  // families 6 / 7: a role-split kernel's block behind the tile kernel's (never both: the z-column kernel packs Cout = 16)
  float* w_block = w_packed + conv3d_s16_packed_floats(Cin, Cout);
  if (conv3d_deep_packs(Cin, Cout)) return vx_pack_conv3d_deep(w_torch, w_block, Cin, Cout, s);
  return vx_pack_conv3d_zc16(w_torch, w_block, Cin, Cout, s);   // (nothing where it does not pack)
}

// ---- queries: the rules of conv3d_route.h under the current configuration ----------------------------------------------------
extern "C" int vx_conv3d_k3_tiles(int D, int H, int W) { return conv3d_tiles_max(D, H, W); }
extern "C" int vx_conv3d_k3_tiles_for(int D, int H, int W, int Cout) { return conv3d_tiles_for(D, H, W, Cout, vx_cfg()); }
extern "C" int vx_conv3d_k3_head_fusable(int Cin, int Cout) { return conv3d_head_fusable(Cin, Cout, vx_cfg()); }
extern "C" int vx_conv3d_k3_prologue_ok(int D, int H, int W, int Cin, int Cout) { return conv3d_prologue_ok(D, H, W, Cin, Cout, vx_cfg()); }
extern "C" int vx_conv3d_k3_skip_prologue_ok(int D, int H, int W, int Cin, int Cout, int xblk) {
  return conv3d_skip_prologue_ok(D, H, W, Cin, Cout, xblk, vx_cfg());
}
extern "C" int vx_conv3d_k3_acc_ok(int D, int H, int W, int Cin, int Cout) { return conv3d_zc16_16to16(D, H, W, Cin, Cout, vx_cfg()) ? 1 : 0; }
extern "C" int vx_conv3d_k3_planar_ok(int D, int H, int W, int Cin, int Cout) { return conv3d_zc16_16to16(D, H, W, Cin, Cout, vx_cfg()) ? 1 : 0; }
extern "C" int vx_conv3d_k3_upfuse_ok(int D, int H, int W, int Cin, int Cout) { return conv3d_upfuse_ok(D, H, W, Cin, Cout, vx_cfg()); }
extern "C" int vx_conv3d_k3_pool_layout(int D, int H, int W, int Cin, int Cout) { return conv3d_pool_layout(D, H, W, Cin, Cout, vx_cfg()); }
extern "C" int vx_conv3d_k3_poolfuse_ok(int D, int H, int W, int Cin, int Cout) { return conv3d_pool_layout(D, H, W, Cin, Cout, vx_cfg()) != 0 ? 1 : 0; }
extern "C" int vx_conv3d_k3_presplit_ok(int D, int H, int W, int Cin, int Cout) { return conv3d_presplit_ok(D, H, W, Cin, Cout, vx_cfg()); }
extern "C" int vx_conv3d_k3_poolfin_ok(int Cin, int Cout) { return conv3d_poolfin_ok(Cin, Cout, vx_cfg()); }
