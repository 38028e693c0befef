// vx_conv2d and its public queries: validate -> route -> launch.  Everything that decides is conv2d_route.h (a pure function of
// the arguments and the configuration); everything that runs on the device is in the family's own file.
#include "conv2d_internal.h"

static int route_or_fail(const vx_conv2d_args* ap, Conv2dRoute* r) {
  if (!ap) VX_FAIL(VX_E_NULL, "vx_conv2d: null args");
  const int rc = conv2d_route(*ap, vx_cfg(), r);
  if (rc != VX_OK) VX_FAIL(rc, "%s", r->err);
  return VX_OK;
}

extern "C" int vx_conv2d_route(const vx_conv2d_args* ap, char* kernel_name, int cap, vx_conv2d_route_info* info) {
  Conv2dRoute r;
  const int rc = route_or_fail(ap, &r);
  if (rc != VX_OK) return rc;
  if (kernel_name && cap > 0) conv2d_route_name(r, kernel_name, cap);
  if (info) *info = {r.nchunks, r.w_all, r.lds_bytes, r.grid_x, r.grid_y};
  return VX_OK;
}

extern "C" int vx_conv2d(const vx_conv2d_args* ap, vx_stream_t stream) {
  Conv2dRoute r;
  const int rc = route_or_fail(ap, &r);
  if (rc != VX_OK) return rc;
  if (r.kernel == CONV2D_S16) return vx_conv2d_s16_launch(r, *ap, (hipStream_t)stream);
  return vx_conv2d_mfma_launch(r, *ap, (hipStream_t)stream);
}

// ---- weight packing and queries: the rules of conv2d_route.h under the current configuration ---------------------------------
extern "C" int vx_conv2d_family(int Cin, int Cout, int KS) { return conv2d_family(Cin, Cout, KS, vx_cfg()); }
extern "C" int64_t vx_conv2d_packed_floats(int Cin, int Cout, int KS) { return conv2d_packed_floats(Cin, Cout, KS, vx_cfg()); }
extern "C" int vx_conv2d_tiles(int H, int W, int KS, int S) { return conv2d_tiles(H, W, KS, S); }

extern "C" int vx_pack_conv2d(const float* w_torch, float* w_packed, int Cin, int Cout, int KS, vx_stream_t stream) {
  if (!w_torch || !w_packed) VX_FAIL(VX_E_NULL, "vx_pack_conv2d: null pointer");
  const int64_t total = vx_conv2d_packed_floats(Cin, Cout, KS);
  if (total < 0) VX_FAIL(VX_E_SHAPE, "vx_pack_conv2d: Cin=%d Cout=%d KS=%d", Cin, Cout, KS);
  if (!conv2d_split16(vx_cfg())) return vx_pack_conv2d_mfma(w_torch, w_packed, Cin, Cout, KS, total, (hipStream_t)stream);
  return vx_pack_conv2d_s16(w_torch, w_packed, Cin, Cout, KS, conv2d_s16_pack(Cin, Cout, KS, vx_cfg()), (hipStream_t)stream);
}
