// The bilinear source coordinate of the 2D upsample kernels (bn2d.hip) and of the 2D SSN validation reduction
// (valstep.hip): one definition, so a pixel interpolated by either carries the same bits.
#pragma once
#include "common.h"

// bilinear source coordinates of F.interpolate(align_corners=False): src = (dst + 0.5) * in/out - 0.5, clamped at 0
__device__ __forceinline__ void bil_coord(int d, int in, float ratio, int& i0, int& i1, float& l1) {
  float s = ((float)d + 0.5f) * ratio - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}
