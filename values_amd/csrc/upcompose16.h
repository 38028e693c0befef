// upscale3 composed into expand_2_1's up half (conv3d_zc16.hip, composed bodies; vx_pack_conv3d_upfused_zc16): the algebra, in
// float64 from the torch-layout tensors, as ONE host / device function per table so that the pack kernel and the host test
// (tests/upcompose16_host.cpp) evaluate the same expressions.
//
// conv3d(k = 3, padding = 1) over ConvTranspose3d(32 -> 16, k = 2, s = 2)(coarse) + up_b, for the output voxel
// (z, y, x) = (2 Z + pz, 2 Y + py, 2 X + px):
//   out[co] = btab[class(z), class(y), class(x)][co]
//           + sum_{a, b, c in {0, 1}} sum_{ci < 32} Weff[pz, py, px][a, b, c][ci][co] coarse[Z + pz - 1 + a, Y + py - 1 + b, X + px - 1 + c][ci]
// per axis, tap k in {0, 1, 2} of parity p: t = p + k - 1, coarse offset o = floor(t / 2), sub-position d = t mod 2, a = o - (p - 1).
// A coarse voxel outside the coarse volume reads as zero: a fine tap outside the fine volume maps only to such a voxel, which is
// the conv's zero padding; the up bias of the taps INSIDE the volume is what the border table carries (classes per axis: 0 first,
// 1 interior, 2 last voxel).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VX_UPC16_FN __host__ __device__ inline
#else
#define VX_UPC16_FN inline
#endif

// tap k of parity p along one axis -> index a in {0, 1} of the coarse tap, sub-position d in {0, 1} of the transposed conv
VX_UPC16_FN void vx_upc16_tap(int p, int k, int* a, int* d) {
  const int t = p + k - 1;                  // fine offset from 2 Q: -1 .. 2
  const int o = t < 0 ? -1 : t >> 1;        // floor(t / 2)
  *d = t - 2 * o;
  *a = o - (p - 1);
}

// Weff[class cls = pz 4 + py 2 + px][tap = a 4 + b 2 + c][ci][co].  w1: the conv's torch weight [16][w1_cin][3][3][3] (the up half
// is its input channels 0..15), uw: the transposed conv's torch weight [32][16][2][2][2].
VX_UPC16_FN double vx_upc16_weff(const float* w1, int w1_cin, const float* uw, int cls, int tap, int ci, int co) {
  const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
  const int ta = tap >> 2, tb = (tap >> 1) & 1, tc = tap & 1;
  double acc = 0.0;
  for (int kz = 0; kz < 3; ++kz) {
    int a, dz; vx_upc16_tap(pz, kz, &a, &dz);
    if (a != ta) continue;
    for (int ky = 0; ky < 3; ++ky) {
      int b, dy; vx_upc16_tap(py, ky, &b, &dy);
      if (b != tb) continue;
      for (int kx = 0; kx < 3; ++kx) {
        int c, dx; vx_upc16_tap(px, kx, &c, &dx);
        if (c != tc) continue;
        for (int cu = 0; cu < 16; ++cu)
          acc += (double)w1[(co * w1_cin + cu) * 27 + kz * 9 + ky * 3 + kx] * (double)uw[(ci * 16 + cu) * 8 + dz * 4 + dy * 2 + dx];
      }
    }
  }
  return acc;
}

// btab[cz][cy][cx][co]: the up bias through the conv's taps that lie inside the volume for that border class
VX_UPC16_FN double vx_upc16_btab(const float* w1, int w1_cin, const float* ub, int cz, int cy, int cx, int co) {
  double acc = 0.0;
  for (int kz = 0; kz < 3; ++kz) {
    if ((cz == 0 && kz == 0) || (cz == 2 && kz == 2)) continue;
    for (int ky = 0; ky < 3; ++ky) {
      if ((cy == 0 && ky == 0) || (cy == 2 && ky == 2)) continue;
      for (int kx = 0; kx < 3; ++kx) {
        if ((cx == 0 && kx == 0) || (cx == 2 && kx == 2)) continue;
        for (int cu = 0; cu < 16; ++cu) acc += (double)w1[(co * w1_cin + cu) * 27 + kz * 9 + ky * 3 + kx] * (double)ub[cu];
      }
    }
  }
  return acc;
}

// the packed block: [class 8][tap 8][hi | lo][lane 64][8 halves] (lane (m, g): row m = co, k = ci 8 g .. 8 g + 7), then btab[27][16] fp32
#define VX_UPC16_WHALVES (8 * 8 * 2 * 64 * 8)
#define VX_UPC16_FLOATS (VX_UPC16_WHALVES / 2 + 27 * 16)
