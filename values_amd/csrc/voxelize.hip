// K44: triangle meshes to a label volume (values_amd/stl.py states the rule).  A voxel is inside a mesh when
// the column below its sample point crosses the mesh an odd number of times.
//   One workgroup owns a row of VOX_TILE_X columns, lanes along x, all its waves on the same row.  Per mesh it walks the
//   triangle list in steps of VOX_CHUNK: every thread takes one triangle (loaded one step ahead) and, when its xy box overlaps the tile's sample range and its
//   projected area is not 0, appends its setup to a list in LDS -- the ordered endpoint and the difference vector of each
//   edge, the sign m of each edge, the three z, the box.  Then the waves share the list, every fourth entry each, and a
//   thread tests its column against its wave's entries.  A hit toggles ONE bit of the column's mask (LDS, 64-bit words,
//   LDS atomics since four waves toggle one column): the first k whose sample lies above the hit.  After the last triangle
//   a prefix XOR along k turns the toggles into inside bits, and the waves write the row, 16 k of every 64 each, one k at a
//   time across the lanes, so every store of a wave is one contiguous row segment.  Later meshes store only their inside
//   voxels, in the same thread as the earlier ones: program order gives the overwrite order.
//   Columns with an odd number of hits are counted by ballot and popcount in wave 0 and leave with one integer atomic per
//   workgroup; a one-thread kernel zeroes the counter first.
// All arithmetic is float64 with plain * - + /, one rounding each: the file is compiled with -ffp-contract=off (Makefile)
// and says so again below.  Plain C++ stores and integer atomics only.  Nothing is uploaded: the grid and the mesh offsets
// travel as kernel arguments.
#include "common.h"
#include "voxel_plan.h"

#pragma clang fp contract(off)

struct vox_args {
  double ox, oy, oz, h;
  int32_t nz, ny, nx, n_meshes;
  long long off[VOX_MAX_MESHES + 1];
};

// the setups of one step, one array per field: every lane reads the same entry at the same time (an LDS broadcast)
struct vox_list {
  double dx[3][VOX_CHUNK], dy[3][VOX_CHUNK];   // q - p of the ordered edge
  float px[3][VOX_CHUNK], py[3][VOX_CHUNK];    // p: a vertex, so float32 holds it exactly
  float m[3][VOX_CHUNK];                       // orient * (swapped ? -1 : +1)
  float z[3][VOX_CHUNK];
  float x0[VOX_CHUNK], x1[VOX_CHUNK], y0[VOX_CHUNK], y1[VOX_CHUNK];
};

__device__ __forceinline__ double vox_sample(double origin, int t, double h) {
  const double u = (double)t + 0.5;
  const double s = u * h;
  return origin + s;
}

// the edge (a, b) on its lexicographically ordered endpoints (x, then y)
__device__ __forceinline__ bool vox_swapped(double ax, double ay, double bx, double by) { return !(ax < bx || (ax == bx && ay < by)); }

__device__ __forceinline__ double vox_edge(double dx, double dy, double px, double py, double sx, double sy) {
  const double ry = sy - py, rx = sx - px;
  const double a = dx * ry, b = dy * rx;
  return a - b;
}

__global__ __launch_bounds__(VOX_THREADS) void voxelize_kernel(const float* __restrict__ tris, vox_args g, float* __restrict__ out,
                                                               unsigned long long* __restrict__ odd_columns) {
  __shared__ unsigned long long mask[VOX_MAX_WORDS * VOX_TILE_X];   // [word][column]: the waves toggle it with LDS atomics
  __shared__ unsigned int hits[VOX_TILE_X];                         // bit 0: the parity of a column's hits
  __shared__ vox_list L;
  __shared__ int n_list[2];
  const int tid = threadIdx.x, lane = tid & (VOX_TILE_X - 1), wave = tid / VOX_TILE_X;
  const int i = blockIdx.x * VOX_TILE_X + lane, j = blockIdx.y;
  const bool valid = i < g.nx;
  const double cx = vox_sample(g.ox, i, g.h), cy = vox_sample(g.oy, j, g.h);
  // the tile's sample range: the samples are monotone in the index, so every column of the row lies inside it
  const int i_lo = blockIdx.x * VOX_TILE_X;
  const int i_hi = i_lo + VOX_TILE_X - 1 < g.nx ? i_lo + VOX_TILE_X - 1 : g.nx - 1;
  const double tx0 = vox_sample(g.ox, i_lo, g.h), tx1 = vox_sample(g.ox, i_hi, g.h);
  const double ty0 = vox_sample(g.oy, j, g.h), ty1 = ty0;
  const int words = (g.nz + 63) >> 6;
  const double inv_h = 1.0 / g.h;
  if (tid == 0) { n_list[0] = 0; n_list[1] = 0; }
  __syncthreads();
  int step = 0;
  unsigned odd_total = 0;   // wave 0 counts
  for (int mesh = 0; mesh < g.n_meshes; ++mesh) {
    // (the barriers of the first step lie between these stores and the first toggle)
    for (int q = tid; q < words * VOX_TILE_X; q += VOX_THREADS) mask[q] = 0;
    if (tid < VOX_TILE_X) hits[tid] = 0;
    const long long end = g.off[mesh + 1];
    float nv[9];   // the thread's triangle of the NEXT step: its loads are in flight while this step's list is tested
#pragma unroll
    for (int q = 0; q < 9; ++q) nv[q] = g.off[mesh] + tid < end ? tris[(g.off[mesh] + tid) * 9 + q] : 0.0f;
    for (long long base = g.off[mesh]; base < end; base += VOX_CHUNK, ++step) {
      int* count = &n_list[step & 1];
      __syncthreads();   // the step before has read its list
      const long long t = base + tid;
      float v[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) v[q] = nv[q];
      if (t + VOX_CHUNK < end) {
#pragma unroll
        for (int q = 0; q < 9; ++q) nv[q] = tris[(t + VOX_CHUNK) * 9 + q];
      }
      if (t < end) {
        const float fx[3] = {v[0], v[3], v[6]}, fy[3] = {v[1], v[4], v[7]}, fz[3] = {v[2], v[5], v[8]};
        const float bx0 = fminf(fx[0], fminf(fx[1], fx[2])), bx1 = fmaxf(fx[0], fmaxf(fx[1], fx[2]));
        const float by0 = fminf(fy[0], fminf(fy[1], fy[2])), by1 = fmaxf(fy[0], fmaxf(fy[1], fy[2]));
        if ((double)bx0 <= tx1 && (double)bx1 >= tx0 && (double)by0 <= ty1 && (double)by1 >= ty0) {
          const double x[3] = {(double)fx[0], (double)fx[1], (double)fx[2]}, y[3] = {(double)fy[0], (double)fy[1], (double)fy[2]};
          // area = E(v0, v1; v2) on the ordered endpoints
          const bool sw = vox_swapped(x[0], y[0], x[1], y[1]);
          const double xp = sw ? x[1] : x[0], yp = sw ? y[1] : y[0], xq = sw ? x[0] : x[1], yq = sw ? y[0] : y[1];
          const double ec = vox_edge(xq - xp, yq - yp, xp, yp, x[2], y[2]);
          const double area = sw ? -ec : ec;
          if (area != 0.0) {   // false for NaN as well: a non-finite triangle hits nothing
            const float orient = area > 0.0 ? 1.0f : -1.0f;
            const int e = atomicAdd(count, 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {   // the edges (v1, v2), (v2, v0), (v0, v1): edge k is opposite vertex k
              const int a = (k + 1) % 3, b = (k + 2) % 3;
              const bool s = vox_swapped(x[a], y[a], x[b], y[b]);
              const int pp = s ? b : a, qq = s ? a : b;
              L.px[k][e] = (pp == 0 ? fx[0] : pp == 1 ? fx[1] : fx[2]);
              L.py[k][e] = (pp == 0 ? fy[0] : pp == 1 ? fy[1] : fy[2]);
              const double qx = qq == 0 ? x[0] : qq == 1 ? x[1] : x[2], qy = qq == 0 ? y[0] : qq == 1 ? y[1] : y[2];
              L.dx[k][e] = qx - (double)L.px[k][e];
              L.dy[k][e] = qy - (double)L.py[k][e];
              L.m[k][e] = s ? -orient : orient;
              L.z[k][e] = fz[k];
            }
            L.x0[e] = bx0; L.x1[e] = bx1; L.y0[e] = by0; L.y1[e] = by1;
          }
        }
      }
      __syncthreads();
      const int n = *count;
      if (tid == 0) n_list[(step + 1) & 1] = 0;   // last read in the step before, next used after the next barrier
      if (valid) {
        for (int e = wave; e < n; e += VOX_WAVES) {   // the waves share the row: each takes every fourth entry
          // straight-line up to the hit, so the entry's LDS loads leave together.  A column outside the triangle's closed
          // xy box is never hit
          bool covered = cx >= (double)L.x0[e] && cx <= (double)L.x1[e] && cy >= (double)L.y0[e] && cy <= (double)L.y1[e];
          double w[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double mk = (double)L.m[k][e];
            const double ek = vox_edge(L.dx[k][e], L.dy[k][e], (double)L.px[k][e], (double)L.py[k][e], cx, cy);
            w[k] = ek * mk;
            covered = covered & (w[k] > 0.0 || (w[k] == 0.0 && mk > 0.0));
          }
          const double z0 = (double)L.z[0][e], z1 = (double)L.z[1][e], z2 = (double)L.z[2][e];
          if (!covered) continue;
          const double a0 = w[0] * z0, a1 = w[1] * z1, a2 = w[2] * z2;
          const double num = (a0 + a1) + a2, den = (w[0] + w[1]) + w[2];
          const double z_hit = num / den;
          // the first k with z_hit < c_z(k): an estimate, then exact steps on the samples themselves
          int k = g.nz;
          if (z_hit == z_hit) {
            double est = (z_hit - g.oz) * inv_h;   // only where the search starts: any value gives the same k
            if (!(est >= 0.0)) est = 0.0;
            if (est > (double)g.nz) est = (double)g.nz;
            k = (int)est;
            while (k > 0 && vox_sample(g.oz, k - 1, g.h) > z_hit) --k;
            while (k < g.nz && !(vox_sample(g.oz, k, g.h) > z_hit)) ++k;
          }
          atomicXor(&hits[lane], 1u);
          if (k < g.nz) atomicXor(&mask[(k >> 6) * VOX_TILE_X + lane], 1ull << (k & 63));
        }
      }
    }
    __syncthreads();   // every toggle of the mesh is in
    // toggles -> inside bits: the prefix XOR along k, carried from word to word (every wave works it out for its lanes); then
    // the column's stores, the 64 k of a word shared among the waves
    const float label = (float)(mesh + 1);
    unsigned long long carry = 0;
    for (int w = 0; w < words; ++w) {
      unsigned long long x = mask[w * VOX_TILE_X + lane];
      x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
      if (carry) x = ~x;
      carry = x >> 63;
      if (valid) {
        const int k_end = g.nz - w * 64 < 64 ? g.nz - w * 64 : 64;
        const int b_end = (wave + 1) * VOX_K_PER_WAVE < k_end ? (wave + 1) * VOX_K_PER_WAVE : k_end;
        for (int b = wave * VOX_K_PER_WAVE; b < b_end; ++b) {
          const bool in = (x >> b) & 1ull;
          const long long idx = ((long long)(w * 64 + b) * g.ny + j) * g.nx + i;
          if (mesh == 0) out[idx] = in ? 1.0f : 0.0f;
          else if (in) out[idx] = label;   // the same thread as for the meshes before: program order is the overwrite order
        }
      }
    }
    if (wave == 0) odd_total += (unsigned)__popcll(__ballot(valid && (hits[lane] & 1u)));
    __syncthreads();   // mask and hits have been read: the next mesh may zero them
  }
  if (tid == 0 && odd_total) atomicAdd(odd_columns, (unsigned long long)odd_total);
}

__global__ void voxelize_zero_kernel(unsigned long long* __restrict__ odd_columns) { *odd_columns = 0; }

extern "C" int vx_voxelize_meshes(const float* tris, const int64_t* mesh_offsets, int n_meshes, const double* origin, double h,
                                  const int32_t* dims, float* out, int64_t* odd_columns, vx_stream_t stream) {
  const char* who = "vx_voxelize_meshes";
  vox_plan p;
  const int rc = vox_plan_meshes(tris, mesh_offsets, n_meshes, origin, h, dims, out, odd_columns, &p);
  if (rc != VX_OK) VX_FAIL(rc, "%s", p.err);
  vox_args g;
  g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2]; g.h = h;
  g.nz = p.nz; g.ny = p.ny; g.nx = p.nx; g.n_meshes = n_meshes;
  for (int m = 0; m <= VOX_MAX_MESHES; ++m) g.off[m] = m <= n_meshes ? mesh_offsets[m] : mesh_offsets[n_meshes];
  hipStream_t s = (hipStream_t)stream;
  // the counter is zeroed by a kernel, not by a memset: captured in a graph, the call is then kernel nodes only
  hipLaunchKernelGGL(voxelize_zero_kernel, dim3(1), dim3(1), 0, s, (unsigned long long*)odd_columns);
  VX_CHECK_LAUNCH(who);
  const dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y), wg(VOX_THREADS);
  hipLaunchKernelGGL(voxelize_kernel, grid, wg, 0, s, tris, g, out, (unsigned long long*)odd_columns);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}
