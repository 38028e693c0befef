// Host-side plan of the mesh voxeliser (voxelize.hip, K44): the argument checks, the tile of columns a workgroup owns,
// the mask words of a column and the grid.  Plain C++ with no HIP in it, so a stand-alone program can run it under a
// host sanitizer (tests/voxel_plan_host.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/values_amd.h"
#include "host_checks.h"

// A workgroup is four waves on ONE row of 64 columns.  The voxeliser is bound by the latency of a wave's walk over its list,
// not by throughput: the volumes are small against the machine, so a tile one sample high gives the most
// workgroups and the shortest lists, and the four waves divide the triangle scan and the list among them.
#define VOX_THREADS 256
#define VOX_TILE_X 64                       // lanes run along x: a wave's stores are contiguous row segments
#define VOX_TILE_Y 1
#define VOX_WAVES (VOX_THREADS / VOX_TILE_X)
#define VOX_K_PER_WAVE (64 / VOX_WAVES)     // of the 64 k of a mask word, the ones a wave stores
#define VOX_CHUNK VOX_THREADS               // triangles a workgroup looks at per step, one per thread: the LDS list's size
#define VOX_MAX_MESHES 16
#define VOX_MAX_DIM 1024
#define VOX_MAX_WORDS (VOX_MAX_DIM / 64)    // 64-bit mask words of one column
#define VOX_MAX_TRIS ((int64_t)1 << 20)

struct vox_plan {
  int32_t nz = 0, ny = 0, nx = 0;
  int32_t tiles_x = 0, tiles_y = 0;   // the grid: blockIdx.x, blockIdx.y
  int32_t words = 0;                  // mask words in use: ceil(nz / 64)
  int64_t n_tri = 0;
  int64_t chunks = 0;                 // steps over all meshes: each mesh is scanned in its own steps
  int code = VX_OK;
  char err[160] = {0};
};

static inline int vox_plan_meshes(const void* tris, const int64_t* mesh_offsets, int n_meshes, const double* origin, double h,
                                  const int32_t* dims, const void* out, const void* odd_columns, vox_plan* p) {
  const char* who = "vx_voxelize_meshes";
  if (!tris || !mesh_offsets || !origin || !dims || !out || !odd_columns) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null pointer", who);
  if (n_meshes < 1 || n_meshes > VOX_MAX_MESHES) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_meshes %d outside 1..%d", who, n_meshes, VOX_MAX_MESHES);
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 1 || dims[a] > VOX_MAX_DIM) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: dims[%d] = %d outside 1..%d", who, a, dims[a], VOX_MAX_DIM);
  if (mesh_offsets[0] != 0) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: mesh_offsets[0] = %lld, not 0", who, (long long)mesh_offsets[0]);
  int64_t chunks = 0;
  for (int m = 0; m < n_meshes; ++m) {
    if (mesh_offsets[m + 1] <= mesh_offsets[m] || mesh_offsets[m + 1] > VOX_MAX_TRIS)
      VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: mesh_offsets[%d] = %lld: offsets increase from 0 to n_tri <= 2^20", who, m + 1, (long long)mesh_offsets[m + 1]);
    chunks += (mesh_offsets[m + 1] - mesh_offsets[m] + VOX_CHUNK - 1) / VOX_CHUNK;
  }
  if (!(h > 0) || !isfinite(h)) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: h = %g is not finite and positive", who, h);
  for (int a = 0; a < 3; ++a)
    if (!isfinite(origin[a])) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: origin[%d] is not finite", who, a);
  if (((uintptr_t)tris & 3) || ((uintptr_t)out & 3)) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: tris or out not aligned to its 4-byte elements", who);
  if ((uintptr_t)odd_columns & 7) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: odd_columns not aligned to its 8-byte element", who);
  p->nz = dims[0]; p->ny = dims[1]; p->nx = dims[2];
  p->tiles_x = (p->nx + VOX_TILE_X - 1) / VOX_TILE_X;
  p->tiles_y = (p->ny + VOX_TILE_Y - 1) / VOX_TILE_Y;
  p->words = (p->nz + 63) / 64;
  p->n_tri = mesh_offsets[n_meshes];
  p->chunks = chunks;
  return VX_OK;
}
