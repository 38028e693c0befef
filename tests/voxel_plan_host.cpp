// Stand-alone driver of values_amd/csrc/voxel_plan.h, the host plan of the mesh voxeliser (argument checks, tile
// arithmetic, mask words, grid), built under -fsanitize=address,undefined by tests/test_stl_cpu.py.  The device pointers
// are made-up addresses: the plan never dereferences them.
//   voxel_plan_host  ->  one line per case: "<name> <code> [tiles_x tiles_y words n_tri chunks]", "BAD-..." on a broken invariant
#include <math.h>
#include <stdio.h>

#include "../values_amd/csrc/voxel_plan.h"

static void* at(uintptr_t a) { return (void*)a; }

static int run(const char* name, const void* tris, const int64_t* off, int n_meshes, const double* origin, double h, const int32_t* dims,
               const void* out, const void* odd) {
  vox_plan p;
  const int rc = vox_plan_meshes(tris, off, n_meshes, origin, h, dims, out, odd, &p);
  if (rc != VX_OK) {
    printf("%s %d\n", name, rc);
    if (p.code != rc || !p.err[0]) printf("%s BAD-ERR\n", name);
    return rc;
  }
  printf("%s %d %d %d %d %lld %lld\n", name, rc, p.tiles_x, p.tiles_y, p.words, (long long)p.n_tri, (long long)p.chunks);
  // every column and every k is owned by exactly one tile / word, and nothing lies past the limits the kernel's LDS has
  if ((int64_t)p.tiles_x * VOX_TILE_X < p.nx || (int64_t)(p.tiles_x - 1) * VOX_TILE_X >= p.nx) printf("%s BAD-TILES-X\n", name);
  if ((int64_t)p.tiles_y * VOX_TILE_Y < p.ny || (int64_t)(p.tiles_y - 1) * VOX_TILE_Y >= p.ny) printf("%s BAD-TILES-Y\n", name);
  if (p.words * 64 < p.nz || (p.words - 1) * 64 >= p.nz || p.words > VOX_MAX_WORDS) printf("%s BAD-WORDS\n", name);
  if (p.n_tri != off[n_meshes] || p.chunks * VOX_CHUNK < p.n_tri || p.chunks > p.n_tri) printf("%s BAD-CHUNKS\n", name);
  if (p.nz != dims[0] || p.ny != dims[1] || p.nx != dims[2]) printf("%s BAD-DIMS\n", name);
  return rc;
}

int main() {
  const uintptr_t T = 0x10000, O = 0x4000000, C = 0x8000000;
  const double org[3] = {-1.0, -1.0, -1.0}, org_nan[3] = {-1.0, NAN, -1.0};
  const int64_t one[2] = {0, 12}, two[3] = {0, 12, 972};
  const int32_t d70[3] = {70, 70, 70};
  run("v_ok", at(T), one, 1, org, 0.1, d70, at(O), at(C));
  run("v_two", at(T), two, 2, org, 0.1, d70, at(O), at(C));

  // the limits of every dimension: 1, a tile, a tile + 1, 1024; 0 and 1025 refused
  const int edge[] = {0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025};
  for (int a = 0; a < 3; ++a)
    for (int v : edge) {
      int32_t d[3] = {7, 7, 7};
      d[a] = v;
      char name[32];
      snprintf(name, sizeof(name), "v_dim%d_%d", a, v);
      const int rc = run(name, at(T), one, 1, org, 0.5, d, at(O), at(C));
      if ((rc == VX_OK) != (v >= 1 && v <= 1024)) printf("%s BAD-LIMIT\n", name);
    }
  const int32_t dmax[3] = {1024, 1024, 1024};
  run("v_max", at(T), one, 1, org, 1e-3, dmax, at(O), at(C));

  // meshes: 1..16, offsets increasing from 0 to n_tri <= 2^20
  int64_t many[18];
  for (int i = 0; i < 18; ++i) many[i] = 300 * i;
  run("v_m16", at(T), many, 16, org, 0.1, d70, at(O), at(C));
  run("v_m17", at(T), many, 17, org, 0.1, d70, at(O), at(C));
  run("v_m0", at(T), many, 0, org, 0.1, d70, at(O), at(C));
  run("v_mneg", at(T), many, -1, org, 0.1, d70, at(O), at(C));
  const int64_t big[2] = {0, (int64_t)1 << 20}, big1[2] = {0, ((int64_t)1 << 20) + 1}, empty[2] = {0, 0}, from1[2] = {1, 12};
  const int64_t flat[3] = {0, 12, 12}, back[3] = {0, 12, 5}, neg[2] = {0, -3};
  run("v_tri_max", at(T), big, 1, org, 0.1, d70, at(O), at(C));
  run("v_tri_over", at(T), big1, 1, org, 0.1, d70, at(O), at(C));
  run("v_tri_zero", at(T), empty, 1, org, 0.1, d70, at(O), at(C));
  run("v_off_from1", at(T), from1, 1, org, 0.1, d70, at(O), at(C));
  run("v_off_flat", at(T), flat, 2, org, 0.1, d70, at(O), at(C));
  run("v_off_back", at(T), back, 2, org, 0.1, d70, at(O), at(C));
  run("v_off_neg", at(T), neg, 1, org, 0.1, d70, at(O), at(C));

  // h and origin
  run("v_h0", at(T), one, 1, org, 0.0, d70, at(O), at(C));
  run("v_hneg", at(T), one, 1, org, -0.1, d70, at(O), at(C));
  run("v_hnan", at(T), one, 1, org, NAN, d70, at(O), at(C));
  run("v_hinf", at(T), one, 1, org, INFINITY, d70, at(O), at(C));
  run("v_hmin", at(T), one, 1, org, 4.9e-324, d70, at(O), at(C));
  run("v_org_nan", at(T), one, 1, org_nan, 0.1, d70, at(O), at(C));

  // null pointers and alignment
  run("v_null_tris", nullptr, one, 1, org, 0.1, d70, at(O), at(C));
  run("v_null_off", at(T), nullptr, 1, org, 0.1, d70, at(O), at(C));
  run("v_null_org", at(T), one, 1, nullptr, 0.1, d70, at(O), at(C));
  run("v_null_dims", at(T), one, 1, org, 0.1, nullptr, at(O), at(C));
  run("v_null_out", at(T), one, 1, org, 0.1, d70, nullptr, at(C));
  run("v_null_odd", at(T), one, 1, org, 0.1, d70, at(O), nullptr);
  run("v_align_tris", at(T + 2), one, 1, org, 0.1, d70, at(O), at(C));
  run("v_align_out", at(T), one, 1, org, 0.1, d70, at(O + 1), at(C));
  run("v_align_odd", at(T), one, 1, org, 0.1, d70, at(O), at(C + 4));
  run("v_align4_ok", at(T + 4), one, 1, org, 0.1, d70, at(O + 4), at(C + 8));
  return 0;
}
