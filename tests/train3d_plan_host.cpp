// Stand-alone driver of values_amd/csrc/train3d_plan.h, the host plan of vx_train_patches_3d (argument checks, item table,
// lane decomposition), built under -fsanitize=address,undefined by tests/test_train3d_plan_cpu.py.  The pointers are
// made-up addresses: the plan never dereferences them.
//   train3d_plan_host  ->  refusals: "<name> <code>"; decomposition: "cover <P0>x<P1>x<P2> <cases> <lanes>", and a line
//                          "BAD-..." for every broken property
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../values_amd/csrc/train3d_plan.h"

static void* at(uintptr_t a) { return (void*)a; }
static const uintptr_t IMG = 0x100000, LAB = 0x200000, DATA = 0x300000, SEG = 0x400000, SIG = 0x500000, ST = 0x600000, WS = 0x700000;

static vx_train3d_item item(int d0, int d1, int d2, int o0, int o1, int o2, int flags = 0) {
  vx_train3d_item it = {};
  it.image = at(IMG); it.label = at(LAB);
  it.image_kind = VX_PREP_F32; it.label_kind = VX_COUNT_B2; it.label_flags = 0;
  it.dims[0] = d0; it.dims[1] = d1; it.dims[2] = d2;
  it.origin[0] = o0; it.origin[1] = o1; it.origin[2] = o2;
  it.flags = flags; it.index = 0;
  return it;
}

struct call {
  std::vector<vx_train3d_item> items = {item(8, 8, 8, 4, 4, 4, 5)};
  int n = 1, P0 = 4, P1 = 4, P2 = 4, seg_u8 = 0, law = 0;
  bool table = true;
  uintptr_t data = DATA, seg = SEG, sig = SIG, st = ST, ws = WS;
  float lo = 0.f, hi = 0.1f;
  int64_t ws_n = 1 << 20;
};

static void refusal(const char* name, const call& c) {
  t3_plan p;
  const int rc = t3_make_plan(c.table ? c.items.data() : nullptr, c.n, c.P0, c.P1, c.P2, at(c.data), at(c.seg), c.seg_u8, c.lo, c.hi, c.law,
                              at(c.sig), at(c.st), at(c.ws), c.ws_n, &p);
  printf("%s %d\n", name, rc);
  if (rc != p.code) printf("%s BAD-CODE\n", name);
  if ((rc != VX_OK) != (strstr(p.err, "vx_train_patches_3d") != nullptr)) printf("%s BAD-MESSAGE\n", name);
}

// every output voxel of every item is written exactly once, from the source element numpy's crop-and-flip names, and no lane
// reads outside its crop
static void cover(int P0, int P1, int P2, const int dims[3]) {
  const int P[3] = {P0, P1, P2};
  std::vector<vx_train3d_item> items;
  for (int a = 0; a < 3; ++a)
    if (dims[a] < P[a]) return;
  const int cand[5] = {0, 1, 2, 3, -1};
  for (int zi = 0; zi < 5; ++zi)
    for (int mask = 0; mask < 8; ++mask) {
      int o[3];
      for (int a = 0; a < 3; ++a) {   // origins 0, 1, 2, 3 and the last one; one past the last becomes the last
        const int c = cand[a == 2 ? zi : (zi + mask + a) % 5];
        o[a] = c < 0 || c > dims[a] - P[a] ? dims[a] - P[a] : c;
      }
      items.push_back(item(dims[0], dims[1], dims[2], o[0], o[1], o[2], mask | (zi & 1 ? 8 : 0)));
    }
  t3_plan p;
  const int n = (int)items.size();
  const int rc = t3_make_plan(items.data(), n, P0, P1, P2, at(DATA), at(SEG), 1, 0.f, 0.1f, 1, nullptr, at(ST), at(WS), t3_workspace_bytes(n), &p);
  if (rc != VX_OK) { printf("cover BAD-PLAN %d %s\n", rc, p.err); return; }
  if (p.lanes != (int64_t)n * p.shape.per || p.grid < 1 || p.grid > T3_MAX_GRID || (int64_t)p.grid * T3_THREADS < (p.lanes < (int64_t)T3_MAX_GRID * T3_THREADS ? p.lanes : 0))
    printf("cover BAD-GRID\n");
  const int64_t pv = p.shape.pv;
  std::vector<int> hits((size_t)(n * pv), 0);
  for (int64_t i = 0; i < p.lanes; ++i) {
    const int it = (int)(i / p.shape.per);
    const t3_item& g = p.table[(size_t)it];
    const t3_lane l = t3_lane_of(p.shape, i - (int64_t)it * p.shape.per, g.D1, g.D2, g.o0, g.o1, g.o2, g.flags);
    if (l.n < 1 || l.n > 4 || l.k0 + l.n > P2 || l.a < 0 || l.a >= P0 || l.b < 0 || l.b >= P1) { printf("cover BAD-LANE\n"); continue; }
    if (l.dst != ((int64_t)l.a * P1 + l.b) * P2 + l.k0) printf("cover BAD-DST\n");
    for (int u = 0; u < l.n; ++u) {
      const int64_t e = l.src + (l.rev ? l.n - 1 - u : u);       // the element output z = k0 + u takes
      const int sz = (int)(e % g.D2), sy = (int)(e / g.D2 % g.D1), sx = (int)(e / g.D2 / g.D1);
      const int wx = g.o0 + ((g.flags & 1) ? P0 - 1 - l.a : l.a), wy = g.o1 + ((g.flags & 2) ? P1 - 1 - l.b : l.b);
      const int wz = g.o2 + ((g.flags & 4) ? P2 - 1 - (l.k0 + u) : l.k0 + u);
      if (sx != wx || sy != wy || sz != wz) printf("cover BAD-SOURCE\n");
      if (sx < g.o0 || sx >= g.o0 + P0 || sy < g.o1 || sy >= g.o1 + P1 || sz < g.o2 || sz >= g.o2 + P2) printf("cover BAD-OUTSIDE\n");
      ++hits[(size_t)(it * pv + l.dst + u)];
    }
    // the run a vector access would read, [src, src + n), lies inside the crop's row
    const int z0 = (int)(l.src % g.D2);
    if (z0 < g.o2 || z0 + l.n > g.o2 + P2) printf("cover BAD-RUN\n");
  }
  for (int h : hits)
    if (h != 1) { printf("cover BAD-COVER\n"); break; }
  printf("cover %dx%dx%d %d %lld\n", P0, P1, P2, n, (long long)p.lanes);
}

int main() {
  call ok;
  refusal("ok", ok);
  { call c; c.table = false; refusal("null_table", c); }
  { call c; c.data = 0; refusal("null_data", c); }
  { call c; c.st = 0; refusal("null_status", c); }
  { call c; c.ws = 0; refusal("null_workspace", c); }
  { call c; c.items[0].image = nullptr; refusal("null_image", c); }
  { call c; c.seg = 0; c.sig = 0; c.items[0].label = nullptr; refusal("ok_no_seg", c); }
  { call c; c.n = 0; refusal("n_zero", c); }
  { call c; c.n = VX_SELECT_MAX_ITEMS + 1; refusal("n_over", c); }
  { call c; c.n = -1; refusal("n_negative", c); }
  { call c; c.P1 = 0; refusal("p_zero", c); }
  { call c; c.items[0].dims[2] = 0; refusal("dim_zero", c); }
  { call c; c.items[0].origin[2] = 5; refusal("crop_past", c); }
  { call c; c.items[0].origin[0] = -1; refusal("crop_before", c); }
  { call c; c.P0 = 9; c.items[0].origin[0] = 0; refusal("volume_small", c); }
  { call c; c.P0 = 1 << 11; c.P1 = 1 << 11; c.P2 = 1 << 10; refusal("p_2_32", c); }
  { call c; c.P0 = 1 << 11; c.P1 = 1 << 11; c.P2 = (1 << 10) - 1; c.items[0] = item(1 << 11, 1 << 11, 1 << 10, 0, 0, 0); refusal("ok_below_2_32", c); }
  { call c; c.lo = -0.5f; refusal("var_negative", c); }
  { call c; c.lo = 0.2f; refusal("var_order", c); }
  { call c; c.hi = __builtin_nanf(""); refusal("var_nan", c); }
  { call c; c.items[0].image_kind = 8; refusal("kind_image", c); }
  { call c; c.items[0].image_kind = -1; refusal("kind_image_neg", c); }
  { call c; c.items[0].label_kind = VX_COUNT_F32; refusal("kind_label", c); }
  { call c; c.items[0].flags = 16; refusal("flags_high", c); }
  { call c; c.items[0].flags = -1; refusal("flags_neg", c); }
  { call c; c.items[0].label_flags = 2; refusal("label_flags", c); }
  { call c; c.law = 2; refusal("law", c); }
  { call c; c.data += 2; refusal("align_data", c); }
  { call c; c.seg += 2; refusal("align_seg", c); }
  { call c; c.seg += 1; c.seg_u8 = 1; refusal("ok_seg_u8_odd", c); }
  { call c; c.sig += 2; refusal("align_sigma", c); }
  { call c; c.st += 1; refusal("align_status", c); }
  { call c; c.items[0].image = at(IMG + 2); refusal("align_image", c); }
  { call c; c.items[0].label = at(LAB + 1); refusal("align_label", c); }
  { call c; c.ws += 8; refusal("align_workspace", c); }
  { call c; c.ws_n = t3_workspace_bytes(1) - 1; refusal("workspace_short", c); }
  { call c; c.items.assign((size_t)VX_SELECT_MAX_ITEMS, item(8, 8, 8, 0, 0, 0)); c.n = VX_SELECT_MAX_ITEMS; c.ws_n = t3_workspace_bytes(c.n); refusal("ok_max", c); }

  const int patches[7][3] = {{1, 1, 1}, {2, 3, 1}, {3, 5, 6}, {4, 4, 4}, {5, 5, 5}, {7, 2, 9}, {8, 8, 8}};
  const int volumes[3][3] = {{9, 7, 13}, {8, 8, 8}, {5, 6, 21}};
  for (const auto& P : patches) {
    for (const auto& V : volumes) cover(P[0], P[1], P[2], V);
    cover(P[0], P[1], P[2], P);
  }
  // past the grid cap: the launch keeps T3_MAX_GRID workgroups and the loop takes another trip
  if (t3_grid((int64_t)T3_MAX_GRID * T3_THREADS) != T3_MAX_GRID || t3_grid((int64_t)T3_MAX_GRID * T3_THREADS + 1) != T3_MAX_GRID || t3_grid(1) != 1 ||
      t3_grid(T3_THREADS + 1) != 2)
    printf("grid BAD-CAP\n");
  return 0;
}
