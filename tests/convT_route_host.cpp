// Stand-alone host program over values_amd/csrc/convT_route.h (the routing of vx_convT_k2s2: a pure function of its arguments),
// built with -fsanitize=address,undefined by tests/test_convT_route_cpu.py.  No GPU, no library, nothing loaded into Python.
//   1. walks the packed-size query and the route itself over grids of configurations, volumes, channels, batch sizes, single fields
//      and field pairs -- zero and negative values, sizes large enough to trip every 32-bit and 64-bit guard -- and prints what it
//      counted, and how many instances of the three lists an accepted route named;
//   2. routes the cases given on stdin ("id N D H W Cin Cout in_pitch out_pitch out_coff xblk half drop conv_fp32":
//      tests/convT_route_cases.py layer_args) and prints "case id rc kernel grid_x grid_y".
#include <stdio.h>
#include <string.h>

#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../values_amd/csrc/convT_route.h"

template <typename T>
static T* P(uintptr_t v) { return (T*)v; }
static int wrap(int64_t v) { return (int)(uint32_t)(uint64_t)v; }      // (a sum on a field that already holds an extreme value)

static vx_convT_args layer(int N, int D, int H, int W, int Cin, int Cout) {
  vx_convT_args a;
  memset(&a, 0, sizeof a);
  a.in = P<float>(0x10000); a.w_packed = P<float>(0x20000); a.bias = P<float>(0x30000); a.out = P<float>(0x40000);
  a.N = N; a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.in_pitch = Cin; a.out_pitch = Cout;
  a.range_flag = P<uint32_t>(0x60000);
  return a;
}

static unsigned long long g_sum = 0;
static void mix(long long v) { g_sum = g_sum * 1099511628211ull + (unsigned long long)v; }
static std::set<std::string> g_named;      // kernels accepted routes named

// a successful route must name an instance that exists and carry a usable geometry: every bound convT_route.h states for the
// kernel it chose, restated on the descriptor
static bool route_is_sound(const ConvTRoute& r, const vx_convT_args& a) {
  if (r.kernel < 0 || r.kernel >= CONVT_NKERNELS || !convT_instance_exists(r.kernel, r.cin, r.rt, r.mask)) return false;
  if (r.grid_x < 1 || r.grid_y < 1 || r.nvox < 1) return false;
  if (r.nvox != (int64_t)((vx_wide)a.N * a.D * a.H * a.W)) return false;
  if (r.mask != (a.drop_mode == VX_DROP_MASK) && r.kernel <= CONVT_S16) return false;
  if (r.kernel == CONVT_MFMA || r.kernel == CONVT_S16) {
    if (r.cin != a.Cin || r.nvox >= (1ll << 27) || r.ncoltiles < 1 || (int64_t)r.ncoltiles * 16 < r.nvox || (int64_t)r.ncoltiles * 16 >= r.nvox + 16) return false;
    if (r.grid_y * r.rt * 2 != a.Cout || (int64_t)r.grid_x * 4 >= (int64_t)r.ncoltiles + 4) return false;
    const int d[3] = {a.W, a.H, a.D};
    const unsigned m[3] = {r.mW, r.mH, r.mD};
    for (int i = 0; i < 3; ++i) {
      if ((vx_wide)r.nvox * d[i] >= ((vx_wide)1 << 32)) return false;
      // the decode at the largest index it meets: exact
      const unsigned v = (unsigned)(r.nvox - 1), q = m[i] ? (unsigned)(((uint64_t)v * m[i]) >> 32) : v;
      if (q != v / (unsigned)d[i]) return false;
    }
  } else {
    if ((int64_t)a.N * 2 * a.D >= (1ll << 31)) return false;
    if (r.kernel == CONVT_ROWS && (r.cin != a.Cin || r.total != (int64_t)((vx_wide)r.nvox * 2 * (a.Cout / 4)) || r.grid_y != 4 || r.grid_x > CONVT_ROWS_MAX_WGS)) return false;
    if (r.kernel == CONVT_GENERIC && (r.grid_y != a.Cout / 2 || r.grid_x > CONVT_GENERIC_MAX_WGS)) return false;
  }
  if ((vx_wide)a.D * a.H * a.W * 8 * a.Cout >= ((vx_wide)1 << 32)) return false;
  char name[128];
  const int n = convT_route_name(r, name, sizeof name);
  if (n <= 0 || n >= (int)sizeof name) return false;
  g_named.insert(name);
  return true;
}

static long long g_routes = 0, g_taken = 0, g_unsound = 0;
static void walk(const vx_convT_args& x, const vx_config& cfg) {
  ConvTRoute r;
  const int rc = convT_route(x, cfg, &r);
  ++g_routes; mix(rc);
  if (rc == VX_OK) { ++g_taken; g_unsound += !route_is_sound(r, x); mix(r.kernel); mix(convT_key(r.cin, r.rt) * 2 + r.mask); mix(r.grid_x); mix(r.grid_y); }
  else if (rc > 0 || !r.err[0]) ++g_unsound;   // a refusal is a VX_E_* code with a message
}

int main() {
  vx_config def;
  memset(&def, 0, sizeof def);
  std::vector<vx_config> cfgs(3, def);
  cfgs[1].conv_fp32 = 1; cfgs[2].conv_fp32 = 2;
  const int dims[] = {-7, 0, 1, 2, 3, 5, 8, 64, 65535, 65536, 1 << 20, 0x7fffffff};
  const int chans[] = {-8, 0, 4, 8, 12, 16, 24, 32, 64, 128, 136, 256};
  const int Ns[] = {1, 3, 0x7fffffff};
  const int nd = sizeof dims / sizeof *dims, nc = sizeof chans / sizeof *chans;

  // ---- 1a. the packed size ----
  long long points = 0;
  for (int i = 0; i < nc; ++i) for (int o = 0; o < nc; ++o) { ++points; mix(convT_packed_floats(chans[i], chans[o])); }
  for (int v : {0x7fffffff, 0x7ffffffc, 0x7ffffff8, 1 << 30}) for (int u : {0x7ffffff8, 1 << 30, 8}) { ++points; mix(convT_packed_floats(v, u)); }
  if (convT_packed_floats(16, 8) != 1024 || convT_packed_floats(6, 8) != -1 || convT_packed_floats(0x7ffffffc, 0x7ffffff8) != -1) ++g_unsound;
  printf("queries %lld points\n", points);

  // ---- 1b. the route: dense launches over the whole grid, then single fields and field pairs over a handful of layers ----
  for (const vx_config& cfg : cfgs)
    for (int n : Ns) for (int a = 0; a < nd; ++a) for (int b = 0; b < nd; ++b) for (int c = 0; c < nd; ++c)
      for (int i = 0; i < nc; ++i) for (int o = 0; o < nc; ++o) {
        vx_convT_args x = layer(n, dims[a], dims[b], dims[c], chans[i], chans[o]);
        if ((a + b + c + i + o) % 4 == 0) { x.drop_mode = VX_DROP_MASK; x.drop_mask = P<uint8_t>(0x50000); }
        walk(x, cfg);
      }
  typedef std::function<void(vx_convT_args&)> Mod;
  const std::vector<Mod> mods = {
    [](vx_convT_args& a) { a.in = nullptr; }, [](vx_convT_args& a) { a.w_packed = nullptr; }, [](vx_convT_args& a) { a.bias = nullptr; }, [](vx_convT_args& a) { a.out = nullptr; },
    [](vx_convT_args& a) { a.in = P<float>(0x10004); }, [](vx_convT_args& a) { a.out = P<float>(0x40008); }, [](vx_convT_args& a) { a.range_flag = nullptr; },
    [](vx_convT_args& a) { a.N = 0; }, [](vx_convT_args& a) { a.N = -1; }, [](vx_convT_args& a) { a.N = 3; }, [](vx_convT_args& a) { a.N = 1 << 20; }, [](vx_convT_args& a) { a.N = 0x7fffffff; },
    [](vx_convT_args& a) { a.D = 0; }, [](vx_convT_args& a) { a.D = 1; }, [](vx_convT_args& a) { a.D = 1 << 20; }, [](vx_convT_args& a) { a.D = 0x7fffffff; },
    [](vx_convT_args& a) { a.H = -7; }, [](vx_convT_args& a) { a.H = 65536; }, [](vx_convT_args& a) { a.H = 0x7fffffff; },
    [](vx_convT_args& a) { a.W = 0; }, [](vx_convT_args& a) { a.W = 3; }, [](vx_convT_args& a) { a.W = 65535; }, [](vx_convT_args& a) { a.W = 65536; }, [](vx_convT_args& a) { a.W = 1 << 20; },
    [](vx_convT_args& a) { a.W = 0x7fffffff; }, [](vx_convT_args& a) { a.W = 1 << 30; },
    [](vx_convT_args& a) { a.Cin = 0; }, [](vx_convT_args& a) { a.Cin = -8; }, [](vx_convT_args& a) { a.Cin = 6; }, [](vx_convT_args& a) { a.Cin = 12; }, [](vx_convT_args& a) { a.Cin = 16; },
    [](vx_convT_args& a) { a.Cin = 32; }, [](vx_convT_args& a) { a.Cin = 64; }, [](vx_convT_args& a) { a.Cin = 128; }, [](vx_convT_args& a) { a.Cin = 256; }, [](vx_convT_args& a) { a.Cin = 0x7ffffffc; },
    [](vx_convT_args& a) { a.Cout = 0; }, [](vx_convT_args& a) { a.Cout = -8; }, [](vx_convT_args& a) { a.Cout = 4; }, [](vx_convT_args& a) { a.Cout = 8; }, [](vx_convT_args& a) { a.Cout = 24; },
    [](vx_convT_args& a) { a.Cout = 64; }, [](vx_convT_args& a) { a.Cout = 136; }, [](vx_convT_args& a) { a.Cout = 1 << 20; }, [](vx_convT_args& a) { a.Cout = 0x7ffffff8; },
    [](vx_convT_args& a) { a.in_pitch = 0; }, [](vx_convT_args& a) { a.in_pitch = wrap((int64_t)a.Cin - 4); }, [](vx_convT_args& a) { a.in_pitch = wrap((int64_t)a.Cin + 2); },
    [](vx_convT_args& a) { a.in_pitch = wrap((int64_t)a.Cin + 4); }, [](vx_convT_args& a) { a.in_pitch = 0x7ffffffc; },
    [](vx_convT_args& a) { a.out_pitch = 0; }, [](vx_convT_args& a) { a.out_pitch = wrap((int64_t)a.Cout + 2); }, [](vx_convT_args& a) { a.out_pitch = wrap((int64_t)a.Cout - 4); },
    [](vx_convT_args& a) { a.out_pitch = 0x7ffffffc; }, [](vx_convT_args& a) { a.out_coff = 4; a.out_pitch = wrap((int64_t)a.out_pitch + 4); },
    [](vx_convT_args& a) { a.out_coff = 2; a.out_pitch = wrap((int64_t)a.out_pitch + 4); }, [](vx_convT_args& a) { a.out_coff = 4; }, [](vx_convT_args& a) { a.out_coff = -4; },
    [](vx_convT_args& a) { a.out_coff = 0x7ffffffc; }, [](vx_convT_args& a) { a.out_coff = (int)0x80000000; },
    [](vx_convT_args& a) { a.out_xblk = 1; }, [](vx_convT_args& a) { a.out_xblk = 2; }, [](vx_convT_args& a) { a.out_xblk = 3; }, [](vx_convT_args& a) { a.out_xblk = 4; },
    [](vx_convT_args& a) { a.out_xblk = -1; }, [](vx_convT_args& a) { a.out_xblk = (int)0x80000000; }, [](vx_convT_args& a) { a.out_half = 1; }, [](vx_convT_args& a) { a.out_half = 2; }, [](vx_convT_args& a) { a.out_half = -1; },
    [](vx_convT_args& a) { a.act = VX_ACT_RELU; }, [](vx_convT_args& a) { a.act = VX_ACT_LRELU; }, [](vx_convT_args& a) { a.act = 7; },
    [](vx_convT_args& a) { a.drop_mode = VX_DROP_HASH; }, [](vx_convT_args& a) { a.drop_mode = VX_DROP_MASK; }, [](vx_convT_args& a) { a.drop_mode = 3; },
    [](vx_convT_args& a) { a.drop_mask = P<uint8_t>(0x50000); }, [](vx_convT_args& a) { a.drop_mode = VX_DROP_MASK; a.drop_mask = P<uint8_t>(0x50000); },
  };
  // (N, D, H, W, Cin, Cout)
  const int layers[][6] = {{2, 4, 4, 4, 16, 8}, {1, 3, 5, 7, 32, 16}, {2, 4, 4, 4, 64, 32}, {2, 3, 5, 6, 128, 64}, {2, 2, 2, 2, 8, 8}, {2, 2, 2, 2, 24, 16},
                           {1, 1, 1, 65535, 16, 8}, {1, 1, 1, 65536, 16, 8}, {1, 1, 1, 65536, 16, 24}, {10, 32, 32, 32, 16, 8}, {1 << 23, 1, 1, 16, 32, 16}};
  const int nm = (int)mods.size();
  for (const vx_config& cfg : cfgs)
    for (const auto& L : layers)
      for (int i = -1; i < nm; ++i) for (int j = i; j < nm; ++j) {
        if (i >= 0 && j == i) continue;
        vx_convT_args x = layer(L[0], L[1], L[2], L[3], L[4], L[5]);
        if (i >= 0) mods[i](x);
        if (j >= 0) mods[j](x);
        walk(x, cfg);
      }
  printf("routes %lld taken %lld unsound %lld checksum %016llx\n", g_routes, g_taken, g_unsound, g_sum);

  // ---- 1c. every instance of the three lists, with and without the mask, and the generic kernel were named by an accepted route ----
  int listed = 0, missing = 0;
  ConvTRoute r;
  auto seen = [&](int kernel, int cin, int rt, int mask) {
    char name[128];
    r.kernel = kernel; r.cin = cin; r.rt = rt; r.mask = mask;
    convT_route_name(r, name, sizeof name);
    ++listed;
    if (!g_named.count(name)) { ++missing; printf("never routed: %s\n", name); }
  };
#define SEEN_MFMA(CIN, RT) seen(CONVT_MFMA, CIN, RT, 0); seen(CONVT_MFMA, CIN, RT, 1);
#define SEEN_S16(CIN, RT) seen(CONVT_S16, CIN, RT, 0); seen(CONVT_S16, CIN, RT, 1);
  CONVT_MFMA_INSTANCES(SEEN_MFMA)
  CONVT_S16_INSTANCES(SEEN_S16)
  seen(CONVT_ROWS, 16, 0, 0); seen(CONVT_GENERIC, 0, 0, 0);     // (the rows kernel's two instances share one name)
  printf("instances listed %d named %d missing %d\n", listed, (int)g_named.size(), missing);

  // ---- 2. the cases on stdin ----
  char id[128];
  int N, D, H, W, Cin, Cout, ip, op, oc, xb, half, drop, fp32;
  while (scanf("%127s %d %d %d %d %d %d %d %d %d %d %d %d %d", id, &N, &D, &H, &W, &Cin, &Cout, &ip, &op, &oc, &xb, &half, &drop, &fp32) == 14) {
    vx_config cfg = def;
    cfg.conv_fp32 = fp32;
    vx_convT_args x = layer(N, D, H, W, Cin, Cout);
    x.in_pitch = ip; x.out_pitch = op; x.out_coff = oc; x.out_xblk = xb; x.out_half = half; x.drop_mode = drop;
    if (drop == VX_DROP_MASK) x.drop_mask = P<uint8_t>(0x50000);
    memset(&r, 0, sizeof r);
    const int rc = convT_route(x, cfg, &r);
    char name[128] = "-";
    if (rc == VX_OK) convT_route_name(r, name, sizeof name);
    printf("case %s %d %s %d %d\n", id, rc, name, r.grid_x, r.grid_y);
  }
  return (g_unsound || missing || (int)g_named.size() != listed) ? 1 : 0;
}
