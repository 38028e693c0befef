// Stand-alone host program over values_amd/csrc/conv2d_route.h (the routing of vx_conv2d: a pure function of its arguments),
// built with -fsanitize=address,undefined by tests/test_conv2d_route_cpu.py.  No GPU, no library, nothing loaded into Python.
//   1. walks the queries and the route itself over grids of configurations, image sizes, channels, kernel sizes, strides, pitches,
//      single flags and flag pairs -- zero and negative values, sizes and pitches large enough to trip the 2 GiB guards -- and
//      prints what it counted, and how many instances of the two lists an accepted route named;
//   2. routes the single-layer cases given on stdin ("id KS S H W Cin Cout N epi c2s_no_wide c2s_no_oct conv_fp32", Cin the REAL
//      channel count: tests/conv2d_route_cases.py layer_args) and prints "case id rc kernel nchunks w_all grid_x grid_y".
#include <stdio.h>
#include <string.h>

#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../values_amd/csrc/conv2d_route.h"

template <typename T>
static T* P(uintptr_t v) { return (T*)v; }
static int wrap(int64_t v) { return (int)(uint32_t)(uint64_t)v; }      // (a mod on a field that already holds an extreme value)
static int r4(int c) { return wrap(((int64_t)c + 3) / 4 * 4); }

// a layer as HighResolutionNet launches it: `cin` REAL input channels at pitch round4, padded to 16 for the kernel; the weights'
// family is that of the real count
static vx_conv2d_args layer(int N, int H, int W, int cin, int Cout, int KS, int S, bool epi, const vx_config& cfg) {
  vx_conv2d_args a;
  memset(&a, 0, sizeof a);
  a.in = P<float>(0x10000); a.w_packed = P<float>(0x20000); a.bias = P<float>(0x30000); a.out = P<float>(0x40000);
  a.N = N; a.H = H; a.W = W; a.Cin = (int)conv2d_cin_padded(cin); a.Cout = Cout; a.KS = KS; a.S = S;
  a.in_pitch = r4(cin); a.out_pitch = r4(Cout);
  a.w_family = conv2d_family(cin, Cout, KS, cfg);
  if (epi) {
    a.out_scale = P<float>(0x60000); a.out_shift = P<float>(0x70000); a.out_add = P<float>(0x80000); a.out_add_pitch = r4(Cout);
    a.out_act = VX_ACT_RELU;
  } else {
    a.stats_partial = P<float>(0x50000);
  }
  return a;
}

static unsigned long long g_sum = 0;
static void mix(long long v) { g_sum = g_sum * 1099511628211ull + (unsigned long long)v; }
static std::set<std::string> g_named;      // instances accepted routes named

// a successful route must name an instance that exists and carry a usable geometry
static bool route_is_sound(const Conv2dRoute& r, const vx_conv2d_args& a) {
  if (r.kernel < 0 || r.kernel >= CONV2D_NKERNELS || !conv2d_instance_exists(r.kernel, r.p)) return false;
  if (r.tiles_x < 1 || r.tiles_y < 1 || r.OH < 1 || r.OW < 1 || r.nchunks < 1 || r.grid_y < 1) return false;
  if (r.grid_x < 1 || r.grid_x > (int64_t)a.N * r.tiles_x * r.tiles_y) return false;
  if (r.lds_bytes < 1 || r.lds_bytes > C2_LDS_BYTES) return false;
  if (r.w_all != 0 && (r.w_all != 1 || r.nchunks < 2 || r.kernel != CONV2D_S16)) return false;
  char name[128];
  const int n = conv2d_route_name(r, name, sizeof name);
  if (n <= 0 || n >= (int)sizeof name) return false;
  g_named.insert(name);
  return true;
}

static long long g_routes = 0, g_taken = 0, g_unsound = 0;
static void walk(const vx_conv2d_args& x, const vx_config& cfg) {
  Conv2dRoute r;
  const int rc = conv2d_route(x, cfg, &r);
  ++g_routes; mix(rc);
  if (rc == VX_OK) { ++g_taken; g_unsound += !route_is_sound(r, x); mix(r.kernel); mix((long long)conv2d_key_of(r.p)); mix(r.grid_x); mix(r.lds_bytes); }
  else if (rc > 0 || !r.err[0]) ++g_unsound;   // a refusal is a VX_E_* code with a message
}

int main() {
  vx_config def;
  memset(&def, 0, sizeof def);
  std::vector<vx_config> cfgs(6, def);
  cfgs[1].conv_fp32 = 1; cfgs[2].conv_fp32 = 2; cfgs[3].c2s_no_wide = 1; cfgs[4].c2s_no_oct = 1; cfgs[5].c2s_no_wide = 1; cfgs[5].c2s_no_oct = 1;
  const int dims[] = {-7, 0, 1, 5, 7, 16, 17, 33, 112, 1 << 20, 0x7fffffff};
  const int cins[] = {-8, 0, 3, 8, 9, 16, 18, 24, 25, 32, 48, 64, 80, 256, 720, 0x7ffffff0};   // REAL channels
  const int couts[] = {-8, 0, 1, 16, 18, 19, 32, 48, 72, 144, 270, 720, 0x7fffffff};
  const int kss[][2] = {{3, 1}, {3, 2}, {1, 1}, {1, 2}, {5, 1}, {3, 0}, {3, 3}, {0, 1}, {-3, -1}};
  const int nd = sizeof dims / sizeof *dims, nci = sizeof cins / sizeof *cins, nco = sizeof couts / sizeof *couts, nk = sizeof kss / sizeof *kss;

  // ---- 1a. the queries ----
  long long points = 0;
  for (int a = 0; a < nd; ++a) for (int b = 0; b < nd; ++b) for (int k = 0; k < nk; ++k) { ++points; mix(conv2d_tiles(dims[a], dims[b], kss[k][0], kss[k][1])); }
  for (const vx_config& cfg : cfgs)
    for (int i = 0; i < nci; ++i) for (int o = 0; o < nco; ++o) for (int k = 0; k < nk; ++k) {
      ++points;
      mix(conv2d_family(cins[i], couts[o], kss[k][0], cfg)); mix(conv2d_packed_floats(cins[i], couts[o], kss[k][0], cfg));
      mix(conv2d_s16_octets(cins[i], kss[k][0], cfg));
    }
  printf("queries %lld points\n", points);

  // ---- 1b. the route: layers over the whole grid, then single flags and flag pairs over a handful of layers ----
  for (const vx_config& cfg : cfgs)
    for (int a = 0; a < nd; ++a) for (int b = 0; b < nd; ++b) for (int i = 0; i < nci; ++i) for (int o = 0; o < nco; ++o) for (int k = 0; k < nk; ++k) {
      const int Ns[3] = {1, 3, 0x7fffffff};
      vx_conv2d_args x = layer(Ns[(a + b + i + o) % 3], dims[a], dims[b], cins[i], couts[o], kss[k][0], kss[k][1], (a + b + i + o + k) % 2, cfg);
      if (cins[i] <= 0) x.Cin = cins[i];           // (the padded count of a real count that is none)
      walk(x, cfg);
    }
  typedef std::function<void(vx_conv2d_args&)> Mod;
  const std::vector<Mod> mods = {
    [](vx_conv2d_args& a) { a.in = nullptr; }, [](vx_conv2d_args& a) { a.w_packed = nullptr; }, [](vx_conv2d_args& a) { a.out = nullptr; },
    [](vx_conv2d_args& a) { a.bias = nullptr; }, [](vx_conv2d_args& a) { a.bias = P<float>(0x30004); },
    [](vx_conv2d_args& a) { a.in = P<float>(0x10004); }, [](vx_conv2d_args& a) { a.out = P<float>(0x40008); }, [](vx_conv2d_args& a) { a.w_packed = P<float>(0x2000c); },
    [](vx_conv2d_args& a) { a.N = 0; }, [](vx_conv2d_args& a) { a.N = -1; }, [](vx_conv2d_args& a) { a.N = 0x7fffffff; },
    [](vx_conv2d_args& a) { a.H = 0; }, [](vx_conv2d_args& a) { a.W = -1; }, [](vx_conv2d_args& a) { a.H = 0x7fffffff; }, [](vx_conv2d_args& a) { a.W = 1 << 24; },
    [](vx_conv2d_args& a) { a.Cin = 0; }, [](vx_conv2d_args& a) { a.Cin = 12; }, [](vx_conv2d_args& a) { a.Cin = wrap((int64_t)a.Cin + 16); }, [](vx_conv2d_args& a) { a.Cout = -8; },
    [](vx_conv2d_args& a) { a.Cout = 0x7fffffff; },
    [](vx_conv2d_args& a) { a.KS = 5; }, [](vx_conv2d_args& a) { a.KS = 1; }, [](vx_conv2d_args& a) { a.S = 2; }, [](vx_conv2d_args& a) { a.S = 0; }, [](vx_conv2d_args& a) { a.S = 3; },
    [](vx_conv2d_args& a) { a.w_family = 0; }, [](vx_conv2d_args& a) { a.w_family = 3; }, [](vx_conv2d_args& a) { a.w_family = wrap((int64_t)a.w_family + 100); },
    [](vx_conv2d_args& a) { a.w_family = wrap((int64_t)a.w_family + 300); }, [](vx_conv2d_args& a) { a.w_family = 0x7fffffff; }, [](vx_conv2d_args& a) { a.w_family = -112; },
    [](vx_conv2d_args& a) { a.in_pitch = wrap((int64_t)a.Cin - 16); }, [](vx_conv2d_args& a) { a.in_pitch = wrap((int64_t)a.Cin - 12); }, [](vx_conv2d_args& a) { a.in_pitch = wrap((int64_t)a.Cin + 2); },
    [](vx_conv2d_args& a) { a.in_pitch = 0x7ffffffc; }, [](vx_conv2d_args& a) { a.in_pitch = a.Cin; },
    [](vx_conv2d_args& a) { a.out_pitch = wrap((int64_t)a.Cout + 2); }, [](vx_conv2d_args& a) { a.out_pitch = 0x7ffffffc; }, [](vx_conv2d_args& a) { a.out_coff = 0x7ffffffc; },
    [](vx_conv2d_args& a) { a.out_coff = 4; a.out_pitch = wrap((int64_t)a.out_pitch + 4); }, [](vx_conv2d_args& a) { a.out_coff = 2; a.out_pitch = wrap((int64_t)a.out_pitch + 4); }, [](vx_conv2d_args& a) { a.out_pitch = wrap((int64_t)a.out_pitch - 4); },
    [](vx_conv2d_args& a) { a.in_scale = P<float>(0x90000); }, [](vx_conv2d_args& a) { a.in_shift = P<float>(0xa0000); },
    [](vx_conv2d_args& a) { a.in_scale = P<float>(0x90000); a.in_shift = P<float>(0xa0000); a.in_cpitch = a.Cin; a.in_relu = 1; },
    [](vx_conv2d_args& a) { a.in_scale = P<float>(0x90000); a.in_shift = P<float>(0xa0000); a.in_cpitch = wrap((int64_t)a.Cin - 15); },
    [](vx_conv2d_args& a) { a.in_scale = P<float>(0x90000); a.in_shift = P<float>(0xa0000); a.in_cpitch = wrap((int64_t)a.Cin - 16); },
    [](vx_conv2d_args& a) { a.in_scale = P<float>(0x90000); a.in_shift = P<float>(0xa0000); a.in_cpitch = a.Cin; a.in_group_images = -1; },
    [](vx_conv2d_args& a) { a.in_scale = P<float>(0x90000); a.in_shift = P<float>(0xa0000); a.in_cpitch = a.Cin; a.in_group_images = 0x7fffffff; },
    [](vx_conv2d_args& a) { a.out_scale = P<float>(0x60000); }, [](vx_conv2d_args& a) { a.out_shift = P<float>(0x70000); },
    [](vx_conv2d_args& a) { a.out_scale = P<float>(0x60000); a.out_shift = P<float>(0x70000); },
    [](vx_conv2d_args& a) { a.out_scale = P<float>(0x60000); a.out_shift = P<float>(0x70000); a.stats_partial = nullptr; },
    [](vx_conv2d_args& a) { a.stats_partial = nullptr; }, [](vx_conv2d_args& a) { a.stats_partial = P<float>(0x50000); },
    [](vx_conv2d_args& a) { a.out_add = P<float>(0x80000); a.out_add_pitch = r4(a.Cout); }, [](vx_conv2d_args& a) { a.out_add = P<float>(0x80004); a.out_add_pitch = r4(a.Cout); },
    [](vx_conv2d_args& a) { a.out_add = P<float>(0x80000); a.out_add_pitch = wrap((int64_t)r4(a.Cout) - 4); }, [](vx_conv2d_args& a) { a.out_add = P<float>(0x80000); a.out_add_pitch = wrap((int64_t)r4(a.Cout) + 2); },
    [](vx_conv2d_args& a) { a.out_add = P<float>(0x80000); a.out_add_pitch = 0x7ffffffc; }, [](vx_conv2d_args& a) { a.out_add = nullptr; a.out_add_pitch = 0; },
    [](vx_conv2d_args& a) { a.out_act = VX_ACT_RELU; }, [](vx_conv2d_args& a) { a.out_act = VX_ACT_NONE; }, [](vx_conv2d_args& a) { a.out_act = VX_ACT_LRELU; }, [](vx_conv2d_args& a) { a.out_act = -1; },
  };
  // (H, W, real Cin, Cout, KS, S, epilogue)
  const int layers[][7] = {{20, 33, 3, 64, 3, 2, 0},  {20, 33, 18, 18, 3, 1, 0},  {17, 31, 18, 36, 3, 2, 1},  {17, 21, 32, 32, 3, 1, 1}, {20, 33, 48, 48, 3, 1, 0},
                           {9, 35, 80, 48, 3, 1, 0},  {20, 33, 64, 16, 3, 1, 1},  {9, 21, 256, 72, 1, 1, 0},  {9, 21, 720, 72, 1, 1, 1}, {5, 7, 64, 16, 1, 1, 0},
                           {112, 112, 16, 16, 3, 1, 0}, {1, 1, 270, 270, 1, 1, 1}};
  const int nm = (int)mods.size();
  for (const vx_config& cfg : cfgs)
    for (const auto& L : layers)
      for (int i = -1; i < nm; ++i) for (int j = i; j < nm; ++j) {
        if (i >= 0 && j == i) continue;
        vx_conv2d_args x = layer(2, L[0], L[1], L[2], L[3], L[4], L[5], L[6] != 0, cfg);
        if (i >= 0) mods[i](x);
        if (j >= 0) mods[j](x);
        walk(x, cfg);
      }
  printf("routes %lld taken %lld unsound %lld checksum %016llx\n", g_routes, g_taken, g_unsound, g_sum);

  // ---- 1c. every instance of the two lists was named by an accepted route ----
  int listed = 0, missing = 0;
  Conv2dRoute r;
  auto seen = [&](int kernel, int a, int b, int c, int d, int e, int f, int g) {
    const int p[7] = {a, b, c, d, e, f, g};
    char name[128];
    r.kernel = kernel;
    for (int i = 0; i < 7; ++i) r.p[i] = p[i];
    conv2d_route_name(r, name, sizeof name);
    ++listed;
    if (!g_named.count(name)) { ++missing; printf("never routed: %s\n", name); }
  };
#define SEEN_C2(KS, S, NT, NSUB, TY) seen(CONV2D_MFMA, KS, S, NT, NSUB, TY, 0, 0);
#define SEEN_C2S(KS, S, NT, NSUB, TY, OCT, EPI) seen(CONV2D_S16, KS, S, NT, NSUB, TY, OCT, EPI);
  C2_INSTANCES(SEEN_C2)
  C2S_INSTANCES(SEEN_C2S)
  printf("instances listed %d named %d missing %d\n", listed, (int)g_named.size(), missing);

  // ---- 2. the cases on stdin ----
  char id[128];
  int KS, S, H, W, Cin, Cout, N, epi, no_wide, no_oct, fp32;
  while (scanf("%127s %d %d %d %d %d %d %d %d %d %d %d", id, &KS, &S, &H, &W, &Cin, &Cout, &N, &epi, &no_wide, &no_oct, &fp32) == 12) {
    vx_config cfg = def;
    cfg.c2s_no_wide = no_wide; cfg.c2s_no_oct = no_oct; cfg.conv_fp32 = fp32;
    const vx_conv2d_args x = layer(N, H, W, Cin, Cout, KS, S, epi != 0, cfg);
    memset(&r, 0, sizeof r);
    const int rc = conv2d_route(x, cfg, &r);
    char name[128] = "-";
    if (rc == VX_OK) conv2d_route_name(r, name, sizeof name);
    printf("case %s %d %s %d %d %d %d\n", id, rc, name, r.nchunks, r.w_all, r.grid_x, r.grid_y);
  }
  return (g_unsound || missing || (int)g_named.size() != listed) ? 1 : 0;
}
