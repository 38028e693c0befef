// Stand-alone host program over values_amd/csrc/conv3d_route.h (the routing of vx_conv3d_k3: a pure function of its arguments),
// built with -fsanitize=address,undefined by tests/test_conv3d_route_cpu.py.  No GPU, no library, nothing loaded into Python.
//   1. walks every rule, query and the route itself over grids of configurations, shapes, channels and flag pairs -- zero and
//      negative dimensions, dimensions and pitches large enough to trip every 32-bit guard -- and prints what it counted;
//   2. routes the dense single-layer cases given on stdin ("id D H W Cin Cout N epilogue conv_fp32") and prints "id rc kernel".
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../values_amd/csrc/conv3d_route.h"

template <typename T>
static T* P(uintptr_t v) { return (T*)v; }

static vx_conv3d_args dense(int N, int D, int H, int W, int Cin, int Cout, const vx_config& cfg) {
  vx_conv3d_args a;
  memset(&a, 0, sizeof a);
  a.in = P<float>(0x10000); a.w_packed = P<float>(0x20000); a.bias = P<float>(0x30000); a.out = P<float>(0x40000);
  a.N = N; a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.in_pitch = Cin; a.out_pitch = Cout;
  a.w_family = conv3d_family(Cin, Cout, cfg);
  return a;
}

static unsigned long long g_sum = 0;
static void mix(long long v) { g_sum = g_sum * 1099511628211ull + (unsigned long long)v; }

// a successful route must name an instance that exists and carry a usable geometry
static bool route_is_sound(const Conv3dRoute& r) {
  if (r.kernel < 0 || r.kernel >= CONV3D_NKERNELS || !conv3d_instance_exists(r.kernel, r.p, r.np)) return false;
  if (r.tiles_x < 1 || r.tiles_y < 1 || r.tiles_z < 1) return false;
  if ((r.kernel == CONV3D_XP8W || r.kernel == CONV3D_ZC16 || r.kernel == CONV3D_DEEP) && r.nitems < 1) return false;
  char name[128];
  const int n = conv3d_route_name(r, name, sizeof name);
  return n > 0 && n < (int)sizeof name;
}

int main() {
  vx_config def;
  memset(&def, 0, sizeof def);
  def.s16_skip_raw = 1;
  std::vector<vx_config> cfgs(9, def);
  cfgs[1].conv_fp32 = 1; cfgs[2].conv_fp32 = 2; cfgs[3].s16_no_xp8 = 1; cfgs[4].s16_no_zc16 = 1; cfgs[5].s16_no_deep = 1;
  cfgs[6].s16_no_upfuse = 1; cfgs[7].s16_no_poolfuse = 1; cfgs[8].s16_generic = 1;
  const int dims[] = {-7, 0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 40, 64, 96, 128, 1 << 20, 0x7fffffff};
  const int chans[] = {-8, 0, 3, 8, 16, 24, 32, 64, 128, 256, 512};
  const int nd = sizeof dims / sizeof *dims, nc = sizeof chans / sizeof *chans;

  // ---- 1a. the queries ----
  long long points = 0;
  for (const vx_config& cfg : cfgs)
    for (int a = 0; a < nd; ++a) for (int b = 0; b < nd; ++b) for (int c = 0; c < nd; ++c) {
      const int D = dims[a], H = dims[b], W = dims[c];
      mix(conv3d_tiles_max(D, H, W));
      for (int i = 0; i < nc; ++i) for (int o = 0; o < nc; ++o) {
        if ((a + 2 * b + 3 * c + i + o) % 3) continue;     // (a third of the grid)
        const int Cin = chans[i], Cout = chans[o];
        ++points;
        mix(conv3d_prologue_ok(D, H, W, Cin, Cout, cfg)); mix(conv3d_upfuse_ok(D, H, W, Cin, Cout, cfg));
        mix(conv3d_pool_layout(D, H, W, Cin, Cout, cfg)); mix(conv3d_presplit_ok(D, H, W, Cin, Cout, cfg));
        mix(conv3d_zc16_16to16(D, H, W, Cin, Cout, cfg));
        for (int xb = 0; xb <= 4; ++xb) mix(conv3d_skip_prologue_ok(D, H, W, Cin, Cout, xb, cfg));
        if (a == 0 && b == 0) {
          mix(conv3d_poolfin_ok(Cin, Cout, cfg)); mix(conv3d_head_fusable(Cin, Cout, cfg)); mix(conv3d_family(Cin, Cout, cfg));
          mix(conv3d_packed_floats(Cin, Cout, cfg));
        }
        if (i == 0) mix(conv3d_tiles_for(D, H, W, Cout, cfg));
      }
    }
  printf("queries %lld points\n", points);

  // ---- 1b. the route: dense launches over the whole grid, then single flags and flag pairs over a handful of layers ----
  long long routes = 0, taken = 0, unsound = 0;
  Conv3dRoute r;
  for (const vx_config& cfg : cfgs)
    for (int a = 0; a < nd; ++a) for (int b = 0; b < nd; ++b) for (int c = 0; c < nd; ++c)
      for (int i = 0; i < nc; ++i) for (int o = 0; o < nc; ++o) {
          if ((a + 2 * b + 3 * c + i + o) % 5) continue;   // (a fifth of the grid: every value of every axis still meets every other)
          const int Ns[3] = {1, 3, 0x7fffffff};
          vx_conv3d_args x = dense(Ns[(a + b + c + i) % 3], dims[a], dims[b], dims[c], chans[i], chans[o], cfg);
          if ((a + b + c + i + o) % 3 == 0) x.stats_partial = P<float>(0x50000);
          const int rc = conv3d_route(x, cfg, &r);
          ++routes; mix(rc);
          if (rc == VX_OK) { ++taken; unsound += !route_is_sound(r); mix(r.kernel); mix((long long)conv3d_key_of(r.p, r.np)); }
        }
  typedef std::function<void(vx_conv3d_args&)> Mod;
  const std::vector<Mod> mods = {
    [](vx_conv3d_args& a) { a.in_planar = 1; }, [](vx_conv3d_args& a) { a.out_planar = 1; },
    [](vx_conv3d_args& a) { a.products = 1; }, [](vx_conv3d_args& a) { a.products = 2; },
    [](vx_conv3d_args& a) { a.up_in = P<float>(0x60000); a.up_w = P<float>(0x61000); a.up_b = P<float>(0x62000); a.up_pitch = 16; },
    [](vx_conv3d_args& a) { a.up_in = P<float>(0x60000); a.up_w = P<float>(0x61000); a.up_b = P<float>(0x62000); a.up_pitch = 32; },
    [](vx_conv3d_args& a) { a.up_in = P<float>(0x60000); a.up_w = P<float>(0x61000); a.up_b = P<float>(0x62000); a.up_pitch = 0x7ffffffc; },
    [](vx_conv3d_args& a) { a.up_in = P<float>(0x60004); a.up_w = P<float>(0x61000); a.up_b = P<float>(0x62000); a.up_pitch = 16; },
    [](vx_conv3d_args& a) { a.up_fused = P<float>(0x63000); }, [](vx_conv3d_args& a) { a.up_split = 1; },
    [](vx_conv3d_args& a) { a.pool_out = P<float>(0x64000); a.pool_flags = P<uint32_t>(0x65000); }, [](vx_conv3d_args& a) { a.pool_out = P<float>(0x64000); },
    [](vx_conv3d_args& a) { a.stats_partial = P<float>(0x50000); }, [](vx_conv3d_args& a) { a.in_pool_flags = P<uint32_t>(0x66000); },
    [](vx_conv3d_args& a) { a.in_mean = P<float>(0x67000); a.in_rstd = P<float>(0x68000); }, [](vx_conv3d_args& a) { a.in_mean = P<float>(0x67000); },
    [](vx_conv3d_args& a) { a.in_split = 1; }, [](vx_conv3d_args& a) { a.in_f16 = 1; }, [](vx_conv3d_args& a) { a.out_f16 = 1; },
    [](vx_conv3d_args& a) { a.out_split = 1; },
    [](vx_conv3d_args& a) { a.acc_in = P<float>(0x69000); a.acc_pitch = 16; }, [](vx_conv3d_args& a) { a.acc_in = P<float>(0x69000); a.acc_pitch = 0x7ffffffc; },
    [](vx_conv3d_args& a) { a.in_xblk = 1; }, [](vx_conv3d_args& a) { a.in_xblk = 2; }, [](vx_conv3d_args& a) { a.in_xblk = 4; }, [](vx_conv3d_args& a) { a.in_xblk = 3; },
    [](vx_conv3d_args& a) { a.out_xblk = 2; a.out_half = 1; }, [](vx_conv3d_args& a) { a.out_xblk = 3; },
    [](vx_conv3d_args& a) { a.head_out = P<float>(0x6a000); a.head_w = P<float>(0x6b000); a.head_b = P<float>(0x6c000); a.head_C = 1; },
    [](vx_conv3d_args& a) { a.head_out = P<float>(0x6a000); a.head_w = P<float>(0x6b000); a.head_b = P<float>(0x6c000); a.head_C = 4; a.out = nullptr; },
    [](vx_conv3d_args& a) { a.head_out = P<float>(0x6a000); a.head_w = P<float>(0x6b000); a.head_b = P<float>(0x6c000); a.head_C = 5; },
    [](vx_conv3d_args& a) { a.head_out = P<float>(0x6a000); a.head_w = P<float>(0x6b000); a.head_b = P<float>(0x6c000); a.head_C = 9; },
    [](vx_conv3d_args& a) { a.act = 1; }, [](vx_conv3d_args& a) { a.act = 2; }, [](vx_conv3d_args& a) { a.act = 3; }, [](vx_conv3d_args& a) { a.act = -1; },
    [](vx_conv3d_args& a) { a.drop_mode = VX_DROP_HASH; }, [](vx_conv3d_args& a) { a.drop_mode = VX_DROP_MASK; a.drop_mask = P<uint8_t>(0x6d000); },
    [](vx_conv3d_args& a) { a.drop_mode = VX_DROP_MASK; }, [](vx_conv3d_args& a) { a.drop_mode = 3; },
    [](vx_conv3d_args& a) { a.in_drop_mode = VX_DROP_HASH; }, [](vx_conv3d_args& a) { a.in_drop_mode = VX_DROP_MASK; },
    [](vx_conv3d_args& a) { a.in_repeat = 2; }, [](vx_conv3d_args& a) { a.in_repeat = 0x7fffffff; },
    [](vx_conv3d_args& a) { a.in_pitch = a.Cin - 4; }, [](vx_conv3d_args& a) { a.in_pitch = a.Cin + 2; }, [](vx_conv3d_args& a) { a.in_pitch = 0x7ffffffc; },
    [](vx_conv3d_args& a) { a.out_pitch = a.Cout + 2; }, [](vx_conv3d_args& a) { a.out_pitch = 0x7ffffffc; }, [](vx_conv3d_args& a) { a.out_coff = 0x7ffffffc; },
    [](vx_conv3d_args& a) { a.out_coff = 4; a.out_pitch = a.Cout + 4; },
    [](vx_conv3d_args& a) { a.in = P<float>(0x10004); }, [](vx_conv3d_args& a) { a.out = P<float>(0x40008); }, [](vx_conv3d_args& a) { a.in = nullptr; },
    [](vx_conv3d_args& a) { a.N = 0x7fffffff; }, [](vx_conv3d_args& a) { a.N = 0; }, [](vx_conv3d_args& a) { a.N = -1; },
    [](vx_conv3d_args& a) { a.D = 0; }, [](vx_conv3d_args& a) { a.W = -1; }, [](vx_conv3d_args& a) { a.D = 0x7ffffffc; }, [](vx_conv3d_args& a) { a.W = 0x7fffffe0; },
    [](vx_conv3d_args& a) { a.Cin = 0; }, [](vx_conv3d_args& a) { a.Cin = 12; }, [](vx_conv3d_args& a) { a.Cout = -8; }, [](vx_conv3d_args& a) { a.w_family = 0; },
  };
  const int layers[][5] = {{64, 64, 64, 8, 8}, {64, 64, 64, 16, 8}, {32, 32, 32, 8, 16}, {32, 32, 32, 16, 16}, {16, 16, 16, 16, 32}, {8, 8, 8, 64, 64},
                           {6, 8, 8, 32, 32}, {5, 7, 9, 32, 16}, {5, 7, 9, 24, 8}, {32, 32, 32, 64, 32}, {2, 2, 2, 32, 32}, {64, 64, 64, 8, 24}};
  const int nm = (int)mods.size();
  for (const vx_config& cfg : cfgs)
    for (const auto& L : layers)
      for (int i = -1; i < nm; ++i) for (int j = i; j < nm; ++j) {
        if (i >= 0 && j == i) continue;
        vx_conv3d_args x = dense(2, L[0], L[1], L[2], L[3], L[4], cfg);
        if (i >= 0) mods[i](x);
        if (j >= 0) mods[j](x);
        const int rc = conv3d_route(x, cfg, &r);
        ++routes; mix(rc);
        if (rc == VX_OK) { ++taken; unsound += !route_is_sound(r); mix(r.kernel); mix((long long)conv3d_key_of(r.p, r.np)); }
        else if (rc > 0 || !r.err[0]) ++unsound;   // a refusal is a VX_E_* code with a message
      }
  printf("routes %lld taken %lld unsound %lld checksum %016llx\n", routes, taken, unsound, g_sum);

  // ---- 2. the cases on stdin ----
  char id[128], epi[32];
  int D, H, W, Cin, Cout, N, fp32;
  while (scanf("%127s %d %d %d %d %d %d %31s %d", id, &D, &H, &W, &Cin, &Cout, &N, epi, &fp32) == 9) {
    vx_config cfg = def;
    cfg.conv_fp32 = fp32;
    vx_conv3d_args x = dense(N, D, H, W, Cin, Cout, cfg);
    x.range_flag = P<uint32_t>(0x70000);
    if (!strcmp(epi, "stats")) x.stats_partial = P<float>(0x50000);
    else {
      x.act = VX_ACT_LRELU;
      if (!strcmp(epi, "lrelu_hash")) { x.drop_mode = VX_DROP_HASH; x.drop_seed = 77; x.drop_layer = 3; }
      if (!strcmp(epi, "lrelu_mask")) { x.drop_mode = VX_DROP_MASK; x.drop_mask = P<uint8_t>(0x6d000); }
    }
    const int rc = conv3d_route(x, cfg, &r);
    char name[128] = "-";
    if (rc == VX_OK) conv3d_route_name(r, name, sizeof name);
    printf("case %s %d %s\n", id, rc, name);
  }
  return unsound ? 1 : 0;
}
