// Stand-alone host program over values_amd/csrc/stream3d_route.h (the routing of the 3D streaming passes: pure functions of their
// arguments), built with -fsanitize=address,undefined by tests/test_stream3d_route_cpu.py.  No GPU, no library, nothing loaded into
// Python.  Walks every pass's route over grids of its arguments -- zero and negative values, sizes large enough to trip every 32-bit,
// 64-bit and 2^32-decode guard -- and over single fields and field pairs of a handful of good layers; counts as unsound a refusal
// without a message and an accepted route that breaks a condition the kernels rely on (restated here on the descriptor); prints what
// it counted, and how many instances of the list an accepted route named.
#include <stdio.h>
#include <string.h>

#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../values_amd/csrc/stream3d_route.h"

template <typename T>
static T* P(uintptr_t v) { return (T*)v; }
static int wrap(int64_t v) { return (int)(uint32_t)(uint64_t)v; }      // (a sum on a field that already holds an extreme value)

static vx_norm_args layer(int N, int D, int H, int W, int C, bool pool) {
  vx_norm_args a;
  memset(&a, 0, sizeof a);
  a.x = P<float>(0x10000); a.mean = P<float>(0x20000); a.rstd = P<float>(0x30000); a.out = P<float>(0x40000);
  a.N = N; a.D = D; a.H = H; a.W = W; a.C = C;
  a.x_pitch = C; a.out_pitch = C;
  if (pool) { a.pool_out = P<float>(0x50000); a.pool_pitch = C; }
  a.act = VX_ACT_LRELU;
  return a;
}
static vx_stat_src source() {
  vx_stat_src s;
  memset(&s, 0, sizeof s);
  s.stats_partial = P<float>(0x70000); s.tiles = 5; s.eps = 1e-5f; s.count = 100;
  return s;
}

static unsigned long long g_sum = 0;
static void mix(long long v) { g_sum = g_sum * 1099511628211ull + (unsigned long long)v; }
static std::set<std::string> g_named;      // kernels accepted routes named
static long long g_routes = 0, g_taken = 0, g_unsound = 0;

static const vx_wide TWO32 = (vx_wide)1 << 32, TWO31 = (vx_wide)1 << 31;
static bool magic_exact(unsigned m, unsigned i, int d) { return (m ? (unsigned)(((uint64_t)i * m) >> 32) : i) == i / (unsigned)d && (m != 0 || d == 1); }
static vx_wide ceil_div(vx_wide a, vx_wide b) { return (a + b - 1) / b; }

static bool name_ok(const Stream3dRoute& r) {
  char name[96];
  const int n = stream3d_route_name(r, name, sizeof name);
  if (n <= 0 || n >= (int)sizeof name) return false;
  g_named.insert(name);
  return true;
}

// what norm_act_drop_pool_kernel / norm_act_drop_fanout_kernel rely on, restated from the arguments
static bool norm_is_sound(const Stream3dRoute& r, const vx_norm_args& a, int x_repeat, const vx_stat_src* st) {
  const bool pool = a.pool_out != nullptr;
  if (r.kernel != S3_NORM && r.kernel != S3_FANOUT) return false;
  if (r.kernel == S3_NORM && !stream3d_norm_instance_exists(r.pool, r.wide, r.fold)) return false;
  if ((r.kernel == S3_FANOUT) != (!pool && x_repeat > 1)) return false;
  if (a.C < 4 || a.C % 4 || a.N < 1 || a.D < 1 || a.H < 1 || a.W < 1 || x_repeat < 1) return false;
  if ((vx_wide)a.D * a.H * a.W * a.C >= TWO32) return false;
  const bool wide = pool && a.C > 128;
  if (pool && (a.D % 2 || a.H % 2 || a.W % 2 || (!wide && 32 % (a.C / 4)))) return false;
  if (r.kernel == S3_NORM && (r.pool != pool || r.wide != wide || r.fold != (st != nullptr))) return false;
  if (st && (x_repeat != 1 || a.C > VX_STAT_MAXC || a.mean || a.rstd)) return false;
  const vx_wide C4 = a.C / 4, PW = (wide ? a.W / 2 : a.W) * C4, RH = pool ? a.H / 2 : a.H, RD = pool ? a.D / 2 : a.D, per = RD * RH * PW;
  if (per < 1 || r.pieces != per || per * (PW > RH ? PW : RH) >= TWO32) return false;
  const unsigned last = (unsigned)(per - 1);
  if (!magic_exact(r.mPW, last, (int)PW) || !magic_exact(r.mC4, last, (int)C4) || !magic_exact(r.mH, last, (int)RH)) return false;
  const int samples = r.kernel == S3_FANOUT ? a.N / x_repeat : a.N;
  if (r.kernel == S3_FANOUT && a.N % x_repeat) return false;
  if (r.grid_y != samples || r.grid_y < 1 || r.grid_y > 65535) return false;
  if ((vx_wide)samples * a.D >= TWO31 || (r.kernel == S3_NORM && (vx_wide)a.N * a.D >= TWO31)) return false;
  if ((a.x_xblk || (a.out && a.out_xblk)) && (vx_wide)2 * a.W * a.C >= TWO31) return false;   // (follows from the decode bound)
  vx_wide cap = ceil_div(per, 256);
  if (r.kernel == S3_FANOUT && ceil_div(32768, samples) < cap) cap = ceil_div(32768, samples);
  if (r.kernel == S3_NORM && !pool && ceil_div(16384, samples) < cap) cap = ceil_div(16384, samples);
  if (st) cap = (cap + 3) / 4;
  if (r.grid_x < 1 || r.grid_x != cap) return false;
  if (a.out && !a.out_xblk && (int64_t)a.out_coff + a.C > a.out_pitch) return false;
  return name_ok(r);
}

static void count(int rc, const Stream3dRoute& r, bool sound) {
  ++g_routes; mix(rc);
  if (rc == VX_OK) { ++g_taken; g_unsound += !sound; mix(r.kernel); mix(stream3d_key(r.pool, r.wide, r.fold)); mix(r.grid_x); mix(r.grid_y); mix(r.pieces); }
  else if (rc > 0 || !r.err[0]) ++g_unsound;   // a refusal is a VX_E_* code with a message
}
static void walk_norm(const vx_norm_args& a, int x_repeat, const vx_stat_src* st) {
  Stream3dRoute r;
  const int rc = stream3d_norm_route(a, x_repeat, st, &r);
  count(rc, r, rc == VX_OK && norm_is_sound(r, a, x_repeat, st));
}
// the small passes: grid_x within its cap, grid_y = N in 1..65535, pieces the 128-bit product
static bool small_is_sound(const Stream3dRoute& r, int N, vx_wide pieces, int cap) {
  if (pieces < 1 || pieces >= TWO31 || r.pieces != pieces || r.grid_y != N || N < 1 || N > 65535) return false;
  const vx_wide bx = ceil_div(pieces, 256);
  return r.grid_x >= 1 && r.grid_x == (bx > cap ? cap : bx) && name_ok(r);
}

int main() {
  const int dims[] = {-7, 0, 1, 2, 3, 6, 64, 65536, 1 << 20, 0x7fffffff};
  const int chans[] = {-4, 0, 4, 6, 8, 12, 16, 128, 132, 512, 516, 1 << 20, 0x7ffffffc};
  const int Ns[] = {-1, 0, 1, 3, 6, 65535, 65536, 131070, 0x7fffffff};
  const int reps[] = {1, 2, 3};
  const vx_stat_src src = source();

  // ---- 1. vx_norm_act_drop_pool and its forms: dense launches over the whole grid ----
  for (int n : Ns) for (int d : dims) for (int h : dims) for (int w : dims) for (int c : chans) for (int pool = 0; pool < 2; ++pool) {
    for (int rep : reps) walk_norm(layer(n, d, h, w, c, pool), rep, nullptr);
    vx_norm_args a = layer(n, d, h, w, c, pool);
    a.mean = a.rstd = nullptr;
    walk_norm(a, 1, &src);
  }
  // ... then single fields and field pairs over a handful of layers
  typedef std::function<void(vx_norm_args&)> Mod;
  const std::vector<Mod> mods = {
    [](vx_norm_args& a) { a.x = nullptr; }, [](vx_norm_args& a) { a.out = nullptr; }, [](vx_norm_args& a) { a.pool_out = nullptr; }, [](vx_norm_args& a) { a.mean = nullptr; },
    [](vx_norm_args& a) { a.mean = a.rstd = nullptr; }, [](vx_norm_args& a) { a.pool_out = P<float>(0x50000); a.pool_pitch = a.C; },
    [](vx_norm_args& a) { a.range_flag = P<uint32_t>(0x60000); },
    [](vx_norm_args& a) { a.N = 0; }, [](vx_norm_args& a) { a.N = -1; }, [](vx_norm_args& a) { a.N = 4; }, [](vx_norm_args& a) { a.N = 65535; }, [](vx_norm_args& a) { a.N = 65536; },
    [](vx_norm_args& a) { a.N = 131070; }, [](vx_norm_args& a) { a.N = 1 << 20; }, [](vx_norm_args& a) { a.N = 0x7fffffff; },
    [](vx_norm_args& a) { a.D = 0; }, [](vx_norm_args& a) { a.D = 1; }, [](vx_norm_args& a) { a.D = 3; }, [](vx_norm_args& a) { a.D = 1 << 16; }, [](vx_norm_args& a) { a.D = 1 << 20; },
    [](vx_norm_args& a) { a.D = 0x7fffffff; }, [](vx_norm_args& a) { a.H = -7; }, [](vx_norm_args& a) { a.H = 5; }, [](vx_norm_args& a) { a.H = 65536; }, [](vx_norm_args& a) { a.H = 0x7fffffff; },
    [](vx_norm_args& a) { a.W = 0; }, [](vx_norm_args& a) { a.W = 3; }, [](vx_norm_args& a) { a.W = 65536; }, [](vx_norm_args& a) { a.W = 1 << 27; }, [](vx_norm_args& a) { a.W = 1 << 28; },
    [](vx_norm_args& a) { a.W = 0x7ffffffe; },
    [](vx_norm_args& a) { a.C = 0; }, [](vx_norm_args& a) { a.C = -4; }, [](vx_norm_args& a) { a.C = 6; }, [](vx_norm_args& a) { a.C = 12; a.x_pitch = a.out_pitch = a.pool_pitch = 12; },
    [](vx_norm_args& a) { a.C = 4; }, [](vx_norm_args& a) { a.C = 132; a.x_pitch = a.out_pitch = a.pool_pitch = 132; }, [](vx_norm_args& a) { a.C = 516; a.x_pitch = a.out_pitch = a.pool_pitch = 516; },
    [](vx_norm_args& a) { a.C = 0x7ffffffc; a.x_pitch = a.out_pitch = a.pool_pitch = 0x7ffffffc; },
    [](vx_norm_args& a) { a.x_pitch = 0; }, [](vx_norm_args& a) { a.x_pitch = wrap((int64_t)a.C + 2); }, [](vx_norm_args& a) { a.x_pitch = wrap((int64_t)a.C + 4); }, [](vx_norm_args& a) { a.x_pitch = 0x7ffffffc; },
    [](vx_norm_args& a) { a.out_pitch = 0; }, [](vx_norm_args& a) { a.out_pitch = wrap((int64_t)a.C + 2); }, [](vx_norm_args& a) { a.out_pitch = 0x7ffffffc; },
    [](vx_norm_args& a) { a.out_coff = 4; a.out_pitch = wrap((int64_t)a.out_pitch + 4); }, [](vx_norm_args& a) { a.out_coff = 2; }, [](vx_norm_args& a) { a.out_coff = 4; },
    [](vx_norm_args& a) { a.out_coff = -4; }, [](vx_norm_args& a) { a.out_coff = 0x7ffffffc; }, [](vx_norm_args& a) { a.out_coff = (int)0x80000000; },
    [](vx_norm_args& a) { a.pool_pitch = 0; }, [](vx_norm_args& a) { a.pool_pitch = wrap((int64_t)a.C + 8); }, [](vx_norm_args& a) { a.pool_pitch = 6; },
    [](vx_norm_args& a) { a.out_xblk = 1; }, [](vx_norm_args& a) { a.out_xblk = 2; }, [](vx_norm_args& a) { a.out_xblk = 3; }, [](vx_norm_args& a) { a.out_xblk = 4; }, [](vx_norm_args& a) { a.out_xblk = -1; },
    [](vx_norm_args& a) { a.out_xblk = (int)0x80000000; }, [](vx_norm_args& a) { a.out_half = 1; }, [](vx_norm_args& a) { a.out_half = 2; }, [](vx_norm_args& a) { a.out_half = -1; },
    [](vx_norm_args& a) { a.x_xblk = 1; }, [](vx_norm_args& a) { a.x_xblk = 2; }, [](vx_norm_args& a) { a.x_xblk = 3; }, [](vx_norm_args& a) { a.x_xblk = 4; }, [](vx_norm_args& a) { a.x_xblk = (int)0x80000000; },
    [](vx_norm_args& a) { a.x_half = 1; }, [](vx_norm_args& a) { a.x_half = 2; },
    [](vx_norm_args& a) { a.act = VX_ACT_RELU; }, [](vx_norm_args& a) { a.act = 7; }, [](vx_norm_args& a) { a.drop_mode = VX_DROP_HASH; }, [](vx_norm_args& a) { a.drop_mode = VX_DROP_MASK; },
    [](vx_norm_args& a) { a.drop_mode = VX_DROP_MASK; a.drop_mask = P<uint8_t>(0x80000); },
  };
  // (N, D, H, W, C, pooling)
  const int layers[][6] = {{2, 4, 4, 4, 8, 0}, {2, 4, 4, 4, 8, 1}, {3, 3, 5, 7, 12, 0}, {2, 2, 6, 10, 128, 1}, {2, 2, 2, 4, 256, 1}, {6, 1, 1, 21, 16, 0},
                           {1, 72, 57, 341, 12, 0}, {1, 73, 57, 341, 12, 0}, {65535, 1, 1, 1, 4, 0}, {20000, 2, 3, 50, 8, 0}, {66000, 1, 1, 70, 16, 0}};
  const int nm = (int)mods.size();
  for (const auto& L : layers)
    for (int form = 0; form < 4; ++form)          // plain, _bcast 2, _bcast 3, _stats
      for (int i = -1; i < nm; ++i) for (int j = i; j < nm; ++j) {
        if (i >= 0 && j == i) continue;
        vx_norm_args a = layer(L[0], L[1], L[2], L[3], L[4], L[5]);
        if (form == 3) a.mean = a.rstd = nullptr;
        if (i >= 0) mods[i](a);
        if (j >= 0) mods[j](a);
        walk_norm(a, form == 1 ? 2 : form == 2 ? 3 : 1, form == 3 ? &src : nullptr);
      }
  // the statistics source's own fields, through the pass that checks it first
  for (int tiles : {-1, 0, 1, 0x7fffffff}) for (int64_t cnt : {(int64_t)-1, (int64_t)0, (int64_t)1, INT64_MAX}) for (int c : {8, 512, 516}) for (int nul = 0; nul < 2; ++nul) {
    vx_stat_src s = src;
    s.tiles = tiles; s.count = cnt;
    if (nul) s.stats_partial = nullptr;
    vx_norm_args a = layer(2, 2, 2, 2, c, 0);
    a.mean = a.rstd = nullptr;
    walk_norm(a, 1, &s);
  }
  const long long norm_routes = g_routes;

  // ---- 2. the small passes ----
  Stream3dRoute r;
  const void* good = P<float>(0x10000);
  const void* ptrs[] = {nullptr, good, P<float>(0x10004)};
  const int sN[] = {-1, 0, 1, 3, 65535, 65536, 1 << 20, 0x7fffffff};
  const int64_t big[] = {-1, 0, 1, 5, 127, 128, 129, 16385, 70001, (1ll << 26), (1ll << 28) - 1, 1ll << 28, (1ll << 30) - 1, 1ll << 30, 1ll << 31, (1ll << 32) - 4, 1ll << 32,
                         1ll << 33, 1ll << 61, 1ll << 62, INT64_MAX};
  // vx_instnorm_finalize
  for (int n : sN) for (int c : chans) for (int t : {0, 1, 37}) for (int64_t v : {(int64_t)0, (int64_t)1, INT64_MAX}) for (const void* p : ptrs) {
    const int rc = stream3d_finalize_route(p, n, t, c, v, good, p ? good : nullptr, &r);
    count(rc, r, rc == VX_OK && r.grid_y == 1 && r.grid_x >= 1 && (vx_wide)r.grid_x == (vx_wide)n * c && name_ok(r));
  }
  // vx_prenorm_split(_stats), vx_pool_finish
  for (int n : sN) for (int64_t v : big) for (const void* p : ptrs) for (const void* q : ptrs) for (int fold = 0; fold < 2; ++fold) for (int nost = 0; nost < 2; ++nost) {
    int rc = stream3d_split_route(fold ? "vx_prenorm_split_stats" : "vx_prenorm_split", p, q, good, fold, nost ? nullptr : &src, n, v, &r);
    count(rc, r, rc == VX_OK && r.fold == fold && (fold ? !nost : q != nullptr) && vx_aligned16(p) && small_is_sound(r, n, (vx_wide)v * 2, fold ? 128 : 512));
    if (fold) continue;
    for (int pitch : {-8, 0, 4, 8, 10, 12, 0x7ffffffc}) {
      rc = stream3d_finish_route(p, good, good, good, q, pitch, n, v, &r);
      count(rc, r, rc == VX_OK && pitch >= 8 && pitch % 4 == 0 && vx_aligned16(p) && vx_aligned16(q) && small_is_sound(r, n, (vx_wide)v * 2, 64));
    }
  }
  // vx_pool_finish_z(_stats)
  for (int n : sN) for (int dp : dims) for (int64_t v : big) for (const void* p : ptrs) for (int pitch : {0, 12, 16, 18, 20, 0x7ffffffc}) for (int fold = 0; fold < 2; ++fold) {
    const int rc = stream3d_finish_z_route(fold ? "vx_pool_finish_z_stats" : "vx_pool_finish_z", p, good, fold ? nullptr : good, fold ? nullptr : good, fold, fold ? &src : nullptr,
                                           good, pitch, n, dp, v, &r);
    count(rc, r, rc == VX_OK && r.fold == fold && pitch >= 16 && pitch % 4 == 0 && vx_aligned16(p) && (vx_wide)dp * v < ((vx_wide)1 << 28) &&
                     small_is_sound(r, n, (vx_wide)dp * v * 4, fold ? 16 : 64));
  }
  // vx_drop_hash_mask
  for (int n : sN) for (int64_t v : big) for (const void* p : {(const void*)nullptr, good, (const void*)P<char>(0x10002), (const void*)P<char>(0x10004)}) {
    const int rc = stream3d_hash_mask_route(n, v, p, &r);
    const vx_wide bx = ceil_div((vx_wide)n * (v / 4), 256);
    count(rc, r, rc == VX_OK && n >= 1 && v >= 4 && v % 4 == 0 && v < (1ll << 32) && p && ((uintptr_t)p & 3) == 0 && r.grid_y == 1 && r.grid_x >= 1 &&
                     r.grid_x == (bx > 16384 ? 16384 : bx));
  }
  printf("routes %lld norm %lld taken %lld unsound %lld checksum %016llx\n", g_routes, norm_routes, g_taken, g_unsound, g_sum);

  // ---- 3. every instance of the list, and every other kernel that reports a name, was named by an accepted route ----
  int listed = 0, missing = 0;
  auto seen = [&](int kernel, int pool, int wide, int fold) {
    char name[96];
    r.kernel = kernel; r.pool = pool; r.wide = wide; r.fold = fold;
    stream3d_route_name(r, name, sizeof name);
    ++listed;
    if (!g_named.count(name)) { ++missing; printf("never routed: %s\n", name); }
  };
#define SEEN_NORM(P, W, F) seen(S3_NORM, P, W, F);
  STREAM3D_NORM_INSTANCES(SEEN_NORM)
  seen(S3_FANOUT, 0, 0, 0); seen(S3_FINALIZE, 0, 0, 0); seen(S3_FINISH, 0, 0, 0);
  for (int fold = 0; fold < 2; ++fold) { seen(S3_SPLIT, 0, 0, fold); seen(S3_FINISH_Z, 0, 0, fold); }
  printf("instances listed %d named %d missing %d\n", listed, (int)g_named.size(), missing);
  return (g_unsound || missing || (int)g_named.size() != listed) ? 1 : 0;
}
