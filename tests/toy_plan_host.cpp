// Stand-alone driver of values_amd/csrc/toy_plan.h, the host plan of the toy data kernels (reflect index, clipped object
// box, blur tiles, order-statistics workspace and argument checks), built under -fsanitize=address,undefined by
// tests/test_toydata_cpu.py.  The pointers are made-up addresses: the plan never dereferences them.
//   toy_plan_host  ->  "reflect <mismatches>", then one line per case: "<name> <code> <numbers>"
#include <stdio.h>

#include "../values_amd/csrc/toy_plan.h"

static void* at(uintptr_t a) { return (void*)a; }

// the extended line written out by hand: ... | a b c | c b a | a b c | ...
static int reflect_walk(int i, int n) {
  int pos = 0, dir = 1;   // walk |i| steps from index 0 over the mirrored copies
  if (i >= 0) {
    for (int s = 0; s < i; ++s) {
      if (dir == 1 && pos == n - 1) dir = -1;
      else if (dir == -1 && pos == 0) dir = 1;
      else pos += dir;
    }
  } else {
    dir = -1;   // index -1 mirrors index 0
    for (int s = 0; s < -i - 1; ++s) {
      if (dir == -1 && pos == n - 1) dir = 1;
      else if (dir == 1 && pos == 0) dir = -1;
      else pos -= dir;
    }
  }
  return pos;
}

static void embed_case(const char* name, const void* obj, const void* img, int o0, int o1, int o2, int f0, int f1, int f2, int d0, int d1, int d2) {
  const int32_t od[3] = {o0, o1, o2}, off[3] = {f0, f1, f2}, d[3] = {d0, d1, d2};
  toy_embed_plan p;
  const int rc = toy_plan_embed(obj, od, off, img, d, &p);
  if (rc == VX_OK) printf("%s %d %d %d %d %d %d %d\n", name, rc, p.lo[0], p.hi[0], p.lo[1], p.hi[1], p.lo[2], p.hi[2]);
  else printf("%s %d\n", name, rc);
}

static void blur_case(const char* name, const void* src, const void* dst, const void* w, int d0, int d1, int d2, int axis, int radius) {
  const int32_t d[3] = {d0, d1, d2};
  toy_blur_plan p;
  const int rc = toy_plan_blur(src, dst, d, axis, w, radius, &p);
  if (rc == VX_OK) printf("%s %d %d %d %lld %zu %d\n", name, rc, p.tw, p.ring_rows, (long long)p.blocks, p.lds, p.vec);
  else printf("%s %d\n", name, rc);
  if (rc == VX_OK && p.lds > TOY_LDS_BYTES) printf("%s BAD-LDS\n", name);
}

static void os_case(const char* name, const void* x, int64_t n, const int64_t* ks, int n_k, const void* out, const void* st, const void* ws, int64_t wsb) {
  toy_os_plan p;
  const int rc = toy_plan_order_stats(x, n, ks, n_k, out, st, ws, wsb, &p);
  if (rc == VX_OK) {
    printf("%s %d %d %d %zu", name, rc, p.n_u, p.reads, p.bytes);
    for (int i = 0; i < n_k; ++i) printf(" %lld %lld", (long long)p.u[p.idx[i][0]], (long long)p.u[p.idx[i][1]]);
    printf("\n");
    for (int i = 1; i < p.n_u; ++i) if (p.u[i - 1] >= p.u[i]) printf("%s BAD-ORDER\n", name);
  } else {
    printf("%s %d\n", name, rc);
  }
}

int main() {
  int bad = 0;
  for (int n = 1; n <= 5; ++n)
    for (int r = 0; r <= TOY_MAX_RADIUS; ++r)
      for (int i = -r; i < n + r; ++i) {
        const int got = toy_reflect(i, n);
        if (got < 0 || got >= n || got != reflect_walk(i, n)) ++bad;
      }
  printf("reflect %d\n", bad);

  const uintptr_t A = 0x10000, B = 0x4000000, W = 0x8000000, S = 0x100000000, D = 0x200000000;
  embed_case("e_inside", at(A), at(B), 5, 6, 7, 3, 4, 5, 20, 20, 20);
  embed_case("e_clip_low", at(A), at(B), 9, 9, 9, -6, -2, -8, 20, 20, 20);
  embed_case("e_clip_high", at(A), at(B), 9, 9, 9, 15, 0, 19, 20, 20, 20);
  embed_case("e_outside", at(A), at(B), 4, 4, 4, -4, 30, 0, 20, 20, 20);
  embed_case("e_null", nullptr, at(B), 4, 4, 4, 0, 0, 0, 20, 20, 20);
  embed_case("e_dim0", at(A), at(B), 4, 0, 4, 0, 0, 0, 20, 20, 20);
  embed_case("e_huge", at(A), at(B), 4, 4, 4, 0, 0, 0, 1 << 20, 1 << 20, 4);
  embed_case("e_align", at(A + 2), at(B), 4, 4, 4, 0, 0, 0, 20, 20, 20);
  embed_case("e_align_img", at(A), at(B + 4), 4, 4, 4, 0, 0, 0, 20, 20, 20);

  blur_case("b_256_a0", at(S), at(D), at(W), 256, 256, 256, 0, 32);
  blur_case("b_256_a1", at(S), at(D), at(W), 256, 256, 256, 1, 32);
  blur_case("b_256_a2", at(S), at(D), at(W), 256, 256, 256, 2, 32);
  blur_case("b_r0", at(A), at(B), at(W), 3, 3, 3, 1, 0);
  blur_case("b_r56", at(A), at(B), at(W), 70, 65, 130, 0, 56);
  blur_case("b_r57", at(A), at(B), at(W), 70, 65, 130, 0, 57);
  blur_case("b_r112", at(A), at(B), at(W), 70, 65, 130, 1, 112);
  blur_case("b_r113", at(A), at(B), at(W), 70, 65, 130, 1, 113);
  blur_case("b_r128", at(A), at(B), at(W), 70, 65, 130, 1, 128);
  blur_case("b_r128_a2", at(A), at(B), at(W), 1, 1, 257, 2, 128);
  blur_case("b_odd", at(A), at(B), at(W), 5, 7, 3, 1, 8);
  blur_case("b_off16", at(A + 8), at(B), at(W), 4, 4, 4, 2, 8);
  blur_case("b_r129", at(A), at(B), at(W), 4, 4, 4, 0, 129);
  blur_case("b_rneg", at(A), at(B), at(W), 4, 4, 4, 0, -1);
  blur_case("b_axis", at(A), at(B), at(W), 4, 4, 4, 3, 2);
  blur_case("b_dim0", at(A), at(B), at(W), 4, 0, 4, 0, 2);
  blur_case("b_null", at(A), nullptr, at(W), 4, 4, 4, 0, 2);
  blur_case("b_nullw", at(A), at(B), nullptr, 4, 4, 4, 0, 2);
  blur_case("b_align", at(A + 4), at(B), at(W), 4, 4, 4, 0, 2);
  blur_case("b_inplace", at(A), at(A), at(W), 4, 4, 4, 0, 2);
  blur_case("b_overlap", at(A), at(A + 64), at(W), 4, 4, 4, 0, 2);
  blur_case("b_touch", at(A), at(A + 512), at(W), 4, 4, 4, 0, 2);
  blur_case("b_huge", at(A), at(B), at(W), 1 << 20, 1 << 20, 4, 0, 2);

  const int64_t ks1[] = {0, 98, 99, 50, 50};
  os_case("o_ok", at(A), 100, ks1, 5, at(B), at(W), at(W + 256), 1 << 20);
  int64_t many[32];
  for (int i = 0; i < 32; ++i) many[i] = 3 * i;
  os_case("o_32", at(A), 1000, many, 32, at(B), at(W), at(W + 256), 1 << 20);
  const int64_t k0[] = {0};
  os_case("o_n1", at(A), 1, k0, 1, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_nk0", at(A), 100, ks1, 0, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_nk33", at(A), 100, ks1, 33, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_n0", at(A), 0, ks1, 1, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_rank", at(A), 99, ks1, 3, at(B), at(W), at(W + 256), 1 << 20);
  const int64_t kneg[] = {-1};
  os_case("o_rank_neg", at(A), 99, kneg, 1, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_null", nullptr, 100, ks1, 5, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_null_ks", at(A), 100, nullptr, 5, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_align", at(A + 4), 100, ks1, 5, at(B), at(W), at(W + 256), 1 << 20);
  os_case("o_ws_align", at(A), 100, ks1, 5, at(B), at(W), at(W + 8), 1 << 20);
  os_case("o_ws_short", at(A), 100, ks1, 5, at(B), at(W), at(W + 256), (int64_t)toy_os_bytes() - 1);
  return 0;
}
