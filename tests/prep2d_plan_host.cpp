// Stand-alone driver of values_amd/csrc/prep2d_plan.h, the host plan of vx_crop_resize_batched (argument checks, output
// sizes, work blocks, workspace layout), built under -fsanitize=address,undefined by tests/test_preprocess2d_cpu.py.  The
// pointers are made-up addresses: the plan never dereferences them.
//   prep2d_plan_host  ->  one line per case: "<name> <code> <work blocks> <workspace bytes>", "size <size> <k> <out>" for
//                         the output sizes, and "<name> BAD-BLOCKS" where the lanes' pixels do not tile an item's output
#include <stdio.h>

#include <vector>

#include "../values_amd/csrc/prep2d_plan.h"

static uint8_t* at(uintptr_t a) { return (uint8_t*)a; }
static const uintptr_t A = 0x10000, B = 0x4000000, C = 0x8000000, P = 0x20000;

static vx_p2d_item item(int mode, int bpp, uintptr_t pal, int H, int W, int y0, int x0, int ch, int cw, int k) {
  vx_p2d_item it = {};
  it.src = at(A); it.palette = pal ? at(pal) : nullptr;
  it.H = H; it.W = W; it.bpp = bpp; it.y0 = y0; it.x0 = x0; it.crop_h = ch; it.crop_w = cw; it.factor = k; it.mode = mode;
  it.out_rgb = at(B); it.out_ids = at(C);
  return it;
}

static vx_p2d_tables tables() {
  vx_p2d_tables t = {};
  t.id2trainid = at(P); t.trainid2color = at(P + 256); t.color2trainid = (const uint32_t*)at(P + 1024);
  t.n_color = 35; t.default_id = 128;
  return t;
}

// every pixel of every item's output is produced by exactly one lane step of exactly one of the item's blocks, by the
// index arithmetic of the kernel (preprocess2d.hip: p0 = block * P2D_BLOCK_PIX + (u * P2D_THREADS + tid) * P2D_PER_LANE)
static bool tiles(const p2d_plan& p) {
  int64_t next = 0;
  for (const p2d_item_dev& d : p.items) {
    const int64_t npix = (int64_t)d.oh * d.ow;
    if (d.block0 != next || d.n_blocks != (npix + P2D_BLOCK_PIX - 1) / P2D_BLOCK_PIX) return false;
    next += d.n_blocks;
    std::vector<uint8_t> hit((size_t)npix, 0);
    for (int64_t b = 0; b < d.n_blocks; ++b)
      for (int u = 0; u < P2D_STEPS; ++u)
        for (int tid = 0; tid < P2D_THREADS; ++tid) {
          const int64_t p0 = b * P2D_BLOCK_PIX + (int64_t)(u * P2D_THREADS + tid) * P2D_PER_LANE;
          for (int j = 0; j < P2D_PER_LANE && p0 + j < npix; ++j) ++hit[(size_t)(p0 + j)];
        }
    for (uint8_t h : hit)
      if (h != 1) return false;
  }
  return next == p.n_blocks;
}

static void run(const char* name, const std::vector<vx_p2d_item>& items, int n_items, const vx_p2d_tables* t, bool null_table = false) {
  p2d_plan p;
  const int rc = p2d_plan_items(null_table ? nullptr : items.data(), n_items, t, &p);
  printf("%s %d %lld %zu\n", name, rc, (long long)p.n_blocks, rc == VX_OK ? p.bytes : (size_t)0);
  if (rc == VX_OK && !tiles(p)) printf("%s BAD-BLOCKS\n", name);
  if (rc != VX_OK && !p.err[0]) printf("%s NO-MESSAGE\n", name);
}

int main() {
  const int IMG = VX_P2D_IMAGE, IDS = VX_P2D_LABEL_IDS, COL = VX_P2D_LABEL_COLOR;
  const vx_p2d_tables t = tables();
  for (int k : {2, 4, 6})
    for (int size : {1, 2, 3, 5, 6, 7, 8, 9, 10, 15, 16, 18, 21, 1024, 1912}) printf("size %d %d %d\n", size, k, p2d_out_size(size, k));
  printf("size 8 3 %d\nsize 8 0 %d\nsize 0 4 %d\nsize 8 -2 %d\n", p2d_out_size(8, 3), p2d_out_size(8, 0), p2d_out_size(0, 4), p2d_out_size(8, -2));

  run("empty", {}, 0, &t);
  run("null", {}, 2, &t, true);
  run("count", {}, VX_SELECT_MAX_ITEMS + 1, &t, true);
  run("negative", {}, -1, &t, true);
  run("one_image", {item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, nullptr);
  run("one_ids", {item(IDS, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("one_color", {item(COL, 1, P, 13, 22, 2, 3, 8, 16, 2)}, 1, &t);
  run("contract", {item(IMG, 3, 0, 1052, 1914, 14, 1, 1024, 1912, 4)}, 1, &t);
  // mixed sizes and modes; the third item's 30 x 101 output ends its first block inside row 20
  run("mixed", {item(IMG, 4, 0, 13, 22, 2, 3, 8, 16, 4), item(COL, 3, 0, 1052, 1914, 14, 1, 1024, 1912, 4),
                item(IMG, 3, 0, 121, 405, 0, 1, 120, 404, 4), item(IDS, 1, 0, 9, 17, 0, 0, 8, 16, 2),
                item(COL, 4, 0, 7, 7, 0, 0, 6, 6, 4)}, 5, &t);
  std::vector<vx_p2d_item> many(4096, item(IDS, 1, 0, 9, 17, 0, 0, 8, 16, 4));
  run("many", many, 4096, &t);

  run("bpp", {item(IMG, 2, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("mode", {item(3, 3, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("pal_bpp3", {item(COL, 3, P, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("color_grey", {item(COL, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("image_grey", {item(IMG, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("ids_rgb", {item(IDS, 3, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("ids_pal", {item(IDS, 1, P, 13, 22, 2, 3, 8, 16, 4)}, 1, &t);
  run("dim0", {item(IMG, 3, 0, 0, 22, 0, 0, 8, 16, 4)}, 1, &t);
  run("huge", {item(IMG, 4, 0, 1 << 15, 1 << 14, 0, 0, 8, 16, 4)}, 1, &t);          // H W bpp = 2^31
  run("below_huge", {item(IMG, 1, P, (1 << 15) - 1, 1 << 16, 0, 0, 8, 16, 4)}, 1, &t);
  run("odd", {item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, 3)}, 1, &t);
  run("factor0", {item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, 0)}, 1, &t);
  run("factor_neg", {item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, -4)}, 1, &t);
  run("crop_right", {item(IMG, 3, 0, 13, 22, 2, 7, 8, 16, 4)}, 1, &t);
  run("crop_below", {item(IMG, 3, 0, 13, 22, 6, 3, 8, 16, 4)}, 1, &t);
  run("crop_neg", {item(IMG, 3, 0, 13, 22, -1, 3, 8, 16, 4)}, 1, &t);
  run("crop_empty", {item(IMG, 3, 0, 13, 22, 2, 3, 0, 16, 4)}, 1, &t);
  run("crop_wrap", {item(IMG, 3, 0, 13, 22, 0x7FFFFFFF, 3, 8, 16, 4)}, 1, &t);
  run("out0", {item(IMG, 3, 0, 13, 22, 2, 3, 1, 16, 4)}, 1, &t);                     // 1 / 4 rounds to 0 rows
  {
    vx_p2d_item it = item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, 4);
    it.src = nullptr;
    run("null_src", {it}, 1, &t);
    it = item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, 4);
    it.out_rgb = nullptr;
    run("null_rgb", {it}, 1, &t);
    it = item(IMG, 3, 0, 13, 22, 2, 3, 8, 16, 4);
    it.out_ids = nullptr;                                                             // an image has no ids
    run("image_no_ids", {it}, 1, nullptr);
    it = item(IDS, 1, 0, 13, 22, 2, 3, 8, 16, 4);
    it.out_ids = nullptr;
    run("null_ids", {it}, 1, &t);
    run("null_tables", {item(IDS, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, nullptr);
    vx_p2d_tables u = tables();
    u.id2trainid = nullptr;
    run("null_id_table", {item(IDS, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &u);
    u = tables();
    u.trainid2color = nullptr;
    run("null_colour_table", {item(IDS, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &u);
    u = tables();
    u.color2trainid = nullptr;
    run("null_lookup", {item(COL, 3, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &u);
    run("lookup_unused", {item(IDS, 1, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &u);
    u = tables();
    u.n_color = 257;
    run("n_color", {item(COL, 3, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &u);
    u = tables();
    u.default_id = 256;
    run("default_id", {item(COL, 3, 0, 13, 22, 2, 3, 8, 16, 4)}, 1, &u);
    it = item(COL, 3, 0, 13, 22, 2, 3, 8, 16, 4);
    it.out_ids = at(C + 4);
    run("ids_align", {it}, 1, &t);
  }
  return 0;
}
