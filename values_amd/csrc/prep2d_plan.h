// Host-side plan of vx_crop_resize_batched (preprocess2d.hip): the argument checks, the output sizes, the work blocks of
// every item and the workspace layout.  Plain C++ with no HIP in it, so a stand-alone program can run it under a host
// sanitizer (tests/prep2d_plan_host.cpp).
//
// A work block is P2D_BLOCK_PIX pixels of an item's OUTPUT in row-major order, counted from the item's first pixel: how
// an item is cut depends on its own output size alone, never on its batch mates, and what a pixel becomes depends on its
// item alone.  AN ITEM'S OUTPUT BYTES ARE EQUAL WHETHER IT IS SUBMITTED ALONE OR IN ANY BATCH, AT ANY POSITION.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/values_amd.h"
#include "host_checks.h"

#define P2D_THREADS 256
#define P2D_PER_LANE 4                                   // consecutive output pixels of a lane in one step
#define P2D_STEPS 2
#define P2D_BLOCK_PIX (P2D_THREADS * P2D_PER_LANE * P2D_STEPS)
#define P2D_MAX_GRID 2048
#define P2D_MAX_COLORS 256

// one item as the kernel reads it
struct p2d_item_dev {
  const uint8_t* src;
  const uint8_t* palette;
  uint8_t* out_rgb;
  void* out_ids;
  int64_t block0;              // its work blocks are [block0, block0 + n_blocks) of the call
  int32_t n_blocks;
  int32_t H, W, bpp;
  int32_t y0, x0, ch, cw;      // the crop box
  int32_t k;                   // the factor
  int32_t oh, ow;              // the output
  int32_t mode, index;         // index: the item's place in the caller's table (status)
};

struct p2d_plan {
  std::vector<p2d_item_dev> items;
  int64_t n_blocks = 0;
  size_t bytes = 0;            // workspace: the item table
  int code = VX_OK;
  char err[200] = {0};
};

// size / k rounded half to even on the exact quotient: cv2.resize's saturate_cast<int>(size * fx) at fx = 1 / k
static inline int p2d_out_size(int size, int k) {
  if (size < 1 || k < 1 || (k & 1)) return 0;
  const int q = size / k, r = size % k;
  if (2 * r > k) return q + 1;
  if (2 * r < k) return q;
  return q + (q & 1);
}

static inline int p2d_plan_items(const vx_p2d_item* items, int n_items, const vx_p2d_tables* tables, p2d_plan* p) {
  const char* who = "vx_crop_resize_batched";
  if (n_items < 0 || n_items > VX_SELECT_MAX_ITEMS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_items %d outside 0..%d", who, n_items, VX_SELECT_MAX_ITEMS);
  if (n_items == 0) return VX_OK;
  if (!items) VX_REFUSE_CODE(p, VX_E_NULL, "%s: null items", who);
  p->items.reserve((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    const vx_p2d_item& it = items[i];
    if (it.bpp != 1 && it.bpp != 3 && it.bpp != 4) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: bpp %d (1, 3 or 4)", who, i, it.bpp);
    if (it.mode != VX_P2D_IMAGE && it.mode != VX_P2D_LABEL_IDS && it.mode != VX_P2D_LABEL_COLOR)
      VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: mode %d", who, i, it.mode);
    if (it.palette && it.bpp != 1) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: a palette with bpp %d", who, i, it.bpp);
    if (it.mode == VX_P2D_LABEL_IDS) {
      if (it.bpp != 1 || it.palette) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: label ids are a grey image (bpp 1, no palette)", who, i);
    } else if (it.bpp == 1 && !it.palette) {
      VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: item %d: bpp 1 without a palette where a colour image is expected", who, i);
    }
    if (it.H < 1 || it.W < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: H=%d W=%d", who, i, it.H, it.W);
    if ((int64_t)it.H * it.W * it.bpp > 0x7FFFFFFF) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: H W bpp >= 2^31", who, i);
    if (it.factor < 1 || (it.factor & 1)) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: factor %d is not a positive even integer", who, i, it.factor);
    if (it.crop_h < 1 || it.crop_w < 1 || it.y0 < 0 || it.x0 < 0 || (int64_t)it.y0 + it.crop_h > it.H || (int64_t)it.x0 + it.crop_w > it.W)
      VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: crop %d x %d at (%d, %d) outside the %d x %d image", who, i, it.crop_h, it.crop_w, it.y0,
                 it.x0, it.H, it.W);
    const int oh = p2d_out_size(it.crop_h, it.factor), ow = p2d_out_size(it.crop_w, it.factor);
    if (oh < 1 || ow < 1) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: item %d: a %d x %d crop at factor %d has no output", who, i, it.crop_h, it.crop_w, it.factor);
    if (!it.src || !it.out_rgb) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null src or out_rgb", who, i);
    if (it.mode != VX_P2D_IMAGE) {
      if (!it.out_ids) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null out_ids", who, i);
      if (!tables) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null tables", who, i);
    }
    if (it.mode == VX_P2D_LABEL_IDS && (!tables->id2trainid || !tables->trainid2color))
      VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null id2trainid or trainid2color", who, i);
    if (it.mode == VX_P2D_LABEL_COLOR) {
      if (tables->n_color < 0 || tables->n_color > P2D_MAX_COLORS) VX_REFUSE_CODE(p, VX_E_SHAPE, "%s: n_color=%d (0..%d)", who, tables->n_color, P2D_MAX_COLORS);
      if (tables->default_id < 0 || tables->default_id > 255) VX_REFUSE_CODE(p, VX_E_DTYPE, "%s: default_id=%d", who, tables->default_id);
      if (tables->n_color > 0 && !tables->color2trainid) VX_REFUSE_CODE(p, VX_E_NULL, "%s: item %d: null color2trainid", who, i);
      if ((uintptr_t)it.out_ids & 7) VX_REFUSE_CODE(p, VX_E_ALIGN, "%s: item %d: int64 out_ids not aligned to 8 bytes", who, i);
    }
    p2d_item_dev d;
    d.src = it.src; d.palette = it.palette; d.out_rgb = it.out_rgb; d.out_ids = it.mode == VX_P2D_IMAGE ? nullptr : it.out_ids;
    d.block0 = p->n_blocks;
    d.n_blocks = (int32_t)(((int64_t)oh * ow + P2D_BLOCK_PIX - 1) / P2D_BLOCK_PIX);
    d.H = it.H; d.W = it.W; d.bpp = it.bpp;
    d.y0 = it.y0; d.x0 = it.x0; d.ch = it.crop_h; d.cw = it.crop_w;
    d.k = it.factor; d.oh = oh; d.ow = ow; d.mode = it.mode; d.index = i;
    p->items.push_back(d);
    p->n_blocks += d.n_blocks;
  }
  p->bytes = vx_align256((size_t)n_items * sizeof(p2d_item_dev));
  return VX_OK;
}
