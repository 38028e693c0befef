// Stand-alone driver of values_amd/csrc/prep_plan.h, the host plan of vx_volume_stats_batched and vx_zscore_pad_batched
// (argument checks, work blocks, workspace layout), built under -fsanitize=address,undefined by
// tests/test_preprocess_cpu.py.  The pointers are made-up addresses: the plan never dereferences them.
//   prep_plan_host  ->  one line per case: "<name> <code> <work blocks> <workspace bytes>"
#include <stdio.h>

#include <vector>

#include "../values_amd/csrc/prep_plan.h"

static void* at(uintptr_t a) { return (void*)a; }

static vx_prep_pad_item pad(uintptr_t src, uintptr_t dst, int kind, int d0, int d1, int d2, int o0, int o1, int o2, int l0, int l1, int l2,
                            int out, int mode, int row) {
  vx_prep_pad_item it = {};
  it.src = at(src); it.dst = at(dst);
  it.dims[0] = d0; it.dims[1] = d1; it.dims[2] = d2;
  it.out_dims[0] = o0; it.out_dims[1] = o1; it.out_dims[2] = o2;
  it.pad_below[0] = l0; it.pad_below[1] = l1; it.pad_below[2] = l2;
  it.kind = kind; it.out_dtype = out; it.mode = mode; it.stats_row = row;
  return it;
}

static void stats_case(const char* name, const std::vector<vx_prep_item>& items, int n_items, bool null_table = false) {
  pp_plan p;
  const int rc = pp_plan_stats(null_table ? nullptr : items.data(), n_items, &p);
  printf("%s %d %lld %zu\n", name, rc, (long long)p.n_blocks, rc == VX_OK ? p.bytes : (size_t)0);
  // the blocks of the items lie back to back and each item's count follows from its own n and kind
  int64_t next = 0;
  for (const pp_stat_item& s : p.stat) {
    if (rc == VX_OK && (s.block0 != next || s.n_blocks != (s.n * pp_elem_bytes(s.kind) + PP_BLOCK_BYTES - 1) / PP_BLOCK_BYTES)) printf("%s BAD-BLOCKS\n", name);
    next += s.n_blocks;
  }
}

static void pad_case(const char* name, const std::vector<vx_prep_pad_item>& items, int n_items, bool null_table = false) {
  pp_plan p;
  const int rc = pp_plan_pad(null_table ? nullptr : items.data(), n_items, &p);
  printf("%s %d %lld %zu\n", name, rc, (long long)p.n_blocks, rc == VX_OK ? p.bytes : (size_t)0);
}

int main() {
  const uintptr_t A = 0x10000, B = 0x4000000;
  stats_case("s_empty", {}, 0);
  stats_case("s_null", {}, 2, true);
  stats_case("s_count", {}, VX_SELECT_MAX_ITEMS + 1, true);
  stats_case("s_negative", {}, -1, true);
  stats_case("s_one", {{at(A), 1, VX_PREP_F64, 0}}, 1);
  stats_case("s_mixed", {{at(A), 4420, VX_PREP_I16, 0}, {at(B), 40 * 33 * 29, VX_PREP_I16, 0}, {at(B + 4), 64 * 64 * 64, VX_PREP_F32, 0},
                         {at(A + 1), 2600, VX_PREP_U8, 0}, {at(A), (int64_t)1 << 40, VX_PREP_F64, 0}}, 5);
  stats_case("s_kind", {{at(A), 8, 8, 0}}, 1);
  stats_case("s_kind_neg", {{at(A), 8, -1, 0}}, 1);
  stats_case("s_n0", {{at(A), 0, VX_PREP_U8, 0}}, 1);
  stats_case("s_nbig", {{at(A), ((int64_t)1 << 40) + 1, VX_PREP_U8, 0}}, 1);
  stats_case("s_nullptr", {{nullptr, 8, VX_PREP_U8, 0}}, 1);
  stats_case("s_align", {{at(A + 2), 8, VX_PREP_I32, 0}}, 1);
  std::vector<vx_prep_item> many((size_t)VX_SELECT_MAX_ITEMS, vx_prep_item{at(A), 3, VX_PREP_I8, 0});
  stats_case("s_max", many, VX_SELECT_MAX_ITEMS);

  pad_case("p_empty", {}, 0);
  pad_case("p_null", {}, 1, true);
  pad_case("p_count", {}, VX_SELECT_MAX_ITEMS + 1, true);
  pad_case("p_ok", {pad(A, B, VX_PREP_I16, 20, 17, 13, 40, 34, 26, 10, 8, 6, VX_F64, VX_PREP_ZSCORE, 0),
                    pad(A, B, VX_PREP_U8, 20, 17, 13, 40, 34, 26, 10, 8, 6, VX_PREP_OWN, VX_PREP_COPY, 1),
                    pad(A, B, VX_PREP_F32, 64, 64, 64, 64, 64, 64, 0, 0, 0, VX_PREP_OWN, VX_PREP_ZSCORE, 2)}, 3);
  pad_case("p_kind", {pad(A, B, 9, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_mode", {pad(A, B, VX_PREP_U8, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F64, 2, 0)}, 1);
  pad_case("p_out", {pad(A, B, VX_PREP_U8, 2, 2, 2, 2, 2, 2, 0, 0, 0, 2, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_copy_out", {pad(A, B, VX_PREP_U8, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F32, VX_PREP_COPY, 0)}, 1);
  pad_case("p_dim0", {pad(A, B, VX_PREP_U8, 2, 0, 2, 2, 2, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_fit", {pad(A, B, VX_PREP_U8, 2, 2, 2, 2, 3, 2, 0, 2, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_below", {pad(A, B, VX_PREP_U8, 2, 2, 2, 2, 3, 2, 0, -1, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_huge", {pad(A, B, VX_PREP_U8, 2, 2, 2, 1 << 20, 1 << 20, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_row", {pad(A, B, VX_PREP_U8, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, VX_SELECT_MAX_ITEMS)}, 1);
  pad_case("p_nullptr", {pad(0, B, VX_PREP_U8, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_src_align", {pad(A + 1, B, VX_PREP_I16, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_dst_align", {pad(A, B + 4, VX_PREP_I16, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F64, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_overlap", {pad(A, A + 4, VX_PREP_I16, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F32, VX_PREP_ZSCORE, 0)}, 1);
  pad_case("p_touch", {pad(A, A + 16, VX_PREP_I16, 2, 2, 2, 2, 2, 2, 0, 0, 0, VX_F32, VX_PREP_ZSCORE, 0)}, 1);
  return 0;
}
