// Stand-alone host program over deep_tail() / deep_stat_parts() of values_amd/csrc/conv3d_route.h (how conv3d_deep.hip shares the
// pairs of its last, partly filled round among idle workgroups), built with -fsanitize=address,undefined by
// tests/test_deep_tail_route_cpu.py.  No GPU, no library, nothing loaded into Python.
//   1. "P G cap" lines on stdin -> "P G cap full rest split tail0 grid";
//   2. a walk over every (P, G, cap) of a grid, checking what the kernel relies on: every pair has exactly one owner per part, no
//      workgroup index leaves the grid, a split never exceeds the cap -- prints "walked <n> unsound <k>".
#include <stdio.h>

#include "../values_amd/csrc/conv3d_route.h"

static bool sound(int P, int G, int cap) {
  const DeepTail t = deep_tail(P, G, cap);
  if (t.full != P / G || t.tail0 != t.full * G || t.rest != P - t.tail0) return false;
  if (t.split != 1 && t.split != 2 && t.split != 4) return false;
  if (t.split > cap || t.split > 1 && (long long)t.rest * t.split > G) return false;
  if (t.split < 4 && cap >= 4 && t.rest > 0 && t.rest * 4 <= G) return false;                     // the largest that fits
  if (t.split < 2 && cap >= 2 && t.rest > 0 && t.rest * 2 <= G) return false;
  if (t.grid != (t.full > 0 ? G : t.rest * t.split) || t.grid < 1 || t.grid > G) return false;
  // the kernel's pair list: workgroup vb < rest * split takes part vb % split of pair tail0 + vb / split
  const int wgs = t.rest * t.split;
  if (wgs > t.grid) return false;
  if (wgs > 0 && t.tail0 + (wgs - 1) / t.split != P - 1) return false;
  return true;
}

int main() {
  int P, G, cap;
  while (scanf("%d %d %d", &P, &G, &cap) == 3) {
    const DeepTail t = deep_tail(P, G, cap);
    printf("%d %d %d %d %d %d %d %d\n", P, G, cap, t.full, t.rest, t.split, t.tail0, t.grid);
  }
  long long walked = 0, unsound = 0;
  const int grids[] = {1, 2, 3, 4, 7, 8, 64, 104, 120, 256, 304, 1024};
  for (int G : grids)
    for (int cap = 1; cap <= 4; cap <<= 1) {
      for (int P = 1; P <= 4 * G + 5; ++P) { ++walked; unsound += sound(P, G, cap) ? 0 : 1; }
      const int big[] = {2147483647, 2147483646, 1 << 30};
      for (int P : big) { ++walked; unsound += sound(P, G, cap) ? 0 : 1; }
    }
  // statistics: as many wave groups as the tile's block holds entries, never more than 4
  for (int epc = 0; epc < 70; ++epc) {
    const int p = deep_stat_parts(epc);
    ++walked;
    if (p != (epc >= 4 ? 4 : epc >= 2 ? 2 : 1) || (epc > 0 && p > epc)) ++unsound;
  }
  printf("walked %lld unsound %lld\n", walked, unsound);
  return unsound ? 1 : 0;
}
