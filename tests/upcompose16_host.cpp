// Host side of tests/test_upcompose16_cpu.py: evaluates values_amd/csrc/upcompose16.h (the algebra the pack kernel of the composed
// level-1 up-convolution runs on the device) on weights read from a file, and prints every Weff element and btab entry.
//   usage: upcompose16_host <file of float32: w1[16][32][3][3][3], uw[32][16][2][2][2], ub[16]>
// Built by the test with -fsanitize=address,undefined; a stand-alone program.
#include <cstdio>
#include <vector>

#include "../values_amd/csrc/upcompose16.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s weights.bin\n", argv[0]); return 2; }
  const size_t n1 = 16 * 32 * 27, nu = 32 * 16 * 8, nb = 16;
  std::vector<float> buf(n1 + nu + nb);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(buf.data(), sizeof(float), buf.size(), f) != buf.size()) { fprintf(stderr, "short read\n"); return 2; }
  fclose(f);
  const float *w1 = buf.data(), *uw = w1 + n1, *ub = uw + nu;
  for (int cls = 0; cls < 8; ++cls)
    for (int tap = 0; tap < 8; ++tap)
      for (int ci = 0; ci < 32; ++ci)
        for (int co = 0; co < 16; ++co) printf("%.17g\n", vx_upc16_weff(w1, 32, uw, cls, tap, ci, co));
  for (int cz = 0; cz < 3; ++cz)
    for (int cy = 0; cy < 3; ++cy)
      for (int cx = 0; cx < 3; ++cx)
        for (int co = 0; co < 16; ++co) printf("%.17g\n", vx_upc16_btab(w1, 32, ub, cz, cy, cx, co));
  printf("floats %d\n", (int)VX_UPC16_FLOATS);
  return 0;
}
