// Stand-alone host check of csrc/procrustes_solve.h, the float64 similarity solve of procrustes_kernel / procrustes_vis_kernel (csrc/eval.hip):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I egohmr_amd/csrc tools/procrustes_check.cpp -o procrustes_check
//     ./procrustes_check cases.txt > aligned.txt
//
// cases.txt:  n, then per case "J masked" and J lines "px py pz gx gy gz m" (float32 values printed with 9 significant digits; m = 0 / 1, read only
// when masked = 1: the visible-joint alignment, whose invisible joints enter the moments as points at the origin).
// aligned.txt: per case J lines "hx hy hz", the similarity applied to the unmasked prediction, with 17 significant digits (float64, before the
// kernels' float32 store).  The moments are accumulated exactly as the kernels do: joint by joint, in float64.
// tests/test_eval_ref_cpu.py builds this under AddressSanitizer + UBSan and compares with the numpy references (tests/eval_ref.py).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "procrustes_solve.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int n = 0;
  if (fscanf(f, "%d", &n) != 1 || n < 0) { fprintf(stderr, "bad case count\n"); return 2; }
  for (int i = 0; i < n; ++i) {
    int J = 0, masked = 0;
    if (fscanf(f, "%d %d", &J, &masked) != 2 || J < 1 || J > (1 << 20)) { fprintf(stderr, "case %d: bad header\n", i); return 2; }
    std::vector<float> p(3 * (size_t)J), g(3 * (size_t)J);
    std::vector<int> m((size_t)J, 1);
    for (int j = 0; j < J; ++j) {
      int mj = 1;
      if (fscanf(f, "%f %f %f %f %f %f %d", &p[3 * j], &p[3 * j + 1], &p[3 * j + 2], &g[3 * j], &g[3 * j + 1], &g[3 * j + 2], &mj) != 7) {
        fprintf(stderr, "case %d: bad joint %d\n", i, j);
        return 2;
      }
      if (masked) m[j] = mj != 0;
    }
    double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
    for (int j = 0; j < J; ++j) {
      const double w = m[j] ? 1.0 : 0.0;
      for (int c = 0; c < 3; ++c) { mu1[c] += w * (double)p[3 * j + c]; mu2[c] += w * (double)g[3 * j + c]; }
    }
    for (int c = 0; c < 3; ++c) { mu1[c] /= J; mu2[c] /= J; }
    double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
    for (int j = 0; j < J; ++j) {
      const double w = m[j] ? 1.0 : 0.0;
      double x1[3], x2[3];
      for (int c = 0; c < 3; ++c) { x1[c] = w * (double)p[3 * j + c] - mu1[c]; x2[c] = w * (double)g[3 * j + c] - mu2[c]; var1 += x1[c] * x1[c]; }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K[r][c] += x1[r] * x2[c];
    }
    double Rm[3][3], scale, t[3];
    procrustes_solve::similarity(K, var1, mu1, mu2, Rm, &scale, t);
    for (int j = 0; j < J; ++j) {
      double h[3];
      for (int r = 0; r < 3; ++r)
        h[r] = scale * (Rm[r][0] * (double)p[3 * j] + Rm[r][1] * (double)p[3 * j + 1] + Rm[r][2] * (double)p[3 * j + 2]) + t[r];
      printf("%.17g %.17g %.17g\n", h[0], h[1], h[2]);
    }
  }
  fclose(f);
  return 0;
}
