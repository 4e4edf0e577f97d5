// The float64 similarity solve of the two Procrustes kernels (csrc/eval.hip), as plain C++ that a host compiler builds too (tools/procrustes_check.cpp):
// utils/pose_utils.py:36-60 of the reference from the moments K = X1 X2^T, var1 = |X1|^2, mu1, mu2 of the centred clouds to R, scale and t.
//   svd3          3 x 3 SVD by one-sided Jacobi, with an orthonormal completion of U for rank-deficient K
//   det3          3 x 3 determinant
//   similarity    R = V Z U^T with Z = diag(1, 1, det(U V^T)) on the smallest singular direction, scale = trace(R K) / var1, t = mu2 - scale R mu1
// Everything is a function of its arguments: no global state, no allocation, no J-sized array.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define EHM_PS_HD __host__ __device__ inline
#else
#define EHM_PS_HD inline
#endif

namespace procrustes_solve {

// One-sided Jacobi on the columns of a 3 x 3 matrix: K V = B with orthogonal columns (B = U diag(s)).  float64: converges in 4 - 6 sweeps.
// The columns of U that belong to a zero singular value are not determined by K; they are completed to a right-handed or left-handed orthonormal frame
// (the caller's Z absorbs the handedness), the known columns are always kept:
//   rank 2   the missing column is the cross product of the other two
//   rank 1   the known column u, a unit vector v orthogonal to it (u x the coordinate axis u is least aligned with) and u x v
//   rank 0   K = 0: U = V (the rotation is irrelevant: the caller's scale is 0)
EHM_PS_HD void svd3(const double K[3][3], double U[3][3], double s[3], double V[3][3]) {
  double Bm[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { Bm[r][c] = K[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int r = 0; r < 3; ++r) { al += Bm[r][p] * Bm[r][p]; be += Bm[r][q] * Bm[r][q]; ga += Bm[r][p] * Bm[r][q]; }
        if (ga == 0.0 || fabs(ga) <= 1e-300) continue;
        off = fmax(off, fabs(ga) / sqrt(fmax(al * be, 1e-300)));
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int r = 0; r < 3; ++r) {
          const double bp = Bm[r][p], bq = Bm[r][q];
          Bm[r][p] = c * bp - sn * bq; Bm[r][q] = sn * bp + c * bq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = c * vp - sn * vq; V[r][q] = sn * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  double smax = 0.0;
  for (int c = 0; c < 3; ++c) {
    s[c] = sqrt(Bm[0][c] * Bm[0][c] + Bm[1][c] * Bm[1][c] + Bm[2][c] * Bm[2][c]);
    smax = fmax(smax, s[c]);
  }
  int good[3] = {0, 0, 0}, ng = 0;
  for (int c = 0; c < 3; ++c) {
    if (s[c] > 1e-13 * smax && s[c] > 0.0) { for (int r = 0; r < 3; ++r) U[r][c] = Bm[r][c] / s[c]; good[ng++] = c; }
  }
  if (ng == 2) {               // rank 2: the missing left vector completes the frame (its sign is absorbed by Z = diag(1, 1, det))
    const int m = 3 - good[0] - good[1], a = good[0], bq = good[1];
    U[0][m] = U[1][a] * U[2][bq] - U[2][a] * U[1][bq];
    U[1][m] = U[2][a] * U[0][bq] - U[0][a] * U[2][bq];
    U[2][m] = U[0][a] * U[1][bq] - U[1][a] * U[0][bq];
  } else if (ng == 1) {        // rank 1: R must still take the known left vector onto its right vector; the other two columns are any orthonormal pair
    const int a = good[0], m1 = (a + 1) % 3, m2 = (a + 2) % 3;
    const double u[3] = {U[0][a], U[1][a], U[2][a]};
    int ax = 0;
    if (fabs(u[1]) < fabs(u[ax])) ax = 1;
    if (fabs(u[2]) < fabs(u[ax])) ax = 2;
    double e[3] = {0.0, 0.0, 0.0};
    e[ax] = 1.0;
    double v[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};   // |u x e| >= sqrt(2 / 3): |u[ax]| <= 1 / sqrt(3)
    const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int r = 0; r < 3; ++r) v[r] /= nv;
    U[0][m1] = v[0]; U[1][m1] = v[1]; U[2][m1] = v[2];
    U[0][m2] = u[1] * v[2] - u[2] * v[1];
    U[1][m2] = u[2] * v[0] - u[0] * v[2];
    U[2][m2] = u[0] * v[1] - u[1] * v[0];
  } else if (ng == 0) {        // K = 0
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) U[r][c] = V[r][c];
  }
}

EHM_PS_HD double det3(const double A[3][3]) {
  return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// pose_utils.py:39-60.  var1 = 0 (a one-point cloud): scale = 0 / 0 = NaN and every aligned point is NaN, as the reference.
EHM_PS_HD void similarity(const double K[3][3], double var1, const double mu1[3], const double mu2[3], double Rm[3][3], double* scale, double t[3]) {
  double U[3][3], s[3], V[3][3];
  svd3(K, U, s, V);
  // Z = diag(1, 1, sign(det(U V^T))) acts on the SMALLEST singular value (numpy sorts them in descending order: pose_utils.py:42-46).  For a
  // rank-deficient K that is a zero direction, so det R = +1 costs nothing of trace(R K).
  int mn = 0;
  if (s[1] < s[mn]) mn = 1;
  if (s[2] < s[mn]) mn = 2;
  const double dsign = det3(U) * det3(V) >= 0.0 ? 1.0 : -1.0;               // det(U V^T) = det U det V
  double tr = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc += (k == mn ? dsign : 1.0) * V[r][k] * U[c][k];   // R = V Z U^T
      Rm[r][c] = acc;
    }
  for (int k = 0; k < 3; ++k) tr += (k == mn ? dsign : 1.0) * s[k];          // trace(R K) = sum_k z_k s_k
  *scale = tr / var1;
  for (int r = 0; r < 3; ++r) t[r] = mu2[r] - *scale * (Rm[r][0] * mu1[0] + Rm[r][1] * mu1[1] + Rm[r][2] * mu1[2]);
}

}  // namespace procrustes_solve
