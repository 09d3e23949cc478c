// The rotation solve of K21 (align_mean.hip): the PROPER rotation R that maximises sum_k b_k . R a_k for a 3 x 3
// cross-covariance M[3 i + j] = sum_k a_k[i] b_k[j], through the eigenvector of the largest eigenvalue of the quaternion
// key matrix (superpose_eig.h).  The sweeps are those of sp_sweep -- the same rotations in the same order, the key matrix
// goes through the same operations and ends in the same bits -- and the product of the rotations is accumulated beside
// them.  Plain C++ (no device intrinsics), so a host program can compile the same text.  superpose_eig.h is unchanged:
// what K17 computes does not pass through this file.
//
// The rule, whatever the spectrum:
//   * V starts as the identity and takes every Jacobi rotation from the right: after SP_SWEEPS sweeps its column j is the
//     eigenvector of the diagonal entry j.
//   * the quaternion is the column of the LARGEST diagonal entry, the LOWEST index among equal ones (inside a degenerate
//     eigenspace -- collinear or coincident atoms, M = 0 -- that is the vector the fixed sweep sequence leaves there: a
//     function of M alone);
//   * it is divided by its length (V is orthogonal to rounding) and its sign is chosen so that its component of largest
//     magnitude, the lowest index among equal ones, is positive.  R does not depend on the sign.
// Every unit quaternion is a rotation with determinant +1: a mirror image is never a solution.
#pragma once

#include "superpose_eig.h"

namespace cgv {

// sp_rotate<P, Q> on the key matrix, and the same rotation applied to the columns P and Q of v (row-major 4 x 4)
template <int P, int Q>
SP_HD void sp_rotate_vec(double* k, double* v) {
  const double apq = k[sp_at(P, Q)], app = k[sp_at(P, P)], aqq = k[sp_at(Q, Q)];
  const double theta = (aqq - app) / (2.0 * apq);
  const double root = __builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0);
  double t = (theta < 0.0 ? -1.0 : 1.0) / root;
  if (apq == 0.0) t = 0.0;
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  k[sp_at(P, P)] = app - t * apq;
  k[sp_at(Q, Q)] = aqq + t * apq;
  k[sp_at(P, Q)] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = k[sp_sym(r, P)], arq = k[sp_sym(r, Q)];
      k[sp_sym(r, P)] = arp - s * (arq + tau * arp);
      k[sp_sym(r, Q)] = arq + s * (arp - tau * arq);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double vp = v[4 * r + P], vq = v[4 * r + Q];
    v[4 * r + P] = vp - s * (vq + tau * vp);
    v[4 * r + Q] = vq + s * (vp - tau * vq);
  }
}

SP_HD void sp_sweep_vec(double* k, double* v) {
  sp_rotate_vec<0, 1>(k, v);
  sp_rotate_vec<0, 2>(k, v);
  sp_rotate_vec<0, 3>(k, v);
  sp_rotate_vec<1, 2>(k, v);
  sp_rotate_vec<1, 3>(k, v);
  sp_rotate_vec<2, 3>(k, v);
}

// M [9] -> R [9] row-major (y = R a superposes a onto b), the unit quaternion q [4] = (w, x, y, z) behind it, and the
// largest eigenvalue (= sp_largest of the swept key matrix)
SP_HD double sp_rotation(const double* M, double* R, double* q) {
  double k[10], v[16];
  sp_key_matrix(M, k);
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < SP_SWEEPS; ++sweep) sp_sweep_vec(k, v);
  double top = k[0];
  int at = 0;
  if (k[4] > top) top = k[4], at = 1;
  if (k[7] > top) top = k[7], at = 2;
  if (k[9] > top) top = k[9], at = 3;
  double w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = at == 0 ? v[4 * r] : at == 1 ? v[4 * r + 1] : at == 2 ? v[4 * r + 2] : v[4 * r + 3];
  const double len = __builtin_sqrt((w[0] * w[0] + w[1] * w[1]) + (w[2] * w[2] + w[3] * w[3]));
  double wb = w[0];
#pragma unroll
  for (int r = 1; r < 4; ++r)
    if (__builtin_fabs(w[r]) > __builtin_fabs(wb)) wb = w[r];
  const double scale = (wb < 0.0 ? -1.0 : 1.0) / len;
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = w[r] * scale;
  const double q0 = q[0], qx = q[1], qy = q[2], qz = q[3];
  R[0] = (q0 * q0 + qx * qx) - (qy * qy + qz * qz);
  R[1] = 2.0 * (qx * qy - q0 * qz);
  R[2] = 2.0 * (qx * qz + q0 * qy);
  R[3] = 2.0 * (qy * qx + q0 * qz);
  R[4] = (q0 * q0 + qy * qy) - (qx * qx + qz * qz);
  R[5] = 2.0 * (qy * qz - q0 * qx);
  R[6] = 2.0 * (qz * qx - q0 * qy);
  R[7] = 2.0 * (qz * qy + q0 * qx);
  R[8] = (q0 * q0 + qz * qz) - (qx * qx + qy * qy);
  return top;
}

}  // namespace cgv
