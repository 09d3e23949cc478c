// The rotation solve of K17 (superpose.hip): the largest eigenvalue of the 4 x 4 quaternion key matrix of a 3 x 3
// cross-covariance M, by cyclic Jacobi with a fixed number of sweeps.  Plain C++ (no device intrinsics), so a host
// program can compile the same text.
//
// With S_ab = M[3 a + b] the key matrix (Horn 1987) is the symmetric, traceless
//   [ Sxx+Syy+Szz   Syz-Szy       Szx-Sxz       Sxy-Syx     ]
//   [               Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
//   [                            -Sxx+Syy-Szz   Syz+Szy     ]
//   [                                          -Sxx-Syy+Szz ]
// whose largest eigenvalue is max over PROPER rotations R of sum_k b_k . R a_k (a mirror image is never a solution:
// every unit quaternion is a rotation).  Its eigenvalues do not change under M -> M^T.
//
// Jacobi needs no non-degenerate spectrum: M = 0 (one atom), rank one (collinear), rank two (planar) and repeated
// eigenvalues (identical structures) are ordinary inputs -- a zero off-diagonal element is skipped, nothing is divided
// by a difference of eigenvalues.  SP_SWEEPS sweeps of the six (p, q) rotations: compiled for the host and run against
// LAPACK's eigvalsh on 960 000 key matrices (random, identical, collinear, planar, rotated and inverted structures of
// 1..20 atoms) the result stops changing after five sweeps (quadratic convergence), at most 7.4 x 2^-52 |K|_F from
// LAPACK's and 0.33 x 2^-52 |K|_F on average; two more sweeps are kept in hand.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SP_HD __host__ __device__ __forceinline__
#else
#define SP_HD inline
#endif

namespace cgv {

constexpr int SP_SWEEPS = 7;

// upper triangle of the key matrix, row-major: k[0..3] row 0, k[4..6] row 1, k[7..8] row 2, k[9]
SP_HD void sp_key_matrix(const double* M, double* k) {
  const double xx = M[0], xy = M[1], xz = M[2], yx = M[3], yy = M[4], yz = M[5], zx = M[6], zy = M[7], zz = M[8];
  k[0] = xx + yy + zz;
  k[1] = yz - zy;
  k[2] = zx - xz;
  k[3] = xy - yx;
  k[4] = xx - yy - zz;
  k[5] = xy + yx;
  k[6] = zx + xz;
  k[7] = -xx + yy - zz;
  k[8] = yz + zy;
  k[9] = -xx - yy + zz;
}

constexpr int sp_at(int i, int j) {                          // slot of element (i, j), i <= j
  return i == 0 ? j : i == 1 ? 3 + j : i == 2 ? 5 + j : 9;
}
constexpr int sp_sym(int i, int j) { return i <= j ? sp_at(i, j) : sp_at(j, i); }

template <int P, int Q>
SP_HD void sp_rotate(double* k) {
  const double apq = k[sp_at(P, Q)], app = k[sp_at(P, P)], aqq = k[sp_at(Q, Q)];
  // t = tan of the rotation angle, the smaller root; theta^2 may overflow to +inf: t = 0, the rotation is the identity
  const double theta = (aqq - app) / (2.0 * apq);
  const double root = __builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0);
  double t = (theta < 0.0 ? -1.0 : 1.0) / root;
  if (apq == 0.0) t = 0.0;                                   // (also where theta is 0 / 0)
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
}

SP_HD void sp_sweep(double* k) {
  sp_rotate<0, 1>(k);
  sp_rotate<0, 2>(k);
  sp_rotate<0, 3>(k);
  sp_rotate<1, 2>(k);
  sp_rotate<1, 3>(k);
  sp_rotate<2, 3>(k);
}

SP_HD double sp_largest(const double* k) {
  const double a = k[0] > k[4] ? k[0] : k[4], b = k[7] > k[9] ? k[7] : k[9];
  return a > b ? a : b;
}

}  // namespace cgv
