// Multibody knots, the quasi-static control: the u that holds x = (q, 0) still
// (DifferentialActionModelFreeFwdDynamics / ContactFwdDynamics::quasiStatic,
// free-fwddyn.hxx:137-160, contact-fwddyn.hxx:169-207),
//   u = (A^+ g)[0:nu],  A = [dtau/du | Jc^T] (nv x p, p = nu + nc),  g = rnea(q, 0, 0),
// the minimum-norm least-squares solution truncated at sigma_k <= max(nv, p) eps sigma_max.
// A may be wide (contacts), tall (a free-floating base) or rank deficient (the Solo12 trot's
// two-foot knots: 18 x 18 of rank 17, and g outside its range), so the solve is rank revealing:
// one-sided (Hestenes) Jacobi on the nv columns of the (p + 1) x nv array [A^T; g^T]. The
// rotations are decided by the top p rows alone and carry the last row along, which ends as
// h = V^T g; the top block ends as B = A^T V = U Sigma (columns orthogonal, |B_k| = sigma_k), so
//   u_i = sum over sigma_k > tol of B[i, k] h_k / sigma_k^2
// and no V is accumulated.
#pragma once

#include "multibody.hpp"

#if !MB_ACTUATION || !MB_PRISMATIC
#error "mb_quasistatic.hpp needs the actuation and prismatic joint records (MB_ACTUATION, MB_PRISMATIC)"
#endif

namespace fddp {
namespace mb {

constexpr int kQsGroup = 8;      // lanes that share one column pair (rows l, l + 8, ...)
constexpr int kQsMaxPairs = 32;  // kMaxJ / 2 disjoint pairs per round
constexpr int kQsSweeps = 30;    // cap of the sweep loop: a knot that reaches it gets u = NaN
constexpr int kQsThreads = kQsGroup * kQsMaxPairs;  // the workgroup: every pair of a round at once
constexpr double kQsEps = 2.220446049250313e-16;

// leading dimension of the (p + 1) x nv array (one column per dof): odd, as lda_of
MB_HD __forceinline__ int qs_ldb(int p) { return (p + 1) | 1; }
// the small arrays after the recursions' partials: g, the zero velocity, ds/du (2 nu), the
// column norms; the pairs' partial sums, their rotation flags, the knot's flags
MB_HD __forceinline__ int64_t qs_small_doubles(int nj) {
  return pad2(5 * (int64_t)nj) + 3 * kQsThreads + kQsMaxPairs + 8;
}
// LDS (doubles) of knot_quasi_static_x for nj dofs, nc contact rows and nu controls.
MB_HD inline int64_t quasi_static_work_doubles(int nj, int nc, int nu) {
  return pad2(WVals::doubles(nj)) + part_doubles(nj) + qs_small_doubles(nj) + (int64_t)qs_ldb(nu + nc) * nj;
}

MB_HD __forceinline__ bool qs_finite(double v) { return v - v == 0.; }

// Round-robin tournament on n2 (even) players: pair k of round r (0 <= r < n2 - 1,
// 0 <= k < n2 / 2), lo < hi. Player n2 - 1 stays, the others rotate; every round's pairs are
// disjoint and every two players meet once per n2 - 1 rounds. A fixed order: it depends on
// nothing but nv, so the result repeats bit for bit.
MB_HD __forceinline__ void qs_pair(int n2, int r, int k, int& lo, int& hi) {
  const int m = n2 - 1;
  int a, c;
  if (k == 0) {
    a = r;
    c = m;
  } else {
    a = (r + k) % m;
    c = (r + m - k) % m;
  }
  lo = a < c ? a : c;
  hi = a < c ? c : a;
}

// u_out[0..nu) = quasiStatic(x) of the multibody Euler knot block P (free or contact dynamics;
// not an impulse knot, nu > 0). x: nq entries are read (the velocity is ignored, as in the
// reference), readable by every lane. Needs kQsThreads threads; every thread must call (the
// phases end in barriers, and the sweep loop's exit is uniform: it is decided from LDS values
// every lane reads alike). `w`: quasi_static_work_doubles(nj, nc, nu). A non-finite q, or a
// knot that has not converged after kQsSweeps sweeps, gives u = NaN.
template <class X>
MB_HD __forceinline__ void knot_quasi_static_x(const X& ex, const double* P, const double* x, double* u_out, double* w) {
  w = ex.lds(w);
  P = ex.lds(P);
  const Blk b = parse_uniform(P);
  const int nj = b.nj, nq = b.nq, nc = b.nc, nu = nj - b.nun, p = nu + nc, ldb = qs_ldb(p);
  double* parts = ex.lds(w + pad2(WVals::doubles(nj)));
  double* g = ex.lds(parts + part_doubles(nj));  // rnea(q, 0, 0)
  double* zv = g + nj;                           // the zero velocity
  double* ds = zv + nj;                          // squashed record: s(0) (nu), ds/du(0) (nu)
  double* nrm = ds + 2 * nj;                     // squared norms of the columns' top p rows
  double* red = ex.lds(g + pad2(5 * (int64_t)nj));  // per lane: its rows' share of (a.a, b.b, a.b)
  double* rot = red + 3 * kQsThreads;            // per pair slot: rotated in this sweep
  double* misc = rot + kQsMaxPairs;              // [0]: q is not finite
  double* Bm = ex.lds(misc + 8);                 // [A^T; g^T], column k (dof k) at Bm + ldb k
  double* Jc = parts;                            // nc x nj, once the recursions are done with their partials
  const WVals W{w, nj, parts};
  // the kinematics the RNEA and the contact Jacobians read (placements, motion subspaces, body
  // inertias): world_kinematics' first two phases; neither reads the CRBA's composites or M
  ex.run([&](int lane) {
    if (lane < nj) {
      w_joint_local(b, W, x, lane);
      zv[lane] = 0.;
    }
    if (lane < kQsMaxPairs) rot[lane] = 0.;
    if (lane == kQsMaxPairs) misc[0] = 0.;
    if (b.sq && lane < nu) squash_eval(b.sq, nu, lane, 0., ds, true);
  });
  ex.run([&](int lane) {
    if (lane < nj) {
      w_walk(b, W, lane);
      w_joint_world(b, W, lane);
    }
    for (int e = lane - 64; e >= 0 && e < nq; e += ex.nt)
      if (!qs_finite(x[e])) misc[0] = 1.;
  });
  world_rnea(ex, b, W, zv, nullptr, g);
  if (nc)
    ex.run([&](int lane) {
      if (lane < nj) contact_jac_lane(b, W, lane, Jc, nullptr);
    });
  // column i: row i of [D | Jc^T], then g_i. D = dtau/du at u = 0: [0_nun; I], S, or S diag(ds/du(0))
  ex.run([&](int lane) {
    for (int e = lane; e < nj * (p + 1); e += ex.nt) {
      const int i = e / (p + 1), r = e - i * (p + 1);
      double v;
      if (r < nu)
        v = b.S ? b.S[(int64_t)r * nj + i] * (b.sq ? ds[nu + r] : 1.) : (i - b.nun == r ? 1. : 0.);
      else if (r < p)
        v = Jc[(int64_t)(r - nu) * nj + i];
      else
        v = g[i];
      Bm[(int64_t)i * ldb + r] = v;
    }
  });
  const int npl = (nj + 1) >> 1, n2 = 2 * npl;  // pairs per round (an odd nv: one with the bye)
  const double epsf = (nj > p ? nj : p) * kQsEps;
  const int ngr = ex.nt / kQsGroup;
  double tol2 = 0.;
  bool conv = false;
#pragma unroll 1
  for (int sweep = 0; sweep <= kQsSweeps; ++sweep) {
    ex.run([&](int lane) {
      if (lane < nj) {
        const double* col = Bm + (int64_t)lane * ldb;
        double s = 0.;
        for (int r = 0; r < p; ++r) s += col[r] * col[r];
        nrm[lane] = s;
      }
    });
    // (every lane reads the same values: the exit below is uniform)
    double mx = 0.;
    for (int k = 0; k < nj; ++k) mx = nrm[k] > mx ? nrm[k] : mx;
    int nrot = 0;
    for (int k = 0; k < npl; ++k) nrot += rot[k] != 0. ? 1 : 0;
    // a column below the truncation threshold is noise: it takes part in no rotation (on a tall
    // A the p - rank noise columns would otherwise rotate against each other for ever)
    tol2 = (epsf * epsf) * mx;
    if (sweep > 0 && nrot == 0) {
      conv = true;
      break;
    }
    if (sweep == kQsSweeps) break;
#pragma unroll 1
    for (int r = 0; r < n2 - 1; ++r) {
      ex.run([&](int lane) {
        const int l = lane & (kQsGroup - 1);
        for (int k = lane / kQsGroup; k < npl; k += ngr) {
          int lo, hi;
          qs_pair(n2, r, k, lo, hi);
          if (hi >= nj) continue;  // the bye
          const double* ca = Bm + (int64_t)lo * ldb;
          const double* cb = Bm + (int64_t)hi * ldb;
          double sa = 0., sb = 0., sg = 0.;
          for (int row = l; row < p; row += kQsGroup) {
            const double va = ca[row], vb = cb[row];
            sa += va * va;
            sb += vb * vb;
            sg += va * vb;
          }
          double* o = red + 3 * (kQsGroup * k + l);
          o[0] = sa;
          o[1] = sb;
          o[2] = sg;
        }
      });
      ex.run([&](int lane) {
        const int l = lane & (kQsGroup - 1);
        for (int k = lane / kQsGroup; k < npl; k += ngr) {
          int lo, hi;
          qs_pair(n2, r, k, lo, hi);
          if (hi >= nj) continue;
          const double* o = red + 3 * kQsGroup * k;
          double al = 0., be = 0., ga = 0.;
          for (int e = 0; e < kQsGroup; ++e) {  // the group's partials, in lane order
            al += o[3 * e];
            be += o[3 * e + 1];
            ga += o[3 * e + 2];
          }
          const bool rotate = al > tol2 && be > tol2 && fabs(ga) > epsf * sqrt(al * be);
          if (l == 0) rot[k] = ((r > 0 && rot[k] != 0.) || rotate) ? 1. : 0.;
          if (!rotate) continue;
          const double zeta = (be - al) / (2. * ga);
          const double t = (zeta < 0. ? -1. : 1.) / (fabs(zeta) + sqrt(1. + zeta * zeta));
          const double c = 1. / sqrt(1. + t * t), s = c * t;
          double* ca = Bm + (int64_t)lo * ldb;
          double* cb = Bm + (int64_t)hi * ldb;
          for (int row = l; row <= p; row += kQsGroup) {  // (the last row, g's, rides along)
            const double va = ca[row], vb = cb[row];
            ca[row] = c * va - s * vb;
            cb[row] = s * va + c * vb;
          }
        }
      });
    }
  }
  bool bad = !conv || misc[0] != 0.;
  for (int k = 0; k < nj; ++k) bad = bad || !qs_finite(nrm[k]) || !qs_finite(Bm[(int64_t)k * ldb + p]);
  ex.run([&](int lane) {
    if (lane >= nu) return;
    double s = 0.;
    for (int k = 0; k < nj; ++k) {
      const double* col = Bm + (int64_t)k * ldb;
      if (nrm[k] > tol2) s += col[lane] * col[p] / nrm[k];
    }
    mb_gstore(u_out + lane, bad ? NAN : s);
  });
}

}  // namespace mb
}  // namespace fddp
