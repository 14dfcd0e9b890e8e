// Multibody knots on the device: IntegratedActionModelEuler ∘
// DifferentialAction{Free,Contact}FwdDynamics and ActionModelImpulseFwdDynamics
// (CostModelSum of State / Control / FramePlacement / FrameTranslation / CoMPosition /
// ContactForce costs) over a kinematic tree of revolute and prismatic joints below either the
// universe or a free-flyer root (StateMultibody on SE(3) x R^n).
//
// Reference: include/crocoddyl/core/integrator/euler.hxx:41-131,
//   multibody/actions/{free,contact,impulse}-fwddyn.hxx, multibody/costs/cost-sum.hxx:89-160,
//   multibody/costs/*.hxx, multibody/states/multibody.hxx:54-240; the rigid-body
//   arithmetic the reference takes from Pinocchio (aba, computeRNEADerivatives,
//   updateFramePlacement, getFrameJacobian, integrate / difference / dIntegrate /
//   dIntegrateTransport / dDifference, exp6, log6, Jexp6, Jlog6) is computed here as:
//   * forward dynamics: a = (M + diag(armature))^-1 (tau - nle), with RNEA and the
//     composite-rigid-body algorithm in world coordinates, where every recursion is
//     an ancestor / subtree sum evaluated one dof per lane (a free-flyer is six dofs
//     that share one body; a prismatic joint is a dof with S = [oR axis; 0] and the local
//     placement (Rpl, ppl + Rpl axis q), as the free-flyer's first three dofs: nothing below
//     the motion subspaces knows the joint type), and the solve by Gauss-Jordan with one
//     column per lane.
//     (The reference's default path is ABA, the same function.)
//   * derivatives: the world-frame analytic RNEA derivatives, one lane per tangent
//     direction (q_j or v_j): every world quantity of the subtree moved by q_j is
//     transported by the joint motion S_j, and what is left reduces to the
//     subtree composites (composite inertia, and P_k = sum_b dY_b-like terms), so
//     d tau_k / d q_j is a 6-vector dot product per pair (see dtau_direction);
//     da/dx = -Kinv (dtau/dx; da0/dx) as computeABADerivatives /
//     the contact KKT inverse (contact-fwddyn.hxx:127-140).
//   * frame-cost Jacobians: the frame's motion under S_j pushed through log6 in dual
//     numbers, which is Jlog6(rMf) * fJf (frame-placement.hxx:63-66);
//   * free-flyer state: M exp6(dq) with Eigen's quaternion extraction, log6(M0^-1 M1),
//     Jexp6 / Jlog6 columns in dual numbers, Ad(exp6(dq)^-1) (pinocchio's
//     SpecialEuclideanOperationTpl<3>).
// Parameter-block layout: include/fddp_hip.h (FDDP_KNOT_EULER_FREEFWD).
//
// The first sections are headers of their own, each of which compiles alone, included below
// in the order of their definitions; the later sections follow in this file:
//   mb_base.hpp     diagnostic hooks, stores / LDS accessors, constants, Blk and its parsers
//   mb_spatial.hpp  3-vectors, rotations, spatial algebra, joint records, quaternions
//   mb_solve.hpp    DevExec / HostExec, Gauss-Jordan family, gj_mfma, mb_solve, mb_invert
//   mb_se3.hpp      Dual, exp6 / log6, ff_integrate / ff_difference, Jexp6 / Jlog6 columns
//   mb_world.hpp    WVals, the world-value and RNEA / CRBA recursions
//   mb_costs.hpp    CRec, Act, residuals and activations, cost counting, contacts
//   (here)          mb_mfma and the tree-sparse LTDL; world_kinematics, world_rnea, euler_step
//                   and the knot calcs; the calcDiff: its derivation and LDS plan (DiffLayout,
//                   diff_layout, diff_spill and their check), the per-lane derivative pieces,
//                   the matrix-core products, knot_calc_diff_x / knot_calc_diff
#pragma once

#include "mb_base.hpp"
#include "mb_spatial.hpp"
#include "mb_solve.hpp"
#include "mb_se3.hpp"
#include "mb_world.hpp"
#include "mb_costs.hpp"

namespace fddp {
namespace mb {

// Placements, world quantities, composite inertias and M (into A, zeroed by
// the caller) for configuration q; `costs(wave, l)` runs on waves >= 1 in
// the phase after the kinematics (nullptr-like no-op allowed).
// `early(wave, l)` runs on waves >= 1 beside the local placements (work on x / u only).
#if defined(__HIP_DEVICE_COMPILE__)
// ---- fp64 matrix-core products (v_mfma_f64_16x16x4_f64) ---------------------------
// Fragment maps (MI355X guide, f64 16x16x4): A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15], C/D col = lane & 15, row = (lane >> 4) + 4 reg.
// Every wave of the workgroup takes 16 x 16 output tiles round-robin; loads outside
// the operands read as exact zeros, so padded rows / columns stay zero.
typedef double mb_f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mb_f64x4 mb_mfma(double a, double b, mb_f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
typedef __attribute__((address_space(3))) double mb_lds_d;
#endif

// ---- tree-sparse LTDL of the joint-space inertia (RBDA 6.3) ------------------------
// M (nj x nj, column-major at ld lda, both triangles as the CRBA writes them) has the
// branch-induced sparsity of the kinematic tree: M_ij != 0 only when i is an ancestor-
// or-self of j or j of i, in the dof tree whose parent of d is chain_parent(b, d) (the
// free-flyer's six dofs form a chain). Featherstone's LTDL factorisation M = L^T D L
// keeps L (unit lower triangular) on that pattern, and the reference's solvers reach
// M^-1 through Pinocchio's sparse Cholesky of M (contact-fwddyn.hxx:94,132: forwardDynamics
// / getKKTContactDynamicMatrixInverse; free-fwddyn.hxx:64: aba). A dof's row is final once
// all its descendants are eliminated, and dofs of one depth are never ancestor and
// descendant of each other, so a whole depth level is eliminated in one step, deepest
// first: the chain of dependent steps is the tree depth (16 on Talos) instead of the nj (38)
// pivots of a dense factorisation, and each step is one FMA per pattern entry.
// G = L^-1 (same pattern) follows level by level from the root, and
//   M^-1 = G D^-1 G^T,   M^-1 B = G (D^-1 (G^T B)),
// whose sums run over common ancestors only.
// Storage: L, then G, in place of M's lower triangle on the pattern, D on the diagonal;
// M's upper triangle is left as it was. The factorisation and G run on wave 0 alone
// (run_w0 steps, one wave-level fence per level); the products on the whole workgroup.
struct TreeWork {
  Mask* cm;      // nj: chain ancestors-or-self of each dof (index order = depth order)
  Mask* dsc;     // nj: strict descendants
  Mask* lev;     // 64: the dofs of each depth
  double* dinv;  // nj: 1 / D
  int* bad;      // set on a non-positive D (the LLT failure)
};
MB_HD __forceinline__ Mask chain_mask(const Blk& b, const WVals& W, int d) {
  return (b.ff && d < 6) ? ((Mask(2) << d) - 1) : *W.anc(d);
}
MB_HD __forceinline__ int mask_depth(Mask m) { return __builtin_popcountll(m) - 1; }
MB_HD __forceinline__ int mask_low(Mask m) { return __builtin_ctzll(m); }
// 1 / d to working precision: v_rcp_f64 corrected by x0 (1 + e + e^2), e = 1 - d x0
// (relative error e^3, as the blocked Gauss-Jordan's pivots)
MB_HD __forceinline__ double mb_recip(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double x0 = __builtin_amdgcn_rcp(d);
  const double e = __builtin_fma(-d, x0, 1.);
  return __builtin_fma(x0, __builtin_fma(e, e, e), x0);
#else
  return 1. / d;
#endif
}
// the tree's depth (uniform: every thread computes it from the ancestor masks)
MB_HD inline int tree_depth(const Blk& b, const WVals& W) {
  int md = 0;
  for (int k = 0; k < b.nj; ++k) {
    const int d = mask_depth(chain_mask(b, W, k));
    md = d > md ? d : md;
  }
  return md;
}
// M -> (L, D) in place, then L -> G = L^-1 in place; tw.dinv = 1 / D. md: tree_depth.
// The level steps as executor phases (the host emulation; the device for trees deeper
// than its register fast path, tree_ltdl_wave).
template <class X>
MB_HD inline void tree_ltdl_steps(const X& ex, const Blk& b, const WVals& W, double* A_, int lda, const TreeWork& tw,
                                  int md) {
  const int nj = b.nj;
  double* A = ex.lds(A_);
  ex.run_w0([&](int lane) {
    if (lane < nj) {
      const Mask c = chain_mask(b, W, lane);
      Mask d = 0;
      for (int k = lane + 1; k < nj; ++k) d |= ((chain_mask(b, W, k) >> lane) & 1ull) << k;
      tw.cm[lane] = c;
      tw.dsc[lane] = d;
    }
    Mask lv = 0;  // lane l: the dofs at depth l
    for (int k = 0; k < nj; ++k) lv |= Mask(mask_depth(chain_mask(b, W, k)) == lane ? 1 : 0) << k;
    tw.lev[lane] = lv;
    if (lane == 0) *tw.bad = 0;
  });
  // Level L, deepest first: (a) every row i above level L takes the contributions of its
  // descendants k at depth L (rows final since the deeper levels), H_ij -= H_ki H_kj / D_k
  // for j in the ancestors-or-self of i; (b) the rows of level L + 1 (final now) are
  // scaled to L_kj = H_kj / D_k. (a) reads the rows of level L and writes rows above it,
  // (b) rewrites the rows of level L + 1: no lane reads what another writes.
#pragma unroll 1
  for (int L = md; L >= -1; --L)
    ex.run_w0([&](int i) {
      if (i >= nj) return;
      const Mask ci = tw.cm[i];
      const int di = mask_depth(ci);
      if (di < L) {
        Mask km = tw.dsc[i] & tw.lev[L];
        while (km) {
          const int k = mask_low(km);
          km &= km - 1;
          const double f = A[k + lda * i] * mb_recip(A[k + lda * k]);
          Mask jm = ci;
          while (jm) {
            const int j = mask_low(jm);
            jm &= jm - 1;
            A[i + lda * j] -= f * A[k + lda * j];
          }
        }
      } else if (di == L + 1) {
        const double d = A[i + lda * i];
        const double inv = mb_recip(d);
        if (!(d > 0.)) *tw.bad = 1;
        tw.dinv[i] = inv;
        Mask jm = ci & ~(Mask(1) << i);
        while (jm) {
          const int j = mask_low(jm);
          jm &= jm - 1;
          A[i + lda * j] *= inv;
        }
      }
    });
  // G = L^-1: G_k = e_k - sum_{m in anc(k)} L_km G_m, level L from the root: row k (deeper
  // than L) takes the term of its ancestor m at depth L, whose row is final; position (k, m)
  // holds L_km until this step and G_km from it on.
#pragma unroll 1
  for (int L = 0; L < md; ++L)
    ex.run_w0([&](int k) {
      if (k >= nj) return;
      const Mask ck = tw.cm[k];
      if (mask_depth(ck) <= L) return;
      const int m = mask_low(ck & tw.lev[L]);
      const double l = A[k + lda * m];
      Mask im = ck & ((Mask(1) << m) - 1);
      while (im) {
        const int i = mask_low(im);
        im &= im - 1;
        A[k + lda * i] -= l * A[m + lda * i];
      }
      A[k + lda * m] = -l;
    });
  ex.sync();
}
constexpr int kTreeKD = 16;  // depth bound of the device fast path (below)
#if defined(__HIP_DEVICE_COMPILE__)
// Device fast path of tree_ltdl for trees of depth < kTreeKD, on wave 0 in one phase:
// lane i holds row i of the factor in registers, path-indexed (entry s = the column of
// i's ancestor at depth s; s = depth(i) the diagonal), so every update is a static-index
// register FMA; the rows other lanes need (a level's rows, then G's rows) go through LDS
// (PR: nj x kTreeKD), the levels and descendant sets are wave ballots, and one wave-level
// fence separates the levels. Same results as the generic steps up to the summation order
// of a row's contributions.
typedef __attribute__((address_space(3))) Mask mb_lds_mask;
typedef __attribute__((address_space(3))) int mb_lds_int;
__device__ __forceinline__ void tree_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// (the LDS operands arrive typed as LDS; the own row lives in registers during the
// elimination, then L in the row's LDS copy, so only G's row is in registers after it)
// (Inlined into the rollout kernel at its 256-VGPR cap it does not build: the register
// allocation trips the backend's "even aligned vector registers" check. The rollout takes
// the dense solve instead, k_fwd.hip MB_CALC_DENSE.)
__device__ __forceinline__ Mask readlane_mask(Mask v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return (Mask(hi) << 32) | lo;
}
__device__ __forceinline__ void tree_ltdl_wave(const mb_lds_mask* anc, int ff, int nj, mb_lds_d* A, int lda, int md,
                                               mb_lds_d* PR, mb_lds_d* dinv_out, mb_lds_int* bad_out) {
  // Written for the instruction stream of one wave: every register array index is static
  // (the levels are unrolled, so level L touches only the path entries s < L), the
  // level's dofs are a uniform (scalar) loop with their rows read as LDS broadcasts, and
  // every LDS access is unconditional within its lanes.
  constexpr int KD = kTreeKD;
  const int pld = md + 1;  // PR row stride (a row has depth + 1 <= md + 1 entries)
  MB_GJ_MARK(0);
  const int lane = (int)threadIdx.x & 63;
  const bool act = lane < nj;
  const int rl = act ? lane : 0;  // (inactive lanes read row 0 and store nothing)
  const Mask cmi = act ? ((ff && lane < 6) ? ((Mask(2) << lane) - 1) : anc[lane]) : Mask(1);
  const int di = act ? mask_depth(cmi) : -1;
  // the ancestors by depth (col[s], s <= di; col[di] = the dof itself; beyond: the dof)
  int col[KD];
  {
    Mask cur = cmi;
#pragma unroll
    for (int s = 0; s < KD; ++s) {
      const int c = (int)__builtin_ctzll(cur | (Mask(1) << 63));
      col[s] = c < nj ? c : rl;
      cur &= cur - 1;
    }
  }
  // row i of M, path-indexed (entries beyond the diagonal are never read)
  double R[KD];
#pragma unroll
  for (int s = 0; s < KD; ++s) R[s] = A[rl + lda * col[s]];
  mb_lds_d* pr = PR + pld * rl;
  MB_GJ_MARK(1);
  double dinv = 0.;
  bool bad = false;
  // the rows of depth L are final: stored for the level that reads them, with 1 / D
  // (L static: the diagonal is R[L], and the row has L + 1 entries)
  auto finalize = [&](auto Lc) __attribute__((always_inline)) {
    constexpr int L = decltype(Lc)::value;
    if (act && di == L) {
#pragma unroll
      for (int s = 0; s <= L; ++s) pr[s] = R[s];
      const double d = R[L];
      dinv = mb_recip(d);
      bad = bad || !(d > 0.);
      dinv_out[lane] = dinv;
    }
  };
  // (the deepest level: every row of depth md is final from the start)
#pragma unroll
  for (int s = 0; s < KD; ++s)
    if (act && di == md && s <= md) pr[s] = R[s];
  if (act && di == md) {
    double d = 0.;
#pragma unroll
    for (int s = 0; s < KD; ++s) d = s == di ? R[s] : d;
    dinv = mb_recip(d);
    bad = bad || !(d > 0.);
    dinv_out[lane] = dinv;
  }
  tree_wave_sync();
  MB_GJ_MARK(2);
  // elimination, deepest level first: row i takes the contributions of its descendants k
  // at depth L, H_is -= (H_ki / D_k) H_ks over the path entries s <= depth(i) < L
  auto level = [&](auto Lc) __attribute__((always_inline)) {
    constexpr int L = decltype(Lc)::value;
    if (L > md) return;
    Mask lev = __ballot(act && di == L);  // the dofs at depth L (uniform)
    const bool mine = act && di < L;
    while (lev) {
      const int k = mask_low(lev);
      lev &= lev - 1;
      const Mask ck = readlane_mask(cmi, k);
      if (mine && ((ck >> lane) & 1ull)) {
        const mb_lds_d* pk = PR + pld * k;
        const double f = pk[di] * dinv_out[k];
#pragma unroll
        for (int s = 0; s < L; ++s) R[s] = __builtin_fma(-f, pk[s], R[s]);
      }
    }
    finalize(std::integral_constant<int, L - 1>{});
    tree_wave_sync();
    MB_GJ_MARK(3 + md - L);
  };
  static_assert(KD == 16, "the levels below are unrolled for kTreeKD = 16");
  level(std::integral_constant<int, 15>{});
  level(std::integral_constant<int, 14>{});
  level(std::integral_constant<int, 13>{});
  level(std::integral_constant<int, 12>{});
  level(std::integral_constant<int, 11>{});
  level(std::integral_constant<int, 10>{});
  level(std::integral_constant<int, 9>{});
  level(std::integral_constant<int, 8>{});
  level(std::integral_constant<int, 7>{});
  level(std::integral_constant<int, 6>{});
  level(std::integral_constant<int, 5>{});
  level(std::integral_constant<int, 4>{});
  level(std::integral_constant<int, 3>{});
  level(std::integral_constant<int, 2>{});
  level(std::integral_constant<int, 1>{});
  MB_GJ_MARK(19);
  // L = row i / D_i below the diagonal (registers; the final row values are in R)
  double Lr[KD];
#pragma unroll
  for (int s = 0; s < KD; ++s) Lr[s] = R[s] * dinv;
  // G = L^-1 from the root: row k takes the term of its ancestor at depth t (whose G row,
  // final after step t - 1, is read from PR); the rows of depth t + 1 are final after step t
  double Gr[KD];
#pragma unroll
  for (int s = 0; s < KD; ++s) Gr[s] = 0.;
  tree_wave_sync();
#pragma unroll
  for (int t = 0; t < KD - 1; ++t) {
    if (t < md) {
      if (act && di > t) {
        const mb_lds_d* pm = PR + pld * col[t];
        double g[KD];
#pragma unroll
        for (int s = 0; s < t; ++s) g[s] = pm[s];
        const double l = Lr[t];
#pragma unroll
        for (int s = 0; s < t; ++s) Gr[s] = __builtin_fma(-l, g[s], Gr[s]);
        Gr[t] = -l;
        if (di == t + 1)
#pragma unroll
          for (int s = 0; s <= t; ++s) pr[s] = Gr[s];
      }
      tree_wave_sync();
    }
  }
  MB_GJ_MARK(20);
  // G below the diagonal into A's pattern entries (D stays on the diagonal)
  if (act)
#pragma unroll
    for (int s = 0; s < KD - 1; ++s)
      if (s < di) A[lane + lda * col[s]] = Gr[s];
  if (lane == 0) *bad_out = 0;
  tree_wave_sync();
  if (bad) *bad_out = 1;
  MB_GJ_MARK(21);
}
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// G's entry (r, m) from the dense storage tree_ltdl leaves (G below the diagonal on the
// pattern, exact zeros elsewhere below it, D on the diagonal: G_rr = 1), zero above the
// diagonal and outside nj
__device__ __forceinline__ double tree_gd(const mb_lds_d* A, int lda, int nj, int r, int m) {
  const bool in = r < nj && m < nj;
  const double v = A[in ? r + lda * m : 0];
  return (!in || m > r) ? 0. : (m == r ? 1. : v);
}
// Minv = G D^-1 G^T on the matrix cores: the upper 16 x 16 tiles, each entry with r <= c
// stored at (r, c) and (c, r) (exactly symmetric); a tile's k-range stops at the smaller
// block (G is lower triangular)
__device__ __forceinline__ void tree_minv_mfma(const double* A_, int lda, int nj, const double* dinv_, double* Mi_) {
  const mb_lds_d* A = (const mb_lds_d*)lds_ptr(A_);
  const mb_lds_d* dinv = (const mb_lds_d*)lds_ptr(dinv_);
  mb_lds_d* Mi = (mb_lds_d*)lds_ptr(Mi_);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  const int li = lane & 15, lk = lane >> 4, nt = (nj + 15) >> 4, ntiles = nt * (nt + 1) / 2;
#pragma unroll 1
  for (int tile = wave; tile < ntiles; tile += nw) {
    int ti = 0, rem = tile;
    while (rem >= nt - ti) {
      rem -= nt - ti;
      ++ti;
    }
    const int tj = ti + rem;
    const int r = 16 * ti + li, c = 16 * tj + li;
    const int kmax = 16 * ti + 16 < nj ? 16 * ti + 16 : nj;
    mb_f64x4 acc0 = {0., 0., 0., 0.}, acc1 = {0., 0., 0., 0.};  // two chains (even / odd k-steps)
#pragma unroll 2
    for (int kb = 0; kb < kmax; kb += 8) {
      const int m0 = kb + lk, m1 = kb + 4 + lk;
      const double w0 = m0 < nj ? dinv[m0] : 0., w1 = m1 < nj ? dinv[m1] : 0.;
      acc0 = mb_mfma(tree_gd(A, lda, nj, r, m0), tree_gd(A, lda, nj, c, m0) * w0, acc0);
      if (kb + 4 < kmax) acc1 = mb_mfma(tree_gd(A, lda, nj, r, m1), tree_gd(A, lda, nj, c, m1) * w1, acc1);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * ti + lk + 4 * q, col = 16 * tj + li;
      const double v = acc0[q] + acc1[q];
      if (row < nj && col < nj && row <= col) {
        Mi[row + lda * col] = v;
        Mi[col + lda * row] = v;
      }
    }
  }
}
// The right-hand sides B (nj x nb at A + lda nj) -> M^-1 B in place on the matrix cores:
// T = D^-1 G^T B (T: nj x nb, ld nj), a workgroup barrier, X = G T. Every thread calls.
__device__ __forceinline__ void tree_solve_mfma(const double* A_, int lda, int nj, int nb, const double* dinv_,
                                                double* T_) {
  const mb_lds_d* A = (const mb_lds_d*)lds_ptr(A_);
  const mb_lds_d* dinv = (const mb_lds_d*)lds_ptr(dinv_);
  mb_lds_d* T = (mb_lds_d*)lds_ptr(T_);
  mb_lds_d* B = (mb_lds_d*)lds_ptr(A_ + (int64_t)lda * nj);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  const int li = lane & 15, lk = lane >> 4, tr = (nj + 15) >> 4, tc = (nb + 15) >> 4;
  // T tile (tm, tcc): rows m, k over r >= 16 tm
#pragma unroll 1
  for (int tile = wave; tile < tr * tc; tile += nw) {
    const int tm = tile / tc, tcc = tile - tm * tc;
    const int m = 16 * tm + li, c = 16 * tcc + li;
    mb_f64x4 acc0 = {0., 0., 0., 0.}, acc1 = {0., 0., 0., 0.};
#pragma unroll 2
    for (int kb = 16 * tm; kb < nj; kb += 8) {
      const int r0 = kb + lk, r1 = kb + 4 + lk;
      const double b0 = (r0 < nj && c < nb) ? B[r0 + lda * c] : 0.;
      const double b1 = (r1 < nj && c < nb) ? B[r1 + lda * c] : 0.;
      acc0 = mb_mfma(tree_gd(A, lda, nj, r0, m), b0, acc0);
      if (kb + 4 < nj) acc1 = mb_mfma(tree_gd(A, lda, nj, r1, m), b1, acc1);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * tm + lk + 4 * q, col = 16 * tcc + li;
      if (row < nj && col < nb) T[row + nj * col] = (acc0[q] + acc1[q]) * dinv[row];
    }
  }
  __syncthreads();
  // X tile (tr_, tcc): rows r, k over m <= 16 tr_ + 15
#pragma unroll 1
  for (int tile = wave; tile < tr * tc; tile += nw) {
    const int ti = tile / tc, tcc = tile - ti * tc;
    const int r = 16 * ti + li, c = 16 * tcc + li;
    const int kmax = 16 * ti + 16 < nj ? 16 * ti + 16 : nj;
    mb_f64x4 acc0 = {0., 0., 0., 0.}, acc1 = {0., 0., 0., 0.};
#pragma unroll 2
    for (int kb = 0; kb < kmax; kb += 8) {
      const int m0 = kb + lk, m1 = kb + 4 + lk;
      const double t0 = (m0 < nj && c < nb) ? T[m0 + nj * c] : 0.;
      const double t1 = (m1 < nj && c < nb) ? T[m1 + nj * c] : 0.;
      acc0 = mb_mfma(tree_gd(A, lda, nj, r, m0), t0, acc0);
      if (kb + 4 < kmax) acc1 = mb_mfma(tree_gd(A, lda, nj, r, m1), t1, acc1);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * ti + lk + 4 * q, col = 16 * tcc + li;
      if (row < nj && col < nb) B[row + lda * col] = acc0[q] + acc1[q];
    }
  }
  __syncthreads();
}
#endif
// M -> (L, D) -> G = L^-1 in place, tw.dinv = 1 / D (tree_ltdl_steps / tree_ltdl_wave).
// PR: (md + 1) * nj doubles of scratch (the device fast path's rows; the generic steps
// use tw.cm / tw.dsc instead, so the two may share their space).
// Independent work of the caller for the waves the factorisation leaves idle: side(slot,
// lane, nlanes) on waves >= 1 (lane counted from wave 1), slots 0 .. nslots - 1 one after
// another, the side waves meeting at an LDS counter (ctr, zeroed by the caller in an
// earlier phase) between slots. Without the device fast path the slots run afterwards as
// ordinary phases.
struct TreeNoSide {
  MB_HD void operator()(int, int, int) const {}
};
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void tree_side_barrier(int* ctr_, int target) {
  mb_lds_int* ctr = (mb_lds_int*)lds_ptr(ctr_);
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (__hip_atomic_load(ctr, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
}
#endif
template <class X, class Side = TreeNoSide>
MB_HD __forceinline__ void tree_ltdl(const X& ex, const Blk& b, const WVals& W, double* A, int lda, const TreeWork& tw,
                                     int md, double* PR, Side side = Side{}, int nslots = 0, int* ctr = nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (md < kTreeKD) {
    double* const Al = ex.lds(A);
    double* const PRl = ex.lds(PR);
    ex.run([&](int tid) {
      if (tid < 64) {
        tree_ltdl_wave((const mb_lds_mask*)ex.lds(W.anc(0)), b.ff ? 1 : 0, b.nj, (mb_lds_d*)Al, lda, md,
                       (mb_lds_d*)PRl, (mb_lds_d*)ex.lds(tw.dinv), (mb_lds_int*)ex.lds(tw.bad));
      } else if (nslots > 0) {
        const int sl = tid - 64, snt = ex.nt - 64;
#pragma unroll 1
        for (int slot = 0; slot < nslots; ++slot) {
          if (slot > 0) tree_side_barrier(ctr, (snt >> 6) * slot);
          side(slot, sl, snt);
        }
      }
    });
    return;
  }
#endif
  (void)PR;
  tree_ltdl_steps(ex, b, W, A, lda, tw, md);
  for (int slot = 0; slot < nslots; ++slot)
    ex.run([&](int lane) {
      if (lane >= 64) side(slot, lane - 64, ex.nt - 64);
    });
}
// G's entry (r, m), m an ancestor-or-self of r (the diagonal holds D: G_rr = 1)
MB_HD __forceinline__ double tree_g(const double* A, int lda, int r, int m) { return m == r ? 1. : A[r + lda * m]; }
// Minv (ld lda) = G D^-1 G^T from tree_ltdl, exactly symmetric (the sum for (r, c) and
// (c, r) has the same terms in the same order). Returns false on a non-positive pivot.
// (device: on the matrix cores, tree_minv_mfma)
template <class X>
MB_HD inline bool tree_minv(const X& ex, const Blk& b, const double* A_, int lda, const TreeWork& tw, double* Mi_) {
#if defined(__HIP_DEVICE_COMPILE__)
  ex.run([&](int) { tree_minv_mfma(A_, lda, b.nj, tw.dinv, Mi_); });
  return *tw.bad == 0;
#endif
  const int nj = b.nj;
  const double* A = ex.lds(A_);
  double* Mi = ex.lds(Mi_);
  ex.run([&](int lane) {
    for (int e = lane; e < nj * nj; e += ex.nt) {
      const int c = e / nj, r = e - nj * c;
      Mask mm = tw.cm[r] & tw.cm[c];
      double s = 0.;
      while (mm) {
        const int m = mask_low(mm);
        mm &= mm - 1;
        s += (tree_g(A, lda, r, m) * tree_g(A, lda, c, m)) * tw.dinv[m];
      }
      Mi[r + lda * c] = s;
    }
  });
  return *tw.bad == 0;
}
// B (nj x nb at A + lda nj, ld lda: the right-hand sides beside M) -> M^-1 B in place,
// through T = D^-1 G^T B (nj x nb, ld nj). Returns false on a non-positive pivot.
template <class X>
MB_HD inline bool tree_solve(const X& ex, const Blk& b, double* A_, int lda, int nb, const TreeWork& tw, double* T_) {
#if defined(__HIP_DEVICE_COMPILE__)
  ex.run([&](int) { tree_solve_mfma(A_, lda, b.nj, nb, tw.dinv, T_); });
  return *tw.bad == 0;
#endif
  const int nj = b.nj;
  double* A = ex.lds(A_);
  double* T = ex.lds(T_);
  double* B = A + (int64_t)lda * nj;
  ex.run([&](int lane) {
    for (int e = lane; e < nj * nb; e += ex.nt) {
      const int c = e / nj, m = e - nj * c;
      const double* bc = B + (int64_t)lda * c;
      Mask rm = tw.dsc[m];
      double s0 = bc[m], s1 = 0.;  // (two partial sums: the root's row has nj terms)
      while (rm) {
        const int r = mask_low(rm);
        rm &= rm - 1;
        s0 += A[r + lda * m] * bc[r];
        if (!rm) break;
        const int r2 = mask_low(rm);
        rm &= rm - 1;
        s1 += A[r2 + lda * m] * bc[r2];
      }
      T[m + nj * c] = (s0 + s1) * tw.dinv[m];
    }
  });
  ex.run([&](int lane) {
    for (int e = lane; e < nj * nb; e += ex.nt) {
      const int c = e / nj, r = e - nj * c;
      const double* tc = T + (int64_t)nj * c;
      Mask mm = tw.cm[r] & ~(Mask(1) << r);
      double s = tc[r];
      while (mm) {
        const int m = mask_low(mm);
        mm &= mm - 1;
        s += A[r + lda * m] * tc[m];
      }
      B[r + (int64_t)lda * c] = s;
    }
  });
  return *tw.bad == 0;
}

template <class X, class EarlyF, class CostF>
MB_HD inline void world_kinematics(const X& ex, const Blk& b, const WVals& W, const double* q, double* A, int lda,
                                   EarlyF early, CostF costs, bool world_composite = false) {
  const int nj = b.nj;
  ex.run([&](int lane) {
    if (lane < nj) w_joint_local(b, W, q, lane);
    if (lane >= 64) early(lane >> 6, lane & 63);
  });
  ex.run([&](int lane) {
    if (lane < nj) {
      w_walk(b, W, lane);
      w_joint_world(b, W, lane);
    }
  });
  // CRBA about each column's joint: the subtree composites in wave partials (beside them,
  // the cost records on waves >= 1), then the columns (rows split over all the waves); with
  // `world_composite` (the calcDiff) the columns' lanes also store the subtree composites
  // about the world origin
  const int npw = part_waves(ex.nt);
  ex.run([&](int lane) {
    const int w = lane >> 6, j = lane & 63;
    if (j < nj && w < npw) w_crba_composite_part(b, W, j, w, npw);
    if (w >= 1) costs(w, j);
  });
  ex.run([&](int lane) {
    const int w = lane >> 6, j = lane & 63;
    if (j < nj) w_crba_column(b, W, j, A, lda, w, ex.nt >> 6, npw, world_composite);
  });
}

// Joint torques of RNEA(q, qd, qdd) (qdd == nullptr: 0) with the kinematics in W;
// fx (6 per dof, world frame at the origin, may be null): external forces,
// as pinocchio::rnea(model, data, q, v, a, fext).
template <class X>
MB_HD inline void world_rnea(const X& ex, const Blk& b, const WVals& W, const double* qd, const double* qdd,
                             double* tau, const double* fx = nullptr) {
  const int nj = b.nj, nw = part_waves(ex.nt);
  // every ancestor / subtree sum split over the waves (w_*_part), combined by lane i
  ex.run([&](int lane) {
    const int w = lane >> 6, i = lane & 63;
    if (i < nj && w < nw) w_velocity_part(W, qd, i, w, nw);
  });
  ex.run([&](int lane) {
    if (lane < nj) w_velocity_accel_term(W, qd, qdd, lane, nw);
  });
  ex.run([&](int lane) {
    const int w = lane >> 6, i = lane & 63;
    if (i < nj && w < nw) w_accel_part(W, i, w, nw);
  });
  ex.run([&](int lane) {
    if (lane < nj) w_accel_body_force(W, lane, nw, fx);
  });
  ex.run([&](int lane) {
    const int w = lane >> 6, i = lane & 63;
    if (i < nj && w < nw) w_force_part(W, i, w, nw);
  });
  ex.run([&](int lane) {
    if (lane < nj) w_joint_force_comb(W, tau, lane, nw);
  });
}

// Euler step of the state (euler.hxx:64-68 + StateMultibody::integrate): lane i < nj
// writes v_next[i] and the configuration entries of dof i (lane 0 the free-flyer's
// seven: M exp6(v dt + a dt^2)). a: the acceleration (every lane reads a[0..5]).
MB_HD inline void euler_step(const Blk& b, const double* x, const double* a, double dt, double* xnext, int i) {
  const int nq = b.nq;
  const double v = x[nq + i], ai = a[i];
  xnext[nq + i] = v + ai * dt;
  if (b.ff && i < 6) {
    if (i == 0) {
      double dq[6];
      for (int e = 0; e < 6; ++e) dq[e] = x[nq + e] * dt + a[e] * (dt * dt);
      ff_integrate(x, dq, xnext);
    }
  } else {
    const int qi = qof(b, i);
    xnext[qi] = x[qi] + (v * dt + ai * dt * dt);
  }
}

// LDS (doubles) of the calc scratch for nj dofs and nc contact rows.
MB_HD inline int64_t calc_work_doubles(int nj, int nc = 0) {
  return pad2(WVals::doubles(nj)) + (int64_t)lda_of(nj) * (nj + nc + 1) + 2 * nj + kMaxCosts + 8 + (int64_t)nc * nj + nc +
         (int64_t)nc * (nc + 1) + 128 + part_doubles(nj);
}

// The calc's cost records other than the wide ones (knot_calc_x): record item i on lane
// i / 3 of side wave i % 3 (sl: the lane counted from the first side wave, snt: the side
// lanes), each record's weighted value into cv[k]. It rebuilds the block's views from the
// LDS pointers. (With tree_ltdl_wave it is inlined into knot_calc_x, which therefore does not
// build at the rollout's register cap: the rollout runs knot_calc_dense_x.)
MB_HD __forceinline__ void calc_cost_records(const double* P_, double* w_, double* parts_, const double* x_,
                                             const double* ub_, double* cv_, int sl, int snt) {
  const double* P = mb_lds(P_);
  const Blk b = parse_uniform(P);
  const WVals W{mb_lds(w_), b.nj, mb_lds(parts_)};
  const double* x = mb_lds(x_);
  const double* ub = mb_lds(ub_);
  double* cv = mb_lds(cv_);
  const int nu = b.nj - b.nun, nc = b.nc;
  const bool imp = b.impulse;
  const int nsw = snt >> 6, item = nsw * (sl & 63) + (sl >> 6);
  const double* cr = b.C;
  int nn = 0, nw = 0;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    if (wide_cost(C, nw)) {
      ++nw;
    } else {
      if (item == nn) {
        const bool vc = C.type() == C_FRAME_VELOCITY || C.type() == C_CENTROIDAL_MOMENTUM;
        double v = vc && imp ? 0. : cost_activation(b, W, C, x, ub, nu);
        if (force_cost(C.type()) && nc == 0) v = force_cost_activation(b, C, nullptr, nu);
        cv[k] = C.weight() * v;
      }
      ++nn;
    }
    cr += C.size();
  }
}

// model->calc(data, x, u) for the Euler∘FreeFwdDynamics knot (euler.hxx:41-80,
// free-fwddyn.hxx:44-79): a = (M + diag(armature))^-1 (u - nle) in world frame;
// with contacts, Euler∘ContactFwdDynamics (contact-fwddyn.hxx:59-104):
// pinocchio::forwardDynamics by the Schur complement,
//   [Y | z] = M^-1 [Jc^T | tau - nle],  S = Jc Y + damping I,
//   lambda = -S^-1 (Jc z + a0),  a = z + Y lambda.
// Needs >= 256 threads (4 waves): independent work of one phase runs on
// different waves (divergent lanes of one wave would serialise) — wave 0 the
// recursions and composite inertias, waves 1-3 the cost records (state / control residuals row-parallel).
// Every thread must call (phases end in barriers). x, u readable by all lanes;
// writes xnext[0..nx) and returns the knot cost. `w`: calc_work_doubles(nj, nc).
template <class X>
MB_HD __forceinline__ double knot_calc_x(const X& ex, const double* P, int nx, const double* x, const double* u, bool use_u,
                                double* xnext, double* w) {
  w = ex.lds(w);  // the work area and the parameter block live in LDS
  P = ex.lds(P);
  const Blk b = parse_uniform(P);
  const bool imp = b.impulse;  // impulse: [M | Jc^T] only, z = v
  const int nj = b.nj, nq = b.nq, nc = b.nc, nu = nj - b.nun, ncol = imp ? nj + nc : nj + nc + 1;
  const int lda = lda_of(nj);
  double* A = w + pad2(WVals::doubles(nj));  // nj x (nj + nc + 1), ld lda: [M | Jc^T | tau - nle]
  double* tau = A + (int64_t)lda * ncol;
  double* ub = tau + nj;  // u (zero if !use_u)
  double* cv = ub + nj;   // per-cost activations
  double* red = cv + kMaxCosts;
  int* flag = (int*)(red + 2);
  double* Jc = red + 8;                  // nc x nj
  double* a0 = Jc + (int64_t)nc * nj;    // nc
  double* S = a0 + nc;                   // nc x (nc + 1), ld nc: [S | Jc z + a0]
  double* pb = S + (int64_t)nc * (nc + 1);  // Gauss-Jordan pivot-column buffer (128)
  const WVals W{w, nj, pb + 128};            // the recursions' per-wave partials after it
  ex.run([&](int lane) {
    if (lane < nu) ub[lane] = use_u ? u[lane] : 0.;
#if MB_ACTUATION
    // (a squashed record: s(u) once per knot, into xnext, which is not written before the last phase)
    if (b.sq && lane < nu) squash_eval(b.sq, nu, lane, use_u ? u[lane] : 0., xnext, false);
#endif
    for (int e = lane; e < lda * ncol; e += ex.nt) A[e] = 0.;
  });
  // the wide records (state / control residuals: x, u only) row-parallel on waves 3 and 1
  // beside the local placements, their lane partials into pb (free until the
  // factorisation); the other records on the waves the factorisation leaves idle (below)
  world_kinematics(ex, b, W, x, A, lda, [&](int wave, int l) {
    const double* cr = b.C;
    int nw = 0;
    for (int k = 0; k < b.ncost; ++k) {
      const CRec C{cr};
      if (wide_cost(C, nw)) {
        if (wave == (nw == 0 ? 3 : 1)) pb[64 * nw + l] = cost_activation_part(b, C, x, ub, nu, l, 64);
        ++nw;
      }
      cr += C.size();
    }
  }, [&](int wave, int l) {
    // (dense solve: the other records but the frame velocities first,) the contacts'
    // position terms (log6 for the 6D ones): item i on lane i / 3 of wave 1 + i % 3, so
    // that no wave runs two of them (a wave pays for the sum of its divergent lanes' paths)
    if (wave > 3) return;
    const int item = 3 * l + (wave - 1);
    const int kc = item;
    if (!imp && kc >= 0 && kc < b.ncon) {
      int row0;
      const CRec C{contact_rec(b, kc, &row0)};
      contact_a0_position(b, W, C, a0 + row0);
    }
  });
  if (!imp) world_rnea(ex, b, W, x + nq, nullptr, tau);
  ex.run([&](int lane) {
    if (lane < nj) {
#if MB_ACTUATION
      const double ti = act_tau(b, b.sq ? xnext : ub, lane);  // tau = [0_nun; u], or S u / S s(u) with an actuation record
#else
      const double ti = act_tau(b, ub, lane);  // tau = [0_nun; u]
#endif
      if (!imp) A[(int64_t)lda * (nj + nc) + lane] = ti - tau[lane];
      if (nc) contact_jac_lane(b, W, lane, Jc, A, lda);
    }
    if (!imp && lane >= 64 && lane < 64 + b.ncon) {
      int row0;
      const CRec C{contact_rec(b, lane - 64, &row0)};
      contact_a0_drift(b, W, C, a0 + row0);
    }
    if (lane == 128) {  // the wide records' values from their lane partials (pb is the
                        // factorisation's scratch next)
      const double* cr = b.C;
      int nw = 0;
      for (int k = 0; k < b.ncost; ++k) {
        const CRec C{cr};
        if (wide_cost(C, nw)) {
          double a = 0.;
          for (int l = 0; l < 64; ++l) a += pb[64 * nw + l];
          cv[k] = C.weight() * (0.5 * a);
          ++nw;
        }
        cr += C.size();
      }
    }
  });
  // Every other record's weighted value into cv[k], on the waves the factorisation leaves
  // idle: record item i on lane i / 3 of side wave i % 3 (the frame placements / CoM are
  // long serial evaluations, which would otherwise sit on the knot's critical path); the
  // force costs without active contact rows (lambda = 0) here, with contacts after the
  // Schur solve; frame velocities with the body velocities (impulse knots: rejected by the
  // host). The knot cost is their sum in record order (cost-sum.hxx:89-117), at the end.
  auto cost_side = [&](int, int sl, int snt) { calc_cost_records(P, w, W.parts, x, ub, cv, sl, snt); };
  // [Y | z] = M^-1 [Jc^T | tau - nle] by the tree-sparse LTDL of M; its scratch: the depth
  // levels in pb, the dof masks, 1 / D and the intermediate D^-1 G^T B in the recursions'
  // per-wave partials (dead from here on)
  double* const tp = ex.lds(W.parts);
  const TreeWork tw{(Mask*)tp, (Mask*)tp + nj, (Mask*)ex.lds(pb), tp + 2 * nj, ex.lds(flag)};
  // (the device fast path's rows, then D^-1 G^T B, both after the masks and 1 / D)
  tree_ltdl(ex, b, W, A, lda, tw, tree_depth(b, W), tp + 3 * nj, cost_side, 1);
  bool ok = tree_solve(ex, b, A, lda, ncol - nj, tw, tp + 3 * nj);
  // z, then a (impulse: v+, in tau's slot; z = M^-1 M v = v)
  double* a = imp ? tau : A + (int64_t)lda * (nj + nc);
  if (nc > 0) {
    ex.run([&](int lane) {
      for (int e = lane; e < nc * (nc + 1); e += ex.nt) {
        const int col = e / nc, row = e % nc;
        // column col of Y, or z (impulse: v, and the restitution term r Jc v)
        const double* yc = (imp && col == nc) ? x + nq : A + (int64_t)lda * (nj + col);
        double s = 0.;
        for (int i = 0; i < nj; ++i) s += Jc[(int64_t)row * nj + i] * yc[i];
        S[e] = col < nc ? s + (row == col ? b.damping : 0.) : (imp ? (1. + b.r_coeff) * s : s + a0[row]);
      }
    });
    ok = gauss_jordan<1>(ex, S, nc, nc, nc + 1, flag, pb) && ok;
    ex.run([&](int lane) {
      // contact-force costs (lambda = -S^-1 r, in S's last column, negated): record k's
      // value on lane 64 + k into cv[k], summed in record order with the next phase
      const int kf = lane - 64;
      if (kf >= 0 && kf < b.ncost) {
        const double* cr = b.C;
        for (int k = 0; k < kf; ++k) cr += CRec{cr}.size();
        const CRec C{cr};
        if (force_cost(C.type())) {
          // lambda = -S's last column, read where it lies (no private copy)
          const double* Sl = S + (int64_t)nc * nc;
          cv[kf] = C.weight() * force_cost_activation_at(b, C, [Sl](int k) { return -Sl[k]; }, nu);
        }
      }
      if (lane >= nj) return;
      double s = imp ? x[nq + lane] : a[lane];
      for (int k = 0; k < nc; ++k) s -= A[(int64_t)lda * (nj + k) + lane] * S[(int64_t)nc * nc + k];
      a[lane] = s;
    });
  }
#if MB_CALC_IMPULSE_COM
  if (has_impulse_com(b)) {  // CostModelImpulseCoM: r = Jcom (v+ - v), from v+ (in a)
    ex.run([&](int lane) { impulse_com_calc_bodies(b, W, x, a, lane); });
    ex.run([&](int lane) { impulse_com_calc_value(b, W, cv, lane); });
  }
#endif
  const double dt = b.dt;
  if (!ok)  // a singular mass matrix / Schur complement surfaces as forward_error
    ex.run([&](int i) {
      if (i < nj) a[i] = NAN;
    });
  ex.run([&](int i) {
    if (i == 64) {  // the knot cost: the records' values in record order
      double total = 0.;
      for (int k = 0; k < b.ncost; ++k) total += cv[k];
      red[0] = total;
    }
    if (i >= nj) return;
    if (imp) {  // impulse-fwddyn.hxx:80-81: xnext = (q, v+)
      xnext[nq + i] = nc > 0 ? a[i] : x[nq + i];
      if (!ok) xnext[nq + i] = NAN;
      xnext[i] = x[i];
      if (i == nj - 1 && b.ff) xnext[nq - 1] = x[nq - 1];
      return;
    }
    if (dt != 0.) {
      euler_step(b, x, a, dt, xnext, i);
    } else {
      xnext[i] = x[i];
      xnext[nq + i] = x[nq + i];
      if (i == nj - 1 && b.ff) xnext[nq - 1] = x[nq - 1];
    }
  });
  const double cc = red[0];
  (void)nx;
  return dt != 0. ? dt * cc : cc;
}

// LDS (doubles) of the rollout's calc (knot_calc_dense_x): the L records, the small arrays,
// then one region that first holds the D records and the recursions' partials and, from the
// CRBA columns on, [M | Jc^T | tau - nle], Jc and the Schur block.
MB_HD inline int64_t calc_dense_doubles(int nj, int nc = 0) {
  const int64_t small = 2 * nj + kMaxCosts + 8 + nc + 128;
  const int64_t rec = WVals::dsize(nj) + part_doubles(nj);
  const int64_t fac = (int64_t)lda_of(nj) * (nj + nc + 1) + (int64_t)nc * nj + (int64_t)nc * (nc + 1);
  return WVals::lsize(nj) + pad2(small) + pad2(rec > fac ? rec : fac);
}

// model->calc as knot_calc_x, with the dense factorisation (the blocked Gauss-Jordan of
// gj_mfma on [M | Jc^T | tau - nle]) and a smaller LDS footprint: the rollout's workgroups
// share a CU three at a time on the C5 walk (calc_dense_doubles: 40 KB against
// calc_work_doubles' 60 KB). The phases run in the order
//   local placements | walk, world frames | RNEA (tau = nle) | CRBA composites + cost records |
//   composites stored | CRBA columns into A | Jc, a0, tau column | solve | Schur | a, xnext
// so that the D records and the partials are dead when the columns write A over them.
// Every value is formed by the same arithmetic as in knot_calc_x's dense solve of round 5.
template <class X>
MB_HD __forceinline__ double knot_calc_dense_x(const X& ex, const double* P, int nx, const double* x, const double* u,
                                               bool use_u, double* xnext, double* w) {
  w = ex.lds(w);
  P = ex.lds(P);
  const Blk b = parse_uniform(P);
  const bool imp = b.impulse;  // impulse: [M | Jc^T] only, z = v
  const int nj = b.nj, nq = b.nq, nc = b.nc, nu = nj - b.nun, ncol = imp ? nj + nc : nj + nc + 1;
  const int lda = lda_of(nj);
  double* tau = w + WVals::lsize(nj);
  double* ub = tau + nj;  // u (zero if !use_u)
  double* cv = ub + nj;   // per-cost activations
  double* red = cv + kMaxCosts;
  int* flag = (int*)(red + 2);
  double* a0 = red + 8;     // nc
  double* pb = a0 + nc;     // the wide records' lane partials; the Schur block's pivot buffer
  double* R2 = w + WVals::lsize(nj) + pad2(2 * nj + kMaxCosts + 8 + nc + 128);
  const WVals W{w, nj, R2 + WVals::dsize(nj), R2};
  double* A = R2;                          // from the columns on: nj x ncol, ld lda
  double* Jc = A + (int64_t)lda * ncol;    // nc x nj
  double* S = Jc + (int64_t)nc * nj;       // nc x (nc + 1), ld nc: [S | Jc z + a0]
  const int npw = part_waves(ex.nt);
  ex.run([&](int lane) {
    if (lane < nu) ub[lane] = use_u ? u[lane] : 0.;
#if MB_ACTUATION
    // (a squashed record: s(u) once per knot, into xnext, which is not written before the last phase)
    if (b.sq && lane < nu) squash_eval(b.sq, nu, lane, use_u ? u[lane] : 0., xnext, false);
#endif
  });
  // local placements; the wide records (state / control residuals: x, u only) row-parallel
  // on waves 3 and 1, their lane partials into pb
  ex.run([&](int lane) {
    if (lane < nj) w_joint_local(b, W, x, lane);
    if (lane >= 64) {
      const int wave = lane >> 6, l = lane & 63;
      const double* cr = b.C;
      int nw = 0;
      for (int k = 0; k < b.ncost; ++k) {
        const CRec C{cr};
        if (wide_cost(C, nw)) {
          if (wave == (nw == 0 ? 3 : 1)) pb[64 * nw + l] = cost_activation_part(b, C, x, ub, nu, l, 64);
          ++nw;
        }
        cr += C.size();
      }
    }
  });
  ex.run([&](int lane) {
    if (lane < nj) {
      w_walk(b, W, lane);
      w_joint_world(b, W, lane);
    }
  });
  if (!imp) world_rnea(ex, b, W, x + nq, nullptr, tau);
  // CRBA composites in wave partials; beside them, on waves 1-3, the other cost records
  // (force costs without active contact rows: lambda = 0; frame velocities: impulse knots
  // skip them, as the host rejects them there) and the contacts' position terms (log6 for the
  // 6D ones): item i on lane i / 3 of wave 1 + i % 3, so that no wave runs two of them
  ex.run([&](int lane) {
    const int wave = lane >> 6, l = lane & 63;
    if (l < nj && wave < npw) w_crba_composite_part(b, W, l, wave, npw);
    if (wave < 1 || wave > 3) return;
    const int item = 3 * l + (wave - 1);
    int nn = 0;
    const double* cr = b.C;
    int nw = 0;
    for (int k = 0; k < b.ncost; ++k) {
      const CRec C{cr};
      if (wide_cost(C, nw)) {
        ++nw;
      } else {
        if (item == nn) {
          double v = cost_activation(b, W, C, x, ub, nu, !imp);
          if (force_cost(C.type()) && nc == 0) v = force_cost_activation(b, C, nullptr, nu);
          cv[k] = C.weight() * v;
        }
        ++nn;
      }
      cr += C.size();
    }
    const int kc = item - nn;
    if (!imp && kc >= 0 && kc < b.ncon) {
      int row0;
      const CRec C{contact_rec(b, kc, &row0)};
      contact_a0_position(b, W, C, a0 + row0);
    }
  });
  ex.run([&](int lane) {
    if (lane < nj) w_crba_store_local(W, nj, lane, npw);
  });
  // (from here on the D records and the partials are dead: A, Jc, S over them)
  ex.run([&](int lane) {
    const int wv = lane >> 6, j = lane & 63;
    if (j < nj) w_crba_column(b, W, j, A, lda, wv, ex.nt >> 6, npw, false, true);
  });
  ex.run([&](int lane) {
    if (lane < nj) {
#if MB_ACTUATION
      const double ti = act_tau(b, b.sq ? xnext : ub, lane);  // tau = [0_nun; u], or S u / S s(u) with an actuation record
#else
      const double ti = act_tau(b, ub, lane);  // tau = [0_nun; u]
#endif
      if (!imp) A[(int64_t)lda * (nj + nc) + lane] = ti - tau[lane];
      if (nc) contact_jac_lane(b, W, lane, Jc, A, lda);
    }
    if (!imp && lane >= 64 && lane < 64 + b.ncon) {
      int row0;
      const CRec C{contact_rec(b, lane - 64, &row0)};
      contact_a0_drift(b, W, C, a0 + row0);
    }
    if (lane == 128) {  // the wide records' values from their lane partials
      const double* cr = b.C;
      int nw = 0;
      for (int k = 0; k < b.ncost; ++k) {
        const CRec C{cr};
        if (wide_cost(C, nw)) {
          double a = 0.;
          for (int l = 0; l < 64; ++l) a += pb[64 * nw + l];
          cv[k] = C.weight() * (0.5 * a);
          ++nw;
        }
        cr += C.size();
      }
    }
  });
  bool ok = mb_solve(ex, A, nj, lda, ncol, flag, pb);
  // z, then a (impulse: v+, in tau's slot; z = M^-1 M v = v)
  double* a = imp ? tau : A + (int64_t)lda * (nj + nc);
  if (nc > 0) {
    ex.run([&](int lane) {
      for (int e = lane; e < nc * (nc + 1); e += ex.nt) {
        const int col = e / nc, row = e % nc;
        const double* yc = (imp && col == nc) ? x + nq : A + (int64_t)lda * (nj + col);
        double s = 0.;
        for (int i = 0; i < nj; ++i) s += Jc[(int64_t)row * nj + i] * yc[i];
        S[e] = col < nc ? s + (row == col ? b.damping : 0.) : (imp ? (1. + b.r_coeff) * s : s + a0[row]);
      }
    });
    ok = gauss_jordan<1>(ex, S, nc, nc, nc + 1, flag, pb) && ok;
    ex.run([&](int lane) {
      const int kf = lane - 64;
      if (kf >= 0 && kf < b.ncost) {
        const double* cr = b.C;
        for (int k = 0; k < kf; ++k) cr += CRec{cr}.size();
        const CRec C{cr};
        if (force_cost(C.type())) {
          // lambda = -S's last column, read where it lies (no private copy)
          const double* Sl = S + (int64_t)nc * nc;
          cv[kf] = C.weight() * force_cost_activation_at(b, C, [Sl](int k) { return -Sl[k]; }, nu);
        }
      }
      if (lane >= nj) return;
      double s = imp ? x[nq + lane] : a[lane];
      for (int k = 0; k < nc; ++k) s -= A[(int64_t)lda * (nj + k) + lane] * S[(int64_t)nc * nc + k];
      a[lane] = s;
    });
  }
#if MB_CALC_IMPULSE_COM
  if (has_impulse_com(b)) {  // CostModelImpulseCoM: r = Jcom (v+ - v), from v+ (in a)
    ex.run([&](int lane) { impulse_com_calc_bodies(b, W, x, a, lane); });
    ex.run([&](int lane) { impulse_com_calc_value(b, W, cv, lane); });
  }
#endif
  const double dt = b.dt;
  if (!ok)
    ex.run([&](int i) {
      if (i < nj) a[i] = NAN;
    });
  ex.run([&](int i) {
    if (i == 64) {
      double total = 0.;
      for (int k = 0; k < b.ncost; ++k) total += cv[k];
      red[0] = total;
    }
    if (i >= nj) return;
    if (imp) {
      xnext[nq + i] = nc > 0 ? a[i] : x[nq + i];
      if (!ok) xnext[nq + i] = NAN;
      xnext[i] = x[i];
      if (i == nj - 1 && b.ff) xnext[nq - 1] = x[nq - 1];
      return;
    }
    if (dt != 0.) {
      euler_step(b, x, a, dt, xnext, i);
    } else {
      xnext[i] = x[i];
      xnext[nq + i] = x[nq + i];
      if (i == nj - 1 && b.ff) xnext[nq - 1] = x[nq - 1];
    }
  });
  const double cc = red[0];
  (void)nx;
  return dt != 0. ? dt * cc : cc;
}

template <int NT>
__device__ __forceinline__ double knot_calc(const double* P, int nx, const double* x, const double* u, bool use_u, double* xnext,
                                   double* w) {
  static_assert(NT >= 256, "the multibody calc splits its phases over 4 waves");
#ifdef MB_CALC_DENSE
  return knot_calc_dense_x(DevExec{NT}, P, nx, x, u, use_u, xnext, w);
#else
  return knot_calc_x(DevExec{NT}, P, nx, x, u, use_u, xnext, w);
#endif
}

// ---------------------------------------------------------------------------
// calcDiff: one kMbDiffNT-thread workgroup per (element, knot).
//
// World-frame RNEA derivatives. Perturbing q_j moves the whole subtree of dof j's
// body rigidly by S_j, so every world quantity X of that subtree changes by the
// transport S_j x X (x* for forces) plus an intrinsic part; with
//   V_P, A_P: velocity / acceleration (gravity included) of the parent body of j,
//   u_j = S_j x V_P,  c_j = -S_j x A_P + u_j x V_P,  w_j = (V_b(j) + V_P) x S_j,
// the body accelerations and velocities change by
//   dA_b/dq_j = S_j x A_b + c_j - u_j x V_b,  dV_b/dq_j = S_j x V_b - u_j,
//   dA_b/dv_j = w_j + S_j x V_b,              dV_b/dv_j = S_j,
// for every body b below j, and the transport cancels in tau_k = S_k . F_k, so
//   k below j (incl. j's body):   dtau_k/dq_j = Q_k . c_j - P_k . u_j,   dtau_k/dv_j = Q_k . w_j + P_k . S_j
//   k strict ancestor of j:       dtau_k/dx_j = S_k . G_j
// with Q_k = Ycrb_k S_k (composite inertia), P_k = sum_{b in sub(k)} [V_b x* (Y_b S_k)
// - Y_b (V_b x S_k)] - S_k x* sum_{b in sub(k)} Y_b V_b, and G_j = S_j x* F_j +
// Ycrb_j c_j - B_j u_j (q) / Ycrb_j w_j + B_j S_j (v), B_j x = sum_{b in sub(j)}
// [-Y_b (V_b x x) + x x* (Y_b V_b) + V_b x* (Y_b x)]. Contact forces are fixed in
// their frames (computeRNEADerivatives with fext) and enter through F.
// ---------------------------------------------------------------------------
struct DiffLayout {
  int64_t wv, A, dtau, da, qp, vec, J, red, total;
  // cost-derivative area (after the dynamics, over the dead world values when it
  // fits): group table, per-row Arr / Ar factors, the stacked residual Jacobians
  int64_t R;
  // contact area (nc > 0): Jc nc x nj, a0 nc, lambda nc, Y = Minv Jc^T and
  // H = Y S^-1 (nj x nc each), [S | I | r] nc x (2nc + 1), da0/dx nc x L, fx 6 nj
  int64_t Jc, a0, lam, Y, H, Sx, da0, fx, zv, dfx, dfu;
  // the per-wave partials of the recursions (kinematics / the RNEA at the solved a), the
  // per-body velocity-product maps and their subtree sums; half: doubles per half of A
  int64_t pk, pr, nb, ns, half;
  // the cost table's diagonal terms and residual rows (after the table, or apart from it),
  // and the LDS copy of dtau the da product reads (the spilled plan: over the world values)
  int64_t Rr, dts;
  // with an actuation record: Kinv_atau S (nj x nu at ld lda_of(nj)), da phase .. Fu; -1 without
  // (all-LDS plan: over the first half of A; spilled plan: an area of its own)
  int64_t KS, ksz;
  // with a squashed record: s(u) and D(u) = ds/du (nu each), first phase .. Fu; -1 without (an area of its own)
  int64_t sq, sqsz;
  int spill;       // kSpill* flags the plan was made with
  int64_t ht;      // host emulation: its factorisation scratch (70 nj)
  int64_t htotal;  // host emulation: total plus its own areas (da, the factorisation scratch)
};
// The spilled calcDiff plan (the Talos-size trees): the LDS plan keeps what the phases read
// at random, and the arrays each written once and streamed once go to the knot's own
// output blocks in global memory, dead there until the blocks are written (after their
// last read): dtau/dx into Lxx (read by the da product, the Gauss-Newton blocks write Lxx
// after it), the body maps and their subtree sums into Fx (read up to the tangent
// directions; the da product writes Fx), the jac-cost Jacobians into Lxu (kSpillJ: read by
// the residual rows, before the Gauss-Newton blocks), d lambda / dx, du into Fu (kSpillF:
// read by the residual rows; Fu is written last). The product's epilogue writes Fx
// itself, so da needs no area; Minv and the contact arrays share the factorisation's A
// area. Two workgroups share a CU under it (<= 80 KB with the parameter block).
constexpr int kSpillBlocks = 1, kSpillJ = 2, kSpillF = 4;
// vec area: x (nq + nj <= 2 nj + 1), u (nj), nle / z / a / tau (3 nj), jac-cost
// residuals (6 per cost), Jexp6 / Ad(exp6^-1) (72)
// Cost-derivative area (doubles) for nrows stacked residual rows over L + nu columns.
constexpr int kMaxCostRows = 64;
// source code of a stacked residual row (the cost table's csrc): jac cost f, row e as 8 f + e,
// plus kImpulseComSrc on the rows of an impulse CoM cost; force cost row e as -1 - e
constexpr int kImpulseComSrc = 1024;
// (4 columns of slack: the GEMM reads rows four columns at a time)
MB_HD __forceinline__ int cost_rows_ld(int nj, int nu) { return (int)pad2(2 * nj + nu) + 4; }
constexpr int kMaxCostCols = 3 * kMaxJ;  // diagonal terms per column of [x tangent | u]
MB_HD __forceinline__ int64_t cost_table_doubles() { return 4 * kMaxCosts + 5 * kMaxCostRows; }
MB_HD __forceinline__ int64_t cost_area_doubles(int nj, int nu, int nrows) {
  return cost_table_doubles() + kMaxCostCols + (int64_t)nrows * cost_rows_ld(nj, nu);
}
__host__ __device__ inline DiffLayout diff_layout(int nj, int njac, int nc = 0, bool vel_cols = false, int nu = 0,
                                                  int nrows = 0, int spill = 0, bool act = false,
                                                  bool sat = false) {
  const int L = 2 * nj;
  DiffLayout l;
  l.spill = spill;
  l.KS = -1;
  l.ksz = act ? (int64_t)lda_of(nj) * nu : 0;
  l.sq = -1;
  l.sqsz = act && sat ? 2 * (int64_t)nu : 0;
  const int64_t jsz = (int64_t)6 * (vel_cols ? L : nj) * (njac > 0 ? njac : 1);  // jac-cost Jacobians [cost][6][jw]
  const int64_t ca = cost_area_doubles(nj, nu, nrows);
  const int64_t wvs = pad2(WVals::doubles(nj));
  if (!(spill & kSpillBlocks)) {
    // dtau [k][L] (first the per-body N_b, h_b: 42 per dof); the da area (first the subtree
    // sums Nsub, Hsub; da itself on the host: the device's product writes Fx directly)
    // (da rows at the odd stride L + 1: the Fx assembly reads a column of it per wave)
    const int64_t dsz = pad2((int64_t)nj * (L + 1) > 42 * (int64_t)nj ? (int64_t)nj * (L + 1) : 42 * (int64_t)nj);
    // the world values, then dtau: both dead after the da phase, so the cost-derivative
    // area can run over both
    l.wv = 0;
    l.dtau = l.wv + wvs;
    l.half = pad2((int64_t)lda_of(nj) * nj);
    l.A = l.dtau + dsz;  // [M | Minv], ld lda_of(nj)
    l.da = l.A + 2 * l.half;
    l.pk = l.pr = l.nb = l.dtau;
    l.ns = l.da;
    l.qp = l.da + dsz;
    l.vec = l.qp + (int64_t)12 * nj;      // Q_k, P_k
    l.J = l.vec + pad2(6 * nj + 1 + 6 * kMaxJacCosts + 72);
    l.red = l.J + jsz;
    l.total = l.red + 8 + 128;  // reductions, Gauss-Jordan pivot-column buffer
    l.Jc = l.total;
    l.a0 = l.Jc + (int64_t)nc * nj;
    l.lam = l.a0 + nc;
    l.Y = l.lam + nc;
    l.H = l.Y + (int64_t)nj * nc;
    l.Sx = l.H + (int64_t)nj * nc;
    l.da0 = l.Sx + (int64_t)nc * (2 * nc + 1);
    l.fx = l.da0 + (int64_t)nc * L;
    l.zv = l.fx + 6 * nj;  // impulse: v+ - v
    l.dfx = l.zv + nj;     // d lambda / dx (nc x L), d lambda / du (nc x nj): CostModelContactForce
    l.dfu = l.dfx + (int64_t)nc * L;
    l.total = nc > 0 ? l.dfu + (int64_t)nc * nj : l.total;
    // the table (written on spare lanes during the da phase, beside the dtau reads) within
    // the world values; the diagonal terms and R rows (written after it) also over dtau
    if (cost_table_doubles() <= wvs && ca <= wvs + dsz) {
      l.R = l.wv;
    } else {
      l.R = pad2(l.total);
      l.total = l.R + ca;
    }
    l.Rr = l.R + cost_table_doubles();
    l.dts = l.dtau;
    if (act) l.KS = l.A;  // over M and its factors, dead since M^-1 (nu <= nj columns at the same ld)
    if (l.sqsz) {
      l.sq = pad2(l.total);
      l.total = l.sq + l.sqsz;
    }
    l.ht = pad2(l.total);  // host: the factorisation scratch
    l.htotal = l.ht + pad2((int64_t)70 * nj);
    return l;
  }
  // spilled plan; live ranges (phases of knot_calc_diff_x):
  //   world values        kinematics .. tangent directions; then the cost area
  //   A, first half       M and its factors .. M^-1; then Y (z / Y .. Kinv), the partials
  //                       of the RNEA at the solved a, then da0 / dlambda/dx, du (tangent
  //                       directions .. residual rows) when they fit, else their own area
  //   A, second half      the recursions' partials (kinematics), the factorisation's
  //                       scratch, then M^-1 / Kinv top-left .. Fu
  //   contact area        Jc, a0, lambda, H, [S | I | r], joint forces, v+ - v
  l.half = pad2(lda_of(nj) * (int64_t)nj > part_doubles(nj) ? lda_of(nj) * (int64_t)nj : part_doubles(nj));
  l.wv = 0;
  l.A = wvs;
  l.pk = l.A + l.half;
  l.pr = l.A;
  l.dtau = l.nb = l.ns = -1;  // in the output blocks
  l.qp = l.A + 2 * l.half;
  l.vec = l.qp + (int64_t)12 * nj;
  l.red = l.vec + pad2(6 * nj + 1 + 6 * kMaxJacCosts + 72);
  l.total = l.red + 8 + 128;
  l.J = -1;
  if (!(spill & kSpillJ)) {
    l.J = l.total;
    l.total = pad2(l.J + jsz);
  }
  l.Jc = l.total;
  l.a0 = l.Jc + (int64_t)nc * nj;
  l.lam = l.a0 + nc;
  l.H = l.lam + nc;
  l.Sx = l.H + (int64_t)nj * nc;
  l.fx = l.Sx + (int64_t)nc * (2 * nc + 1);
  l.zv = l.fx + 6 * nj;
  if (nc > 0) l.total = pad2(l.zv + nj);
  const int64_t ysz = (int64_t)nj * nc, d0 = pad2((int64_t)nc * L), dfs = pad2((int64_t)nc * L) + (int64_t)nc * nj;
  l.Y = ysz <= l.half ? l.A : l.total;
  if (nc > 0 && l.Y == l.total) l.total = pad2(l.total + ysz);
  l.da0 = d0 <= l.half ? l.A : l.total;
  if (nc > 0 && l.da0 == l.total) l.total = pad2(l.total + d0);
  // d lambda / dx, du: the knot's Fu block (kSpillF: written after the residual rows read
  // them), else after da0 when both fit the half, else their own area
  if (spill & kSpillF) {
    l.dfx = l.dfu = -1;
  } else {
    l.dfx = (l.da0 == l.A && d0 + dfs <= l.half) ? l.A + d0 : l.total;
    if (nc > 0 && l.dfx == l.total) l.total = pad2(l.total + dfs);
    l.dfu = l.dfx + pad2((int64_t)nc * L);
  }
  // The cost area: where the world values are dead (from the da phase on). With room in
  // the first half of A after da0 (and d lambda / dx, du not there) the table (written
  // during the da phase) goes there, and the da phase reads dtau from an LDS copy over the
  // world values (dts: its loads then never wait behind the Fx stores, as global loads
  // do); the diagonal terms and the rows (from the next phase on) over the world values.
  // Else the whole area over the world values and the first half, when it fits.
  const bool f_in_half = nc > 0 && l.dfx >= l.A && l.dfx < l.A + l.half;
  const int64_t tab0 = (nc > 0 ? d0 : 0), rsz = ca - cost_table_doubles();
  l.dts = -1;
  if (!f_in_half && tab0 + cost_table_doubles() <= l.half && (int64_t)nj * L <= wvs && rsz <= wvs) {
    l.R = l.A + tab0;
    l.Rr = l.wv;
    l.dts = l.wv;
  } else if (cost_table_doubles() + kMaxCostCols <= wvs && ca <= wvs + (f_in_half ? 0 : l.half)) {
    l.R = l.wv;
    l.Rr = l.R + cost_table_doubles();
  } else {
    l.R = pad2(l.total);
    l.total = l.R + ca;
    l.Rr = l.R + cost_table_doubles();
  }
  // (the spilled plan reuses the first half of A to the end: an area of its own. No device object
  // runs this pair today, the launch plan keeps horizons with a record on the all-LDS plan; the
  // host emulation does)
  if (act) {
    l.KS = pad2(l.total);
    l.total = l.KS + l.ksz;
  }
  if (l.sqsz) {
    l.sq = pad2(l.total);
    l.total = l.sq + l.sqsz;
  }
  // host emulation: the da area and the factorisation's scratch of its own
  l.da = pad2(l.total);
  l.ht = l.da + pad2((int64_t)nj * (L + 1));
  l.htotal = l.ht + pad2((int64_t)70 * nj);
  return l;
}
// The spill flags of a handle's plan: spill when the all-LDS plan (with the parameter block
// of psz doubles) exceeds half the CU's LDS, the tree is large enough for the body maps
// and their sums (84 nj doubles) to fit in the Fx block (4 nj^2); the Jacobians go to
// Lxu (2 nj m), d lambda / dx, du to Fu (2 nj m) when they fit.
MB_HD inline int diff_spill(int nj, int njac, int nc, bool vcols, int nu, int nrows, int64_t psz, int m,
                            bool act = false, bool sat = false) {
  const DiffLayout a = diff_layout(nj, njac, nc, vcols, nu, nrows, 0, act, sat);
  if ((pad2(a.total) + pad2(psz)) * 8 <= 80 * 1024 || 84 * (int64_t)nj > 4 * (int64_t)nj * nj) return 0;
  const int64_t jsz = (int64_t)6 * (vcols ? 2 * nj : nj) * (njac > 0 ? njac : 1);
  const int64_t fsz = pad2((int64_t)nc * 2 * nj) + (int64_t)nc * nj;
  return kSpillBlocks | (jsz <= (int64_t)2 * nj * m ? kSpillJ : 0) | (nc > 0 && fsz <= (int64_t)2 * nj * m ? kSpillF : 0);
}

// Live ranges of the calcDiff's LDS arrays (knot_calc_diff_x's phases, in order), for the
// static check of its plans (diff_layout_check): arrays whose areas overlap must not be
// live in a common phase.
enum DiffPhase {
  DP_INIT, DP_KIN, DP_CONTACT, DP_FACTOR, DP_MINV, DP_ZY, DP_SX, DP_SGJ, DP_LAMH, DP_KINV, DP_RNEA2, DP_CALC,
  DP_QPJAC, DP_TANG, DP_DA, DP_RROWS, DP_GN, DP_END
};
struct DiffRegion {
  const char* name;
  int64_t off, size;
  int first, last;
};
// The regions of plan l (host emulation areas excluded); returns their count (<= 40).
MB_HD inline int diff_layout_regions(const DiffLayout& l, int nj, int njac, int nc, bool vcols, int nu, int nrows,
                                     DiffRegion* r) {
  const int L = 2 * nj;
  const bool sp = l.spill & kSpillBlocks;
  const int64_t wvs = WVals::doubles(nj), jsz = (int64_t)6 * (vcols ? L : nj) * (njac > 0 ? njac : 1);
  int k = 0;
  auto add = [&](const char* n, int64_t off, int64_t size, int first, int last) {
    if (off >= 0 && size > 0) r[k++] = DiffRegion{n, off, size, first, last};
  };
  add("world values", l.wv, wvs, DP_INIT, DP_TANG);
  add("M / its factors", l.A, (int64_t)lda_of(nj) * nj, DP_KIN, DP_MINV);
  // (the fast path's rows, or the generic steps' masks; then the recursions' partials are
  // dead, and M^-1 is written)
  // ((depth + 1) nj <= min(kTreeKD, nj) nj doubles, or 2 nj)
  const int64_t fs = (int64_t)nj * (kTreeKD < nj ? kTreeKD : nj);
  add("factorisation scratch", l.A + l.half, fs > 2 * nj ? fs : 2 * nj, DP_FACTOR, DP_FACTOR);
  add("Minv / Kinv", l.A + l.half, (int64_t)lda_of(nj) * nj, DP_MINV, DP_END);
  add("partials (kinematics)", l.pk, part_doubles(nj), DP_KIN, DP_KIN);
  add("partials (RNEA at a)", l.pr, part_doubles(nj), DP_RNEA2, DP_RNEA2);
  add("qp", l.qp, (int64_t)12 * nj, DP_FACTOR, DP_TANG);
  add("vec", l.vec, 6 * nj + 1 + 6 * kMaxJacCosts + 72, DP_INIT, DP_END);
  add("red / pivots", l.red, 8 + 128, DP_INIT, DP_END);
  if (!(l.spill & kSpillJ)) add("jac-cost Jacobians", l.J, jsz, DP_FACTOR, DP_RROWS);
  if (!sp) {
    // (built beside the factorisation, or after the RNEA at a when no wave is idle then)
    add("body maps (side)", l.nb, (int64_t)42 * nj, DP_FACTOR, DP_FACTOR);
    add("body maps", l.nb, (int64_t)42 * nj, DP_QPJAC, DP_QPJAC);
    add("subtree sums", l.ns, (int64_t)42 * nj, DP_FACTOR, DP_TANG);
    add("dtau", l.dtau, (int64_t)nj * L, DP_TANG, DP_DA);
  }
  if (nc > 0) {
    add("Jc", l.Jc, (int64_t)nc * nj, DP_CONTACT, DP_DA);
    add("a0", l.a0, nc, DP_CONTACT, DP_SX);
    add("lambda", l.lam, nc, DP_LAMH, DP_END);
    add("Y", l.Y, (int64_t)nj * nc, DP_ZY, DP_KINV);
    add("H", l.H, (int64_t)nj * nc, DP_LAMH, DP_DA);
    add("[S | I | r]", l.Sx, (int64_t)nc * (2 * nc + 1), DP_SX, DP_DA);
    add("da0", l.da0, (int64_t)nc * L, DP_TANG, DP_DA);
    add("contact joint forces", l.fx, 6 * nj, DP_KINV, DP_RNEA2);
    add("v+ - v", l.zv, nj, DP_KINV, DP_RNEA2);
    if (!(l.spill & kSpillF)) {
      add("d lambda / dx", l.dfx, (int64_t)nc * L, DP_DA, DP_RROWS);
      add("d lambda / du", l.dfu, (int64_t)nc * nj, DP_DA, DP_RROWS);
    }
  }
  add("cost table", l.R, cost_table_doubles(), DP_DA, DP_END);
  add("cost diagonal / rows", l.Rr, cost_area_doubles(nj, nu, nrows) - cost_table_doubles(), DP_RROWS, DP_END);
  if (sp && l.dts >= 0) add("dtau (LDS copy)", l.dts, (int64_t)nj * L, DP_DA, DP_DA);
  add("Kinv S (actuation record)", l.KS, l.ksz, DP_DA, DP_END);
  add("s(u), ds/du (squashed record)", l.sq, l.sqsz, DP_INIT, DP_END);
  return k;
}
// 0 when no two regions of the plan overlap in both LDS and live range (and all lie in
// [0, total)); else the index + 1 of the first region in conflict (a, b: the pair).
MB_HD inline int diff_layout_check(const DiffLayout& l, int nj, int njac, int nc, bool vcols, int nu, int nrows,
                                   int* a = nullptr, int* b = nullptr) {
  DiffRegion r[40];
  const int n = diff_layout_regions(l, nj, njac, nc, vcols, nu, nrows, r);
  for (int i = 0; i < n; ++i) {
    if (r[i].off + r[i].size > l.total) {
      if (a) *a = i, *b = i;
      return i + 1;
    }
    for (int j = i + 1; j < n; ++j) {
      const bool mem = r[i].off < r[j].off + r[j].size && r[j].off < r[i].off + r[i].size;
      const bool live = r[i].first <= r[j].last && r[j].first <= r[i].last;
      if (mem && live) {
        if (a) *a = i, *b = j;
        return i + 1;
      }
    }
  }
  return 0;
}

// The velocity-product terms of the derivatives are linear maps of the subtree
// bodies: with N_b x = V_b x* (Y_b x) - Y_b (V_b x x) and h_b = Y_b V_b,
//   P_k = Nsub_k S_k - S_k x* Hsub_k,   B_j x = Nsub_j x + x x* Hsub_j,
// Nsub / Hsub the subtree sums. lane d < nj: N_d (column-major 6x6) and h_d of d's
// body (zero on the massless free-flyer dofs) into nb[42 d ..].
MB_HD inline void body_nh_lane(const Blk& b, const WVals& W, int d, double* nb) {
  double* o = nb + 42 * d;
  if (!carries_body(b, d)) {
    for (int e = 0; e < 42; ++e) o[e] = 0.;
    return;
  }
  const double m = *W.m(d);
  double c[3], I6[6], V[6];
  for (int e = 0; e < 3; ++e) c[e] = W.c(d)[e];
  for (int e = 0; e < 6; ++e) {
    I6[e] = W.Ic(d)[e];
    V[e] = W.v(d)[e];
  }
  for (int col = 0; col < 6; ++col) {
    double x[6] = {0., 0., 0., 0., 0., 0.}, Yx[6], t1[6], VxX[6], t2[6];
    x[col] = 1.;
    inertia_mul(m, c, I6, x, Yx);
    cross_f(V, Yx, t1);
    cross_m(V, x, VxX);
    inertia_mul(m, c, I6, VxX, t2);
    for (int e = 0; e < 6; ++e) o[6 * col + e] = t1[e] - t2[e];
  }
  inertia_mul(m, c, I6, V, o + 36);
}
// lane j < nj of wave w (of nw): components [11 w, 11 w + 11) of Nsub_j, Hsub_j (sums over
// the bodies below dof j) into ns[42 j ..]; every body read, the others weighted 0 (no
// branch: the unrolled loads overlap), the 42 components split over the waves
template <int kC = 11>  // components per pass (11 for 4 waves, 6 for 8: one pass per wave)
MB_HD inline void subtree_nh_lane(const Blk& b, const WVals& W, int j, const double* nb, double* ns, int w = 0,
                                  int nw = 1) {
  // wave w's components [w per, (w + 1) per), per = ceil(42 / nw), in chunks of kC
  const int per = (42 + nw - 1) / nw, e0 = w * per, e1 = e0 + per < 42 ? e0 + per : 42;
  double acc[kC];
  for (int e = 0; e < kC; ++e) acc[e] = 0.;
  for (int c0 = e0; c0 < e1; c0 += kC) {
#pragma unroll 2
    for (int bb = 0; bb < b.nj; ++bb) {
      const bool in = ((*W.anc(bb) >> j) & 1ull) && carries_body(b, bb);
      const double* o = nb + 42 * bb + c0;
#pragma unroll
      for (int e = 0; e < kC; ++e) {
        const double v = c0 + e < e1 ? o[e] : 0.;
        acc[e] += in ? v : 0.;
      }
    }
#pragma unroll
    for (int e = 0; e < kC; ++e) {
      if (c0 + e < e1) ns[42 * j + c0 + e] = acc[e];
      acc[e] = 0.;
    }
  }
}
// B_j x = Nsub_j x + x x* Hsub_j
MB_HD __forceinline__ void bsub_mul_ns(const double* ns, int j, const double* x, double* o) {
  const double* N = ns + 42 * j;
  double t[6];
  cross_f(x, N + 36, t);
  for (int e = 0; e < 6; ++e) {
    double v = t[e];
    for (int col = 0; col < 6; ++col) v += N[6 * col + e] * x[col];
    o[e] = v;
  }
}
// lane k < nj: Q_k = Ycrb_k S_k, P_k = Nsub_k S_k - S_k x* Hsub_k. qp[12 k ..].
MB_HD inline void qp_lane_ns(const WVals& W, int k, const double* ns, double* qp) {
  double S[6], Q[6], t6[6];
  for (int e = 0; e < 6; ++e) S[e] = W.S(k)[e];
  comp_mul(W, k, S, Q);
  const double* N = ns + 42 * k;
  cross_f(S, N + 36, t6);
  for (int e = 0; e < 6; ++e) {
    double v = -t6[e];
    for (int col = 0; col < 6; ++col) v += N[6 * col + e] * S[col];
    qp[12 * k + e] = Q[e];
    qp[12 * k + 6 + e] = v;
  }
}

// lane k < nj: Q_k = Ycrb_k S_k, P_k (header comment). qp[12 k ..].
MB_HD inline void qp_lane(const Blk& b, const WVals& W, int k, double* qp) {
  double S[6], Q[6], P[6] = {0., 0., 0., 0., 0., 0.}, Hc[6] = {0., 0., 0., 0., 0., 0.};
  for (int e = 0; e < 6; ++e) S[e] = W.S(k)[e];
  comp_mul(W, k, S, Q);
  for (int bb = 0; bb < b.nj; ++bb) {
    if (!((*W.anc(bb) >> k) & 1ull) || !carries_body(b, bb)) continue;
    const double m = *W.m(bb);
    double c[3], I6[6], V[6], YS[6], VxS[6], YVxS[6], t6[6], h[6];
    for (int e = 0; e < 3; ++e) c[e] = W.c(bb)[e];
    for (int e = 0; e < 6; ++e) {
      I6[e] = W.Ic(bb)[e];
      V[e] = W.v(bb)[e];
    }
    inertia_mul(m, c, I6, S, YS);
    cross_m(V, S, VxS);
    inertia_mul(m, c, I6, VxS, YVxS);
    cross_f(V, YS, t6);
    inertia_mul(m, c, I6, V, h);
    for (int e = 0; e < 6; ++e) {
      P[e] += t6[e] - YVxS[e];
      Hc[e] += h[e];
    }
  }
  double t6[6];
  cross_f(S, Hc, t6);
  for (int e = 0; e < 6; ++e) {
    qp[12 * k + e] = Q[e];
    qp[12 * k + 6 + e] = P[e] - t6[e];
  }
}

// B_j x = sum_{b in sub(j)} [-Y_b (V_b x x) + x x* (Y_b V_b) + V_b x* (Y_b x)]
MB_HD inline void bsub_mul(const Blk& b, const WVals& W, int j, const double* x, double* o) {
  for (int e = 0; e < 6; ++e) o[e] = 0.;
  for (int bb = 0; bb < b.nj; ++bb) {
    if (!((*W.anc(bb) >> j) & 1ull) || !carries_body(b, bb)) continue;
    const double m = *W.m(bb);
    double c[3], I6[6], V[6], t[6], Yt[6], h[6], s1[6], Yx[6], s2[6];
    for (int e = 0; e < 3; ++e) c[e] = W.c(bb)[e];
    for (int e = 0; e < 6; ++e) {
      I6[e] = W.Ic(bb)[e];
      V[e] = W.v(bb)[e];
    }
    cross_m(V, x, t);
    inertia_mul(m, c, I6, t, Yt);
    inertia_mul(m, c, I6, V, h);
    cross_f(x, h, s1);
    inertia_mul(m, c, I6, x, Yx);
    cross_f(V, Yx, s2);
    for (int e = 0; e < 6; ++e) o[e] += s1[e] + s2[e] - Yt[e];
  }
}

// Direction dd (q_j for dd < nj, v_j otherwise): column dd of dtau/dx
// (dtau[k * L + dd]), and the motion derivatives of the contact / impulse frames.
// Parent-body quantities: V_P, A_P (gravity included; the root: 0, root_a).
MB_HD inline void parent_motion(const Blk& b, const WVals& W, int j, double* VP, double* AP) {
  const int p = body_parent(b, j);
  for (int e = 0; e < 6; ++e) {
    VP[e] = p >= 0 ? W.v(p)[e] : 0.;
    AP[e] = p >= 0 ? W.a(p)[e] : W.root_a()[e];
  }
}

// part / np: this lane's share of the rows k (the direction's setup is repeated per part)
MB_HD inline void dtau_direction(const Blk& b, const WVals& W, const double* qp, int dd, int L, double* dtau,
                                  const double* ns = nullptr, int part = 0, int np = 1) {
  const int nj = b.nj, j = dd < nj ? dd : dd - nj;
  const bool isq = dd < nj;
  double S[6], VP[6], AP[6], u[6], cj[6], G[6], t6[6], t7[6];
  for (int e = 0; e < 6; ++e) S[e] = W.S(j)[e];
  parent_motion(b, W, j, VP, AP);
  if (isq) {
    cross_m(S, VP, u);
    cross_m(S, AP, t6);
    cross_m(u, VP, t7);
    for (int e = 0; e < 6; ++e) cj[e] = t7[e] - t6[e];
    // G_j = S_j x* F_j + Ycrb_j c_j - B_j u_j
    double F[6], Bu[6];
    for (int e = 0; e < 6; ++e) F[e] = W.F(j)[e];
    cross_f(S, F, G);
    comp_mul(W, j, cj, t6);
    if (ns)
      bsub_mul_ns(ns, j, u, Bu);
    else
      bsub_mul(b, W, j, u, Bu);
    for (int e = 0; e < 6; ++e) G[e] += t6[e] - Bu[e];
  } else {
    // w_j = (V_b(j) + V_P) x S_j ; G_j = Ycrb_j w_j + B_j S_j
    double Vs[6], BS[6];
    for (int e = 0; e < 6; ++e) Vs[e] = W.v(j)[e] + VP[e];
    cross_m(Vs, S, cj);  // (w_j in cj)
    comp_mul(W, j, cj, G);
    if (ns)
      bsub_mul_ns(ns, j, S, BS);
    else
      bsub_mul(b, W, j, S, BS);
    for (int e = 0; e < 6; ++e) G[e] += BS[e];
    for (int e = 0; e < 6; ++e) u[e] = S[e];  // P_k . S_j
  }
  const Mask aj = *W.anc(j);
  int k0 = 0, k1 = nj;
  if (np > 1) k_range(nj, part, np, k0, k1);
  for (int k = k0; k < k1; ++k) {
    double val = 0.;
    if ((*W.anc(k) >> j) & 1ull) {  // k's body below j's (or the same body)
      const double* Q = qp + 12 * k;
      const double* P = Q + 6;
      val = isq ? dot6(Q, cj) - dot6(P, u) : dot6(Q, cj) + dot6(P, u);
    } else if ((aj >> k) & 1ull) {  // k's body a strict ancestor of j's
      val = dot6(W.S(k), G);
    }
    dtau[(int64_t)k * L + dd] = val;
  }
}

// Direction dd: da0/dx column (contact-3d.hxx:46-71, contact-6d.hxx:48-66) at the
// solved acceleration (getJointAccelerationDerivatives after computeRNEADerivatives):
// the frame motion derivative moved to the frame, the classical term of a 3D
// contact, the Baumgarte terms. da0[row * L + dd].
MB_HD inline void contact_direction(const Blk& b, const WVals& W, int dd, int L, double* da0) {
  const int nj = b.nj, j = dd < nj ? dd : dd - nj;
  const bool isq = dd < nj;
  double S[6], VP[6], AP[6], u[6], c0[6], t6[6], t7[6];
  for (int e = 0; e < 6; ++e) S[e] = W.S(j)[e];
  parent_motion(b, W, j, VP, AP);
  for (int e = 0; e < 6; ++e) AP[e] -= W.root_a()[e];  // gravity-free (data.a)
  if (isq) {
    cross_m(S, VP, u);
    cross_m(S, AP, t6);
    cross_m(u, VP, t7);
    for (int e = 0; e < 6; ++e) c0[e] = t7[e] - t6[e];
  } else {
    double Vs[6];
    for (int e = 0; e < 6; ++e) Vs[e] = W.v(j)[e] + VP[e];
    cross_m(Vs, S, c0);  // w_j
  }
  const double* r = b.K;
  int row = 0;
  for (int k = 0; k < b.ncon; ++k) {
    const CRec C{r};
    const double* d = C.d();
    const int fb = frame_dof(b, d);
    const int n = C.type() == C_CONTACT_3D ? 3 : 6;
    if (!((*W.anc(fb) >> j) & 1ull)) {
      for (int e = 0; e < n; ++e) da0[(int64_t)(row + e) * L + dd] = 0.;
      row += n;
      r += C.size();
      continue;
    }
    double Rf[9], pf[3], V[6], dV[6], dA[6], vf[6], dvf[6], daf[6];
    frame_placement(b, W, d, Rf, pf);
    for (int e = 0; e < 6; ++e) V[e] = W.v(fb)[e];
    if (isq) {  // dV = -u_j, dA = c0_j - u_j x V_b (intrinsic parts)
      cross_m(u, V, t6);
      for (int e = 0; e < 6; ++e) {
        dV[e] = -u[e];
        dA[e] = c0[e] - t6[e];
      }
    } else {  // dV = S_j, dA = w_j + S_j x V_b
      cross_m(S, V, t6);
      for (int e = 0; e < 6; ++e) {
        dV[e] = S[e];
        dA[e] = c0[e] + t6[e];
      }
    }
    motion_act_inv(Rf, pf, V, vf);
    motion_act_inv(Rf, pf, dV, dvf);
    motion_act_inv(Rf, pf, dA, daf);
    const double kp = C.r[1], kd = C.r[2];
    if (C.type() == C_CONTACT_3D) {
      double t1[3], t2[3], pv[3] = {0., 0., 0.};
      cross3(dvf + 3, vf, t1);
      cross3(vf + 3, dvf, t2);
      if (isq && kp != 0.) {  // world velocity of the frame origin: oRf Jc
        cross3(S + 3, pf, pv);
        for (int e = 0; e < 3; ++e) pv[e] += S[e];
      }
      for (int e = 0; e < 3; ++e)
        da0[(int64_t)(row + e) * L + dd] = daf[e] + t1[e] + t2[e] + kd * dvf[e] + kp * pv[e];
    } else {
      double rr[6], Jk[6] = {0., 0., 0., 0., 0., 0.};
      if (isq && kp != 0.) frame_residual(b, W, C, S, rr, Jk);
      for (int e = 0; e < 6; ++e) da0[(int64_t)(row + e) * L + dd] = daf[e] + kd * dvf[e] + kp * Jk[e];
    }
    row += n;
    r += C.size();
  }
}

// d(Jc v+)/dq_j for the impulse records (impulse-3d.hxx:33-39 / impulse-6d.hxx:30-36:
// getJointVelocityDerivatives at v+, moved into the frame): -Ad(oMf)^-1 (S_j x V+_P)
// with W.v holding the velocities at v+. dv0[row * L + j].
MB_HD inline void impulse_direction(const Blk& b, const WVals& W, int j, int L, double* dv0) {
  double S[6], VP[6], AP[6], u[6];
  for (int e = 0; e < 6; ++e) S[e] = W.S(j)[e];
  parent_motion(b, W, j, VP, AP);
  cross_m(S, VP, u);
  for (int e = 0; e < 6; ++e) u[e] = -u[e];
  const double* r = b.K;
  int row = 0;
  for (int k = 0; k < b.ncon; ++k) {
    const CRec C{r};
    const int fb = frame_dof(b, C.d());
    const int n = C.type() == C_CONTACT_3D ? 3 : 6;
    double o[6] = {0., 0., 0., 0., 0., 0.};
    if ((*W.anc(fb) >> j) & 1ull) {
      double Rf[9], pf[3];
      frame_placement(b, W, C.d(), Rf, pf);
      motion_act_inv(Rf, pf, u, o);
    }
    for (int e = 0; e < n; ++e) dv0[(int64_t)(row + e) * L + j] = o[e];
    row += n;
    r += C.size();
  }
}

// Column j of the centroidal momentum's two Jacobian halves (CostModelCentroidalMomentum):
// Jq = dhg/dq_j, Jv = column j of Ag. About the world origin, with h_sub(j) the momentum of
// the bodies below dof j, Y_j their composite inertia and V_P the parent body's velocity
// (turning q_j moves the subtree rigidly by S_j and changes its velocities by V_P x S_j; the
// free-flyer's dofs have V_P = 0, as for the frame-velocity cost):
//   dh_O/dv_j = Y_j S_j,   dh_O/dq_j = S_j x* h_sub(j) + Y_j (V_P x S_j).
// Moved to the CoM c, l the linear momentum: k = k_O - c x l, so
//   dk/dq_j = dk_O/dq_j - Jcom_j x l - c x dl/dq_j,   dk/dv_j = dk_O/dv_j - c x dl/dv_j.
// One pass over the bodies gives h_sub(j), the total momentum, the mass and the CoM; the
// columns are stored as they are formed (Jq[e * ld], Jv[e * ld]), the velocity column first,
// so that few values are live at once. href != null (lane 0): the residual into r as well.
MB_HD inline void momentum_columns(const Blk& b, const WVals& W, int j, double* Jq, double* Jv, int64_t ld,
                                   const double* href, double* r) {
  double hs[6] = {0., 0., 0., 0., 0., 0.}, ht[6] = {0., 0., 0., 0., 0., 0.}, c[3] = {0., 0., 0.}, mt = 0.;
  for (int k = 0; k < b.nj; ++k) {
    if (!carries_body(b, k)) continue;
    const double mk = *W.m(k);
    const double sel = ((*W.anc(k) >> j) & 1ull) ? 1. : 0.;
    double ck[3], I6[6], V[6], f[6];
    for (int e = 0; e < 3; ++e) ck[e] = W.c(k)[e];
    for (int e = 0; e < 6; ++e) {
      I6[e] = W.Ic(k)[e];
      V[e] = W.v(k)[e];
    }
    inertia_mul(mk, ck, I6, V, f);
    mt += mk;
    for (int e = 0; e < 3; ++e) c[e] += mk * ck[e];
    for (int e = 0; e < 6; ++e) {
      ht[e] += f[e];
      hs[e] += sel * f[e];
    }
  }
  for (int e = 0; e < 3; ++e) c[e] /= mt;
  if (href) {  // hg = [l; k_O - c x l]
    double t[3];
    cross3(c, ht, t);
    for (int e = 0; e < 3; ++e) {
      r[e] = ht[e] - href[e];
      r[3 + e] = ht[3 + e] - t[e] - href[3 + e];
    }
  }
  double S[6], d6[6], t3[3];
  for (int e = 0; e < 6; ++e) S[e] = W.S(j)[e];
  comp_mul(W, j, S, d6);  // dh_O/dv_j
  cross3(c, d6, t3);
  for (int e = 0; e < 3; ++e) {
    Jv[e * ld] = d6[e];
    Jv[(3 + e) * ld] = d6[3 + e] - t3[e];
  }
  double VP[6], AP[6], u6[6], t6[6];
  parent_motion(b, W, j, VP, AP);
  cross_m(VP, S, u6);
  comp_mul(W, j, u6, d6);
  cross_f(S, hs, t6);
  for (int e = 0; e < 6; ++e) d6[e] += t6[e];  // dh_O/dq_j
  double jc[3], a1[3];
  cross3(S + 3, W.ch(j), t3);  // Jcom col j = (m_sub S_lin + S_ang x h_sub) / m_total
  const double m = *W.cm(j);
  for (int e = 0; e < 3; ++e) jc[e] = (m * S[e] + t3[e]) / mt;
  cross3(jc, ht, a1);
  cross3(c, d6, t3);
  for (int e = 0; e < 3; ++e) {
    Jq[e * ld] = d6[e];
    Jq[(3 + e) * ld] = d6[3 + e] - a1[e] - t3[e];
  }
}

// lane j < nj: column j of every jac-cost Jacobian (Jf[(f*6 + e)*jw + j]; a frame-velocity
// or centroidal-momentum cost also its velocity column nj + j) and, on lane 0, their
// residuals (rf[6 f + e]); lanes j < 6 of a free-flyer knot also the Euler step's
// Jexp6(dq) column j (Je, col-major 6x6) and, on lane 0, Ad(exp6(dq)^-1) (Ai).
// only: -1 every jac cost, -2 none (the free-flyer Euler terms alone), f >= 0 jac cost f
// alone (one (dof, cost) item per lane)
MB_HD inline void jac_lane(const Blk& b, const WVals& W, const double* x, int j, double* Jf, int jw, double* rf,
                           const double* dqff, double* Je, double* Ai, int only = -1) {
  const int nj = b.nj;
  double S[6];
  for (int e = 0; e < 6; ++e) S[e] = W.S(j)[e];
  const double* cr = b.C;
  int f = 0;
  for (int k = 0; k < b.ncost && only != -2; ++k) {
    const CRec C{cr};
    const int t = C.type();
    // (the impulse CoM cost's slot: impulse_com_lane, after the RNEA at v+ - v)
    if (jac_cost(b, t) && (t == C_IMPULSE_COM || (only >= 0 && f != only))) {
      ++f;
    } else if (jac_cost(b, t)) {
      double r[6] = {0., 0., 0., 0., 0., 0.}, Jc[6] = {0., 0., 0., 0., 0., 0.};
      if (t == C_FRAME_PLACEMENT || t == C_FRAME_TRANSLATION || t == C_FRAME_ROTATION) {
        const bool sup = (*W.anc(frame_dof(b, C.d())) >> j) & 1ull;
        frame_residual(b, W, C, sup ? S : nullptr, r, Jc);
      } else if (t == C_FRAME_VELOCITY) {  // getFrameVelocityDerivatives (LOCAL)
        // dv_f/dq_j = -Ad(oMf)^-1 (S_j x V_P) (the transport of the subtree cancels),
        // dv_f/dv_j = Ad(oMf)^-1 S_j, for the dofs that move the frame's body
        const double* d = C.d();
        double Jv[6] = {0., 0., 0., 0., 0., 0.};
        if ((*W.anc(frame_dof(b, d)) >> j) & 1ull) {
          double Rf[9], pf[3], VP[6], AP[6], u6[6];
          frame_placement(b, W, d, Rf, pf);
          parent_motion(b, W, j, VP, AP);
          cross_m(S, VP, u6);
          for (int e = 0; e < 6; ++e) u6[e] = -u6[e];
          motion_act_inv(Rf, pf, u6, Jc);
          motion_act_inv(Rf, pf, S, Jv);
        }
        for (int e = 0; e < 6; ++e) Jf[((int64_t)f * 6 + e) * jw + nj + j] = Jv[e];
        if (j == 0) frame_velocity_res(b, W, d, r);
      } else if (t == C_CENTROIDAL_MOMENTUM) {  // [dhg/dq_j, Ag_j]
        // (the q column stored here, and once more by the common store below)
        double* Jq = Jf + (int64_t)f * 6 * jw + j;
        momentum_columns(b, W, j, Jq, Jq + nj, jw, j == 0 ? C.d() : nullptr, r);
        for (int e = 0; e < 6; ++e) Jc[e] = Jq[(int64_t)e * jw];
      } else if (t == C_COM_POSITION) {  // Jcom col j = (m_sub S_lin + S_ang x h_sub) / m_total
        double mt = 0.;
        for (int bb = 0; bb < nj; ++bb)
          if (carries_body(b, bb)) mt += *W.m(bb);
        double tt[3];
        cross3(S + 3, W.ch(j), tt);
        const double m = *W.cm(j);
        for (int e = 0; e < 3; ++e) Jc[e] = (m * S[e] + tt[e]) / mt;
        if (j == 0) {
          double c[3];
          com_value(b, W, c);
          for (int e = 0; e < 3; ++e) r[e] = c[e] - C.d()[e];
        }
      } else {  // free-flyer block of a state cost: Jlog6(Mref^-1 M) (Jdiff second, multibody.hxx:118-126)
        double Rr[9], pr[3];
        ff_rel(C.d(), x, Rr, pr);
        if (j < 6) jlog6_col(Rr, pr, j, Jc);
        if (j == 0) log6_t<double>(Rr, pr, r);
      }
      const int nr = jac_rows(t);
#pragma unroll
      for (int e = 0; e < 6; ++e)
        if (e < nr) {
          Jf[((int64_t)f * 6 + e) * jw + j] = Jc[e];
          if (j == 0) rf[6 * f + e] = r[e];
        }
      ++f;
    }
    cr += C.size();
  }
  if (dqff && j < 6) {
    jexp6_col(dqff, j, Je + 6 * j);
    if (j == 0) {  // Ad(M^-1) of M = exp6(dq): [[R^T, -R^T [p]x], [0, R^T]]
      double R[9], p[3];
      exp6_t<double>(dqff, R, p);
      for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 6; ++r) Ai[c * 6 + r] = 0.;
      for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
          const double Rt = R[r * 3 + c];  // (R^T)(r, c)
          Ai[c * 6 + r] = Rt;
          Ai[(c + 3) * 6 + r + 3] = Rt;
        }
      for (int c = 0; c < 3; ++c) {  // -R^T [p]x, column c: -R^T (p x e_c)
        const double e[3] = {c == 0 ? 1. : 0., c == 1 ? 1. : 0., c == 2 ? 1. : 0.};
        double t[3], o[3];
        cross3(p, e, t);
        matTvec3(R, t, o);
        for (int r = 0; r < 3; ++r) Ai[(c + 3) * 6 + r] = -o[r];
      }
    }
  }
}

// lane j < nj of an impulse knot: column j of every impulse CoM cost's slot (jac cost f):
// rows 0..2 d(Jcom(q) w)/dq_j at w = v+ - v held fixed, rows 3..5 Jcom's column j; on lane 0
// the residual Jcom w (rf[6 f + e]). W.a holds the bodies' velocities under w (the impulse
// RNEA(q, 0, w) without gravity has V = 0, so its accelerations are sum S_k w_k). Turning q_j
// moves the subtree of j rigidly: dV_b = S_j x (V_b - V_P), dc_b = S_j.lin + S_j.ang x c_b, and
// the body's CoM velocity p_b = V_b.lin + V_b.ang x c_b changes by
// dV_b.lin + dV_b.ang x c_b + V_b.ang x dc_b.
MB_HD inline void impulse_com_lane(const Blk& b, const WVals& W, int j, double* Jf, int jw, double* rf) {
  const int nj = b.nj;
  const double* cr = b.C;
  int f = 0;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    const int t = C.type();
    if (t == C_IMPULSE_COM) {
      double S[6], VP[6], AP[6], dq[3] = {0., 0., 0.}, r[3] = {0., 0., 0.}, mt = 0.;
      for (int e = 0; e < 6; ++e) S[e] = W.S(j)[e];
      parent_motion(b, W, j, VP, AP);
      for (int bb = 0; bb < nj; ++bb) {
        if (!carries_body(b, bb)) continue;
        const double mk = *W.m(bb);
        mt += mk;
        double V[6], c[3], t1[3];
        for (int e = 0; e < 6; ++e) V[e] = W.a(bb)[e];
        for (int e = 0; e < 3; ++e) c[e] = W.c(bb)[e];
        if (j == 0) {
          cross3(V + 3, c, t1);
          for (int e = 0; e < 3; ++e) r[e] += mk * (V[e] + t1[e]);
        }
        if (!((*W.anc(bb) >> j) & 1ull)) continue;
        double D[6], dV[6], dc[3], t2[3];
        for (int e = 0; e < 6; ++e) D[e] = V[e] - AP[e];
        cross_m(S, D, dV);
        cross3(S + 3, c, dc);
        for (int e = 0; e < 3; ++e) dc[e] += S[e];
        cross3(dV + 3, c, t1);
        cross3(V + 3, dc, t2);
        for (int e = 0; e < 3; ++e) dq[e] += mk * (dV[e] + t1[e] + t2[e]);
      }
      double tt[3];
      cross3(S + 3, W.ch(j), tt);
      const double m = *W.cm(j);
      for (int e = 0; e < 3; ++e) {
        Jf[((int64_t)f * 6 + e) * jw + j] = dq[e] / mt;
        Jf[((int64_t)f * 6 + 3 + e) * jw + j] = (m * S[e] + tt[e]) / mt;
        if (j == 0) rf[6 * f + e] = r[e] / mt;
      }
    }
    if (jac_cost(b, t)) ++f;
    cr += C.size();
  }
}

// model->calcDiff for one knot by one workgroup (euler.hxx:83-131,
// free-fwddyn.hxx:82-118, contact-fwddyn.hxx:107-160, impulse-fwddyn.hxx:85-127,
// cost-sum.hxx:122-160). Writes full blocks (entries beyond nu zero). A mass
// matrix that is not positive definite leaves NaN in Fx/Fu, which the backward
// pass reports as backward_error. `w`: diff_layout(nj, njac, nc).total doubles of LDS.
// xnext_out / cost_out (may be null): the knot's calc (xnext, cost) as well;
// Fx == nullptr: calc only (no derivative block is written).
#if defined(__HIP_DEVICE_COMPILE__)
// ---- fp64 matrix-core products of the calcDiff (v_mfma_f64_16x16x4_f64) -------
// (fragment maps and mb_mfma: with the tree-sparse LTDL above)
typedef __attribute__((address_space(1))) double mb_glb_d;
// The shape arguments of the two out-of-line products (nj, nc, L ...) and the wave index
// are wave-uniform, but a function's arguments arrive in vector registers, so every loop
// and branch over them is compiled as lane-divergent: exec-mask bookkeeping around each
// k-chunk and each MFMA, and an s_waitcnt lgkmcnt(0) at every join. MB_MFMA_SCALAR_SHAPE
// (set per kernel object, k_mb.hip) moves them to scalar registers on entry, and the loops
// become scalar branches. Measured per kernel ("Round 7"): calcDiff
// -2.8 % on mb_knot_kernel_s2 (more SGPRs: 23 -> 27 VGPR spills), none on the others.
#ifndef MB_MFMA_SCALAR_SHAPE
#define MB_MFMA_SCALAR_SHAPE 0
#endif
#if MB_MFMA_SCALAR_SHAPE
#define MB_MFMA_UNIFORM(x) x = __builtin_amdgcn_readfirstlane(x)
#else
#define MB_MFMA_UNIFORM(x)
#endif
// The Fx block (euler.hxx:100-112 with JintegrateTransport / Jintegrate;
// impulse-fwddyn.hxx:111-115) straight from the da product's accumulators:
// da = -(Kinv_tl dtau + H da0) (contact-fwddyn.hxx:127-140 as computeABADerivatives / the
// KKT inverse), computed transposed, tile rows = the tangent directions c, tile columns =
// the dofs i: a lane's accumulators are da(i, c) for one i and four c, and the 16 lanes of
// a row group store 16 consecutive rows of a column of the column-major Fx. With the
// contact-force costs (nfd = nc) the same product's rows nj + k' ([H^T | -S^-1]) give
// d lambda / dx (contact-fwddyn.hxx:131-137), row-major nc x L into dfx (LDS, or the Fu
// block in the spilled plan: a generic pointer).
// mode: bit 0 impulse, 1 integrated (dt != 0), 2 free-flyer Euler (Jexp6 rows), 3 ok.
// dtau: read from LDS at dts; in the spilled plan dtg is its global copy (the knot's Lxx
// block) and each wave first copies the direction blocks of its tiles into dts (so the
// tiles' loads are LDS loads, which never wait behind the Fx stores); dtg == nullptr:
// dtau is in LDS already. dts == nullptr: the product reads dtg (global) directly.
template <bool GA>  // GA: the A operand read from global memory (dtg) instead of the LDS copy
__device__ __attribute__((noinline)) void da_fx_mfma(const mb_lds_d* Minv, int lda, const mb_lds_d* H,
                                                     const double* dtg, mb_lds_d* dts, const mb_lds_d* da0, int nj,
                                                     int nc, int L, int mode, double dt, const mb_lds_d* Sinv, int nfd,
                                                     double* dfx, const mb_lds_d* Je, const mb_lds_d* Ai,
                                                     const mb_lds_d* Jc, double* Fx, const mb_lds_d* Z) {
  MB_MFMA_UNIFORM(lda);
  MB_MFMA_UNIFORM(nj);
  MB_MFMA_UNIFORM(nc);
  MB_MFMA_UNIFORM(L);
  MB_MFMA_UNIFORM(mode);
  MB_MFMA_UNIFORM(nfd);
  int wave = (int)threadIdx.x >> 6;
  MB_MFMA_UNIFORM(wave);
  const int lane = (int)threadIdx.x & 63, nw = (int)blockDim.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int NR = nj + nfd, tr = (NR + 15) >> 4, tc = (L + 15) >> 4, K = nj + nc, N = 2 * nj;
  const bool imp = mode & 1, integ = mode & 2, ffe = mode & 4, ok = mode & 8;
  const double mul_v = ok ? -1. : (double)NAN, dt2 = dt * dt;
  const int vcols = imp ? nj : L;  // impulse knots: the v columns of da are zero
  mb_glb_d* const F = (mb_glb_d*)Fx;
  const mb_glb_d* const G = (const mb_glb_d*)dtg;
  // tiles direction-block major, a contiguous range per wave: its tiles share their A
  // operands (at most two direction blocks)
  MB_GJ_MARK(22);
  const int per = (tr * tc + nw - 1) / nw, t0 = wave * per;
  const int t1 = (wave + 1) * per < tr * tc ? (wave + 1) * per : tr * tc;
  if (!GA && G && t0 < t1) {  // this wave's direction blocks of dtau into LDS (loads first)
    const int j0 = t0 / tr, j1 = (t1 - 1) / tr;
    for (int tj = j0; tj <= j1; ++tj) {
      const int c = 16 * tj + li;
      // (nj <= 40: the copy's area, 2 nj^2 doubles, fits the world values' only then)
      double v[10];
#pragma unroll
      for (int s = 0; s < 10; ++s) {
        const int k = 4 * s + lk;
        v[s] = (k < nj && c < L) ? (double)G[k * L + c] : 0.;
      }
#pragma unroll
      for (int s = 0; s < 10; ++s) {
        const int k = 4 * s + lk;
        if (k < nj && c < L) dts[k * L + c] = v[s];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  MB_GJ_MARK(25);
  MB_TILE_DECL;
#pragma unroll 1
  for (int tile = t0; tile < t1; ++tile) {
    MB_TILE_START(1);
    const int tj = tile / tr, ti = tile - tj * tr;
    const int i = 16 * ti + li, ca = 16 * tj + li;
    const bool rv = i < nj, rf = !rv && i < NR, cv = ca < L;
    mb_f64x4 acc = {0., 0., 0., 0.};
    // operands from clamped addresses, every load unconditional, then selected (a load
    // under a lane-dependent condition becomes a branch that waits for it: one LDS round
    // trip per k-step); the k-steps in chunks of 8, the chunk's loads first
    const int cac = ca < L ? ca : L - 1;
    const int ic = i < nj ? i : nj - 1, ir = i - nj < 0 ? 0 : (i - nj < nfd ? i - nj : (nfd > 0 ? nfd - 1 : 0));
    if constexpr (!GA) {
      // two k-ranges, each with one operand source per lane and a per-lane stride (no
      // per-step address selects, which became branches): k < nj (A = dtau, B = Kinv_tl
      // rows / H^T columns), then k' = k - nj < nc (A = da0, B = H rows / -S^-1); the
      // padding k-steps masked in both operands (B's rows past the range are whatever the
      // LDS holds: 0 x NaN would poison the tile); loads of 4 k-steps first, then their MFMAs
      const mb_lds_d* pa = dts + (lk * L + cac);
      const mb_lds_d* pb = rv ? Minv + (lk * lda + ic) : (rf ? H + (ir * nj + lk) : Z);
      const int sb = rv ? 4 * lda : (rf ? 4 : 0);
#pragma unroll 1
      for (int k0 = 0; k0 < nj; k0 += 16) {
        double av[4], bw[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          av[s] = pa[(k0 + 4 * s) * L];
          bw[s] = pb[(k0 / 4 + s) * sb];
        }
        MB_TILE_PIN4(av);
        MB_TILE_PIN4(bw);
        MB_TILE_LAP(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = k0 + 4 * s + lk;
          if (k0 + 4 * s < nj) acc = mb_mfma(cv && k < nj ? av[s] : 0., (rv || rf) && k < nj ? bw[s] : 0., acc);
        }
        MB_TILE_LAP(1);
      }
      const mb_lds_d* qa = da0 + (lk * L + cac);
      const mb_lds_d* qb = rv ? H + (lk * nj + ic) : (rf ? Sinv + (lk * nc + ir) : Z);
      const int sq = rv ? 4 * nj : (rf ? 4 * nc : 0);
      const double sg = rf ? -1. : 1.;
#pragma unroll 1
      for (int k0 = 0; k0 < nc; k0 += 16) {
        double av[4], bw[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          av[s] = qa[(k0 + 4 * s) * L];
          bw[s] = qb[(k0 / 4 + s) * sq];
        }
        MB_TILE_PIN4(av);
        MB_TILE_PIN4(bw);
        MB_TILE_LAP(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = k0 + 4 * s + lk;
          if (k0 + 4 * s < nc) acc = mb_mfma(cv && k < nc ? av[s] : 0., (rv || rf) && k < nc ? sg * bw[s] : 0., acc);
        }
        MB_TILE_LAP(1);
      }
    } else {
    // (chunks of 4 k-steps: the chunk's 24 loads issued, pinned by one empty asm that
    // consumes them all, then selected: sunk into the selects' conditions the loads became
    // branches that each wait for their load)
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += 16) {
      double x1[4], x2[4], m1[4], h1[4], h2[4], s2[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + 4 * s + lk;
        const int kc = k < nj ? k : nj - 1, kn = k - nj < 0 ? 0 : (k - nj < nc ? k - nj : (nc > 0 ? nc - 1 : 0));
        // A(c, k) = [dtau; da0](k, c)
        x1[s] = GA ? (double)G[kc * L + cac] : (double)dts[kc * L + cac];
        x2[s] = da0[kn * L + cac];
        // B(k, i) = [Kinv_tl | H](i, k), the force rows nj + k': [H^T | -S^-1](k', k) (S symmetric)
        m1[s] = Minv[kc * lda + ic];
        h1[s] = H[kn * nj + ic];
        h2[s] = H[ir * nj + kc];
        s2[s] = Sinv[kn * nc + ir];
      }
      asm volatile(""
                   : "+v"(x1[0]), "+v"(x1[1]), "+v"(x1[2]), "+v"(x1[3]), "+v"(x2[0]), "+v"(x2[1]), "+v"(x2[2]),
                     "+v"(x2[3]), "+v"(m1[0]), "+v"(m1[1]), "+v"(m1[2]), "+v"(m1[3]), "+v"(h1[0]), "+v"(h1[1]),
                     "+v"(h1[2]), "+v"(h1[3]), "+v"(h2[0]), "+v"(h2[1]), "+v"(h2[2]), "+v"(h2[3]), "+v"(s2[0]),
                     "+v"(s2[1]), "+v"(s2[2]), "+v"(s2[3]));
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + 4 * s + lk;
        const bool km = k < nj, kh = !km && k < K;
        const double av = !cv ? 0. : (km ? x1[s] : (kh ? x2[s] : 0.));
        const double bw = rv ? (km ? m1[s] : (kh ? h1[s] : 0.)) : (rf ? (km ? h2[s] : (kh ? -s2[s] : 0.)) : 0.);
        if (k0 + 4 * s < K) acc = mb_mfma(av, bw, acc);
      }
    }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 16 * tj + lk + 4 * q;
      // da(i, c) (a failed factorisation: NaN; impulse: 0 in the v columns)
      const double dav = acc[q] * (c >= vcols ? 0. * mul_v : mul_v);
      // the free-flyer Euler rows i < 6 mix da(0..5, c): lanes li = 0..5 of this row group
      double d6[6];
      if (ffe && ti == 0)
#pragma unroll
        for (int r = 0; r < 6; ++r) d6[r] = __shfl(dav, (lane & 48) | r);
      if (i >= nj && i < NR && c < vcols) dfx[(i - nj) * L + c] = acc[q];
      if (i >= nj || c >= L) continue;
      double fq, fv;  // Fx(i, c), Fx(nj + i, c)
      if (imp) {  // [[I, 0], [-G dtau_dq - H dv0_dq, G M = I - H Jc]]
        fq = c == i ? 1. : 0.;
        if (c < nj) {
          fv = dav;
        } else {
          double s = 0.;
          for (int k = 0; k < nc; ++k) s += H[k * nj + i] * Jc[k * nj + (c - nj)];
          fv = ok ? (c - nj == i ? 1. : 0.) - s : (double)NAN;
        }
      } else if (!integ) {
        fq = c == i ? 1. : 0.;
        fv = c == nj + i ? 1. : 0.;
      } else {
        if (ffe && i < 6) {  // Jexp6(dq) (da dt^2 + [0 dt I]) + Ad(exp6(dq)^-1)
          double s2 = c < 6 ? Ai[c * 6 + i] : 0.;
#pragma unroll
          for (int r = 0; r < 6; ++r) s2 += Je[r * 6 + i] * (d6[r] * dt2 + (c == nj + r ? dt : 0.));
          fq = s2;
        } else {
          fq = dav * dt2 + (c == nj + i ? dt : 0.) + (c == i ? 1. : 0.);
        }
        fv = dav * dt + (c == nj + i ? 1. : 0.);
      }
      F[(int64_t)c * N + i] = fq;
      F[(int64_t)c * N + nj + i] = fv;
    }
    MB_TILE_LAP(2);
  }
  MB_TILE_FLUSH(32);
  MB_GJ_MARK(23);
}
// The Gauss-Newton blocks sc * (R^T diag(w h) R + the diagonal state / control terms)
// (cost-sum.hxx:122-160) over the combined column space [x tangent (L) | u (m)]: the
// upper-triangle 16 x 16 tiles (bi <= bj) of the (L + m)^2 product; Lxx and Luu are
// written from the upper triangle and mirrored, Lxu from the x-row / u-column tiles.
// wrow[r]: the row's weight times its activation Hessian (w h).
// (noinline: its registers apart from the kernel body's, which is at the VGPR cap here)
__device__ __attribute__((noinline)) void gn_blocks_mfma(const double* Rm, int ldR, const double* wrow, int nrows,
                                                         int L, int nu, int m, double sc, double* Lxx, double* Lxu,
                                                         double* Luu, const double* diag) {
  MB_MFMA_UNIFORM(ldR);
  MB_MFMA_UNIFORM(nrows);
  MB_MFMA_UNIFORM(L);
  MB_MFMA_UNIFORM(nu);
  MB_MFMA_UNIFORM(m);
  int wave = (int)threadIdx.x >> 6;
  MB_MFMA_UNIFORM(wave);
  const int lane = (int)threadIdx.x & 63, nw = (int)blockDim.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int NC = L + m, cv = L + nu, NT = (NC + 15) >> 4, ntiles = NT * (NT + 1) / 2, n = L;
  Rm = lds_ptr(Rm);
  wrow = lds_ptr(wrow);
  diag = lds_ptr(diag);
  MB_TILE_DECL;
#pragma unroll 1
  for (int tile = wave; tile < ntiles; tile += nw) {
    MB_TILE_START(1);
    int bi = 0, rem = tile;
    while (rem >= NT - bi) {
      rem -= NT - bi;
      ++bi;
    }
    const int bj = bi + rem;
    const int ca = 16 * bi + li, cb = 16 * bj + li;
    // (clamped addresses, unconditional loads, then selects: a lane-dependent condition
    // around a load becomes a branch that waits for it)
    const int cac = ca < ldR ? ca : ldR - 1, cbc = cb < ldR ? cb : ldR - 1;
    mb_f64x4 acc = {0., 0., 0., 0.};
    // (the tile's transpose: the accumulator rows run over bj, its columns over bi, so
    // lane li holds row 16 bi + li and the 16 lanes of a column store 128 contiguous
    // bytes of the column-major blocks); chunks of 4 k-steps, the chunk's 12 loads issued
    // first and pinned by one empty asm (not sunk into the selects' branches)
#pragma unroll 1
    for (int k0 = 0; k0 < nrows; k0 += 16) {
      double x[4], y[4], wr[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int r = k0 + 4 * s + lk, rc = r < nrows ? r : nrows - 1;
        const mb_lds_d* Rr = (const mb_lds_d*)Rm + (int64_t)rc * ldR;
        x[s] = Rr[cbc];
        y[s] = Rr[cac];
        wr[s] = ((const mb_lds_d*)wrow)[rc];
      }
      asm volatile(""
                   : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]),
                     "+v"(wr[0]), "+v"(wr[1]), "+v"(wr[2]), "+v"(wr[3]));
      MB_TILE_LAP(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int r = k0 + 4 * s + lk;
        const double a = (r < nrows && cb < cv) ? x[s] : 0.;
        const double bv = (r < nrows && ca < cv) ? y[s] * wr[s] : 0.;
        if (k0 + 4 * s < nrows) acc = mb_mfma(a, bv, acc);
      }
      MB_TILE_LAP(1);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 16 * bi + li, j = 16 * bj + lk + 4 * q;
      if (i > j || j >= NC) continue;
      const double v = sc * (i == j ? acc[q] + diag[i] : acc[q]);
      if (j < L) {  // Lxx (symmetric)
        mb_gstore(Lxx + (int64_t)j * n + i, v);
        if (i < j) mb_gstore(Lxx + (int64_t)i * n + j, v);
      } else if (i < L) {  // Lxu
        mb_gstore(Lxu + (int64_t)(j - L) * n + i, v);
      } else {  // Luu (symmetric)
        mb_gstore(Luu + (int64_t)(j - L) * m + (i - L), v);
        if (i < j) mb_gstore(Luu + (int64_t)(i - L) * m + (j - L), v);
      }
    }
    MB_TILE_LAP(2);
  }
  MB_TILE_FLUSH(36);
}

// The subtree sums of the velocity-product maps (subtree_nh_lane) on the matrix cores:
// Nsub (nj x 42) = T nb with the subtree indicator T[j][b] = 1 when dof j is an ancestor-
// or-self of b and b carries a body; waves w of nw (the caller's numbering) take the
// 16 x 16 output tiles round-robin. (The sums' association changes, not their terms.)
// (AS: the address space of the maps and sums, LDS or the spilled plan's Fx block)
template <class AS>
__device__ __forceinline__ void subtree_nh_mfma(const Blk& b, const WVals& W, const double* nb_, double* ns_, int w,
                                                int nw) {
  const AS* nb = (const AS*)(std::is_same<AS, mb_lds_d>::value ? lds_ptr(nb_) : nb_);
  AS* ns = (AS*)(std::is_same<AS, mb_lds_d>::value ? lds_ptr(ns_) : ns_);
  const int lane = (int)threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int nj = b.nj, tr = (nj + 15) >> 4, tc = 3;  // 42 components in 3 tiles
#pragma unroll 1
  for (int tile = w; tile < tr * tc; tile += nw) {
    const int ti = tile / tc, tj = tile - ti * tc;
    const int j = 16 * ti + li, c = 16 * tj + li;
    mb_f64x4 acc = {0., 0., 0., 0.};
    // the k-steps in chunks of 8: every operand of a chunk loaded first, then its MFMA
    // chain (one LDS round trip per chunk, not per k-step)
#pragma unroll 1
    for (int k0 = 0; k0 < nj; k0 += 32) {
      double av[8], bv[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int bb = k0 + 4 * s + lk;
        const int bs = bb < nj ? bb : 0;
        const double nv = nb[42 * bs + (c < 42 ? c : 0)];
        const bool in = bb < nj && j < nj && carries_body(b, bs) && ((*W.anc(bs) >> j) & 1ull);
        av[s] = in ? 1. : 0.;
        bv[s] = bb < nj && c < 42 ? nv : 0.;
      }
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if (k0 + 4 * s < nj) acc = mb_mfma(av[s], bv[s], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * ti + lk + 4 * q;
      if (row < nj && c < 42) ns[42 * row + c] = acc[q];
    }
  }
}
#endif

// The rows of the impulse CoM costs in the stacked R (lane's entries e = lane (mod nt)):
// d(Jcom w)/dq + Jcom dv+/dq | Jcom (dv+/dv - I), with dv+/dx the bottom rows of Fx (device:
// the block the da product has written, column-major 2 nj x 2 nj; host: from da and H Jc).
// Jf: the jac-cost slots (rows 0..2 d(Jcom w)/dq, 3..5 Jcom).
MB_HD inline void impulse_com_rows(int lane, int nt, const double* csrc, const double* Jf, int jw, double* Rm,
                                            int ldR, int nrows, int nj, int nc, const double* Fx, const double* da,
                                            int Ld, const double* H, const double* Jc, bool ok) {
  const int L = 2 * nj, ne = nrows * ldR;
  for (int e = lane; e < ne; e += nt) {
    const int row = e / ldR, c = e % ldR;
    const int src = (int)mb_lds(csrc)[row];
    if (src < kImpulseComSrc || c >= L) continue;
    const int f = (src - kImpulseComSrc) >> 3, e2 = src & 7;
    const double* Jm = Jf + ((int64_t)f * 6 + 3 + e2) * jw;
    double v = c < nj ? Jf[((int64_t)f * 6 + e2) * jw + c] : -Jm[c - nj];
#if defined(__HIP_DEVICE_COMPILE__)
    const mb_glb_d* Fc = (const mb_glb_d*)Fx + ((int64_t)c * L + nj);
    for (int i = 0; i < nj; ++i) v += Jm[i] * Fc[i];
    (void)nc, (void)da, (void)Ld, (void)H, (void)Jc, (void)ok;
#else
    for (int i = 0; i < nj; ++i) {
      double fv;
      if (c < nj) {
        fv = da[(int64_t)i * Ld + c];
      } else {
        double s = 0.;
        for (int k = 0; k < nc; ++k) s += H[(int64_t)k * nj + i] * Jc[(int64_t)k * nj + (c - nj)];
        fv = ok ? (c - nj == i ? 1. : 0.) - s : NAN;
      }
      v += Jm[i] * fv;
    }
#endif
    mb_lds(Rm)[e] = v;
  }
}

// The two products of an actuation record (tau = S u, S nj x nu column-major) in the calcDiff, on
// every lane of the workgroup: d lambda / du (k, c) = -sum_i H(k, i) S(i, c) into dfu (nc x nj,
// its columns beyond nu zero; null: no force Jacobians) and Kinv_atau S into KS (nj x nu at ld
// lda). A squashed record (tau = S s(u), Dq = ds/du, nu entries; null without): column c of both
// is scaled by Dq[c] here, where they are written, so that their readers (the Fu assembly, the
// force costs' rows) are the linear record's. Out of line on the device, as act_row_dot. dfu may
// be the knot's Fu block (kSpillF).
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline)) void act_products(int lane, int nt, const double* S_, const double* Kinv_, int lda,
                                                       const double* H_, int nj, int nu, int nc, double* dfu,
                                                       double* KS_, const double* Dq_) {
  const double* S = lds_ptr(S_);
  const double* Kinv = lds_ptr(Kinv_);
  const double* H = lds_ptr(H_);
  double* KS = lds_ptr(KS_);
  const double* Dq = Dq_ ? lds_ptr(Dq_) : nullptr;
#else
inline void act_products(int lane, int nt, const double* S, const double* Kinv, int lda, const double* H, int nj, int nu,
                         int nc, double* dfu, double* KS, const double* Dq) {
#endif
  if (dfu)
    for (int e = lane; e < nc * nj; e += nt) {
      const int k = e / nj, c = e % nj;
      double s = 0.;
      if (c < nu) {
        for (int i = 0; i < nj; ++i) s -= H[(int64_t)k * nj + i] * S[(int64_t)c * nj + i];
        if (Dq) s *= Dq[c];
      }
      dfu[e] = s;
    }
  for (int e = lane; e < nj * nu; e += nt) {
    const int c = e / nj, i = e % nj;
    double s = 0.;
    for (int k = 0; k < nj; ++k) s += Kinv[(int64_t)k * lda + i] * S[(int64_t)c * nj + k];
    KS[(int64_t)c * lda + i] = Dq ? s * Dq[c] : s;
  }
}

// SP: the spilled plan fixed at compile time (0 / 1: the device kernels, one variant per
// plan) or taken from `spill` (-1: the host emulation)
template <class X, int SP = -1>
MB_HD __forceinline__ void knot_calc_diff_x(const X& ex, const double* P, int nx, int m, const double* xg, const double* ug,
                                   bool use_u, double* w, double* Fx, double* Fu, double* Lxx, double* Lxu,
                                   double* Luu, double* Lx, double* Lu, double* xnext_out = nullptr,
                                   double* cost_out = nullptr, const double* xu_pre = nullptr, int spill = 0) {
  w = ex.lds(w);  // the work area and the parameter block live in LDS
  P = ex.lds(P);
  const Blk b = parse_uniform(P);
  const bool imp = b.impulse;  // ActionModelImpulseFwdDynamics (impulse-fwddyn.hxx:53-127)
  const int nj = b.nj, nq = b.nq, n = 2 * nj, L = 2 * nj, nc = b.nc, nu = nj - b.nun;
  const int lda = lda_of(nj);
  bool vcols;
  const int njac = count_jac_costs(b, &vcols);
  const int jw = vcols ? L : nj;  // columns of the stored jac-cost Jacobians
  const int nrows = count_cost_rows(b, nu);
  // (calc only, Fx == nullptr: the same plan; it ends before any spilled array is used)
  if (SP == 0) spill = 0;
  if (SP == 1) spill |= kSpillBlocks;
#if MB_ACTUATION
  const DiffLayout l = diff_layout(nj, njac, nc, vcols, nu, nrows, spill, b.S != nullptr, b.sq != nullptr);
  // (a squashed record: s(u), then D(u) = ds/du, one entry per control, formed in the first phase)
  double* const sqs = (b.sq && !imp) ? w + l.sq : nullptr;
#else
  const DiffLayout l = diff_layout(nj, njac, nc, vcols, nu, nrows, spill, b.S != nullptr);
#endif
  const bool spilled = SP >= 0 ? SP == 1 : (spill & kSpillBlocks) != 0;
  // the recursions' per-wave partials (free areas of their phases: DiffLayout)
  const WVals W{w + l.wv, nj, w + l.pk};
  double* A = w + l.A;
  // dtau/dx, the body maps and their subtree sums: LDS, or (spilled) the knot's Lxx / Fx
  // blocks, written there after their last read (DiffLayout)
  double* dtau = spilled ? Lxx : w + l.dtau;
  double* nbm = spilled ? Fx : w + l.nb;
  double* nsub = spilled ? Fx + pad2((int64_t)42 * nj) : w + l.ns;
  double* da = w + l.da;  // (host emulation only)
  const int Ld = L + 1;   // row stride of da (odd: conflict-free column reads)
  double* qp = w + l.qp;
  double* x = w + l.vec;
  double* u = x + nq + nj;
  double* nle = u + nj;   // nle, then RNEA's tau (unused)
  double* av = nle + nj;  // z, then a (impulse: v+)
  double* rf = av + nj;   // jac-cost residuals, 6 per cost
  double* Je = rf + 6 * kMaxJacCosts;  // Jexp6(dq) 6x6
  double* Ai = Je + 36;                // Ad(exp6(dq)^-1) 6x6
  double* Jf = (spill & kSpillJ) ? Lxu : w + l.J;
  double* red = w + l.red;
  int* flag = (int*)(red + 4);
  double* Jc = w + l.Jc;
  double* a0 = w + l.a0;
  double* lam = w + l.lam;
  double* Y = w + l.Y;
  double* H = w + l.H;
  double* Sx = w + l.Sx;
  double* da0 = w + l.da0;
  double* fx = w + l.fx;
  double* zv = w + l.zv;
  ex.run([&](int lane) {
    // xu_pre (device, nq + nj <= nt): this thread's x[lane] / u[lane] loaded by the caller
    // beside the parameter-block copy (one global round trip instead of two)
    if (lane == 0) *(int*)(red + 5) = 0;  // the factorisation's side-work counter
    if (lane == 1) red[7] = 0.;           // an LDS zero (the da product's padding operand)
    if (xu_pre) {
      if (lane < nq + nj) x[lane] = xu_pre[0];
      if (lane < nj) u[lane] = (use_u && lane < nu) ? xu_pre[1] : 0.;
    } else {
      for (int e = lane; e < nq + nj; e += ex.nt) x[e] = xg[e];
      if (lane < nj) u[lane] = (use_u && lane < nu) ? ug[lane] : 0.;  // (impulse: a zero velocity)
    }
  });
  // world-frame kinematics, M into the left half of [M | I], nle
  world_kinematics(ex, b, W, x, A, lda, [](int, int) {}, [](int, int) {}, true);
  if (!imp) world_rnea(ex, b, W, x + nq, nullptr, nle);
  if (nc > 0)  // contact rows at the drift (ddq = 0; ContactModelMultiple::calc)
    ex.run([&](int lane) {
      if (lane < nj) contact_jac_lane(b, W, lane, Jc, nullptr);
      // the a0 terms on the next wave (not after the Jacobian columns on wave 0: a wave
      // runs its divergent lanes' paths one after another)
      for (int k = lane - 64; k >= 0 && k < (imp ? 0 : b.ncon); k += ex.nt) {
        int row0;
        const CRec C{contact_rec(b, k, &row0)};
        contact_a0_position(b, W, C, a0 + row0);
        contact_a0_drift(b, W, C, a0 + row0);
      }
    });
  MB_DUMP(0, A, nj, nj, lda);        // M (+ armature)
  if (!imp) MB_DUMP(1, nle, nj, 1, nj);
  if (nc > 0) {
    MB_DUMP(2, Jc, nj, nc, nj);         // Jc^T (nj x nc)
    MB_DUMP(3, a0, nc, 1, nc);
  }
  double* pb = red + 8;
  // M^-1 by the tree-sparse LTDL of M (tree_ltdl), into the second half of the A area
  // (column-major nj x nj, ld lda); with contacts: d a / d tau after the Schur step.
  double* Minv = A + l.half;
  // The velocity-product maps of the derivatives (per-body N_b, h_b into the dtau area;
  // their subtree sums into the da area; P_k, Q_k) and the cost-Jacobian columns need the
  // velocities and composite inertias only: on the device the waves the factorisation
  // leaves idle build them meanwhile, one map per slot (vp: how many are built), the
  // Jacobian columns beside the body maps when the idle waves are at least two (jac_side).
  // (unused by impulse knots)
  auto vp_side = [&](int slot, int sl, int snt) {
    if (slot == 0) {
      if (!imp)
        for (int d = sl; d < nj; d += 64) body_nh_lane(b, W, d, nbm);
      if (snt >= 128)
        for (int id = sl - 64; id >= 0 && id < nj * njac; id += snt - 64)
          jac_lane(b, W, x, id % nj, Jf, jw, rf, nullptr, nullptr, nullptr, id / nj);
    } else if (slot == 1 && !imp) {
#if defined(__HIP_DEVICE_COMPILE__)
      if (spilled)
        subtree_nh_mfma<mb_glb_d>(b, W, nbm, nsub, sl >> 6, snt >> 6);
      else
        subtree_nh_mfma<mb_lds_d>(b, W, nbm, nsub, sl >> 6, snt >> 6);
#endif
    } else if (slot == 2 && !imp) {
      for (int j = sl; j < nj; j += snt) qp_lane_ns(W, j, nsub, qp);
    }
  };
#if defined(__HIP_DEVICE_COMPILE__)
  // scratch of the factorisation: the depth levels and 1 / D in pb; in the M^-1 area (free
  // until tree_minv, nj lda >= nj^2 doubles) the fast path's rows ((md + 1) nj) or the
  // generic steps' dof masks (2 nj), which never run together
  const int md = tree_depth(b, W);
  // (calc only: no derivative work beside the factorisation)
  const int vp = (md < kTreeKD && ex.nt >= 128 && Fx) ? 3 : 0;
  const bool jac_side = vp > 0 && ex.nt - 64 >= 128;
  double* const tp = ex.lds(Minv);
  const TreeWork tw{(Mask*)tp, (Mask*)tp + nj, (Mask*)ex.lds(pb), ex.lds(pb) + 64, ex.lds(flag)};
  tree_ltdl(ex, b, W, A, lda, tw, md, tp, vp_side, vp, (int*)(red + 5));
#else
  // (host emulation: the factorisation's scratch in an area of its own, no side work)
  const int vp = 0;
  const bool jac_side = false;
  double* const tp = w + l.ht;
  const TreeWork tw{(Mask*)tp, (Mask*)tp + nj, (Mask*)ex.lds(pb), tp + 2 * nj, ex.lds(flag)};
  tree_ltdl(ex, b, W, A, lda, tw, tree_depth(b, W), tp + 3 * nj);
#endif
  bool ok = tree_minv(ex, b, A, lda, tw, Minv);
  Minv = ex.lds(Minv);
  MB_DUMP(4, Minv, nj, nj, lda);
#if MB_ACTUATION
  // (an actuation record: tau = S u, or S s(u), once per dof, -(tau - nle) over nle, which is dead after
  // the next phase; the branch is uniform)
  const double* const Sa = (b.S && !imp) ? ex.lds(b.S) : nullptr;
  if (sqs)  // (s(u) and ds/du, two square roots per control, once per knot)
    ex.run([&](int lane) {
      if (lane < nu) squash_eval(b.sq, nu, lane, u[lane], sqs, true);
    });
  if (Sa)
    ex.run([&](int lane) {
      if (lane < nj) nle[lane] = -(act_tau(b, sqs ? sqs : u, lane) - nle[lane]);
    });
#else
  const double* const Sa = nullptr;
  const double* const sqs = nullptr;
#endif
  // z = (M + A)^-1 (tau - nle) (the acceleration without contacts); Y = Minv Jc^T
  ex.run([&](int lane) {
    if (lane < nj && imp) {
      av[lane] = x[nq + lane];  // z = M^-1 (M v) = v
      zv[lane] = 0.;
      if (lane == 0)
        for (int e = 0; e < 6; ++e) W.root_a()[e] = 0.;  // the impulse RNEA has no gravity
    } else if (lane < nj) {
      double s = 0.;
      if (Sa)
        for (int k = 0; k < nj; ++k) s += Minv[(int64_t)k * lda + lane] * (0. - nle[k]);
      else
        for (int k = 0; k < nj; ++k) s += Minv[(int64_t)k * lda + lane] * ((k < b.nun ? 0. : u[k - b.nun]) - nle[k]);
      av[lane] = ok ? s : NAN;
    }
    for (int e = lane; e < nj * nc; e += ex.nt) {
      const int k = e / nj, i = e % nj;
      double s = 0.;
      for (int r = 0; r < nj; ++r) s += Minv[(int64_t)r * lda + i] * Jc[(int64_t)k * nj + r];
      Y[e] = s;
    }
  });
  if (nc > 0) {
    // [S | I | Jc z + a0], S = Jc Y + damping I; Gauss-Jordan -> [. | S^-1 | S^-1 r]
    ex.run([&](int lane) {
      for (int e = lane; e < nc * (2 * nc + 1); e += ex.nt) {
        const int col = e / nc, row = e % nc;
        double v;
        if (col < nc) {
          double s = 0.;
          for (int i = 0; i < nj; ++i) s += Jc[(int64_t)row * nj + i] * Y[(int64_t)col * nj + i];
          v = s + (row == col ? b.damping : 0.);
        } else if (col < 2 * nc) {
          v = (col - nc == row) ? 1. : 0.;
        } else {
          double s = 0.;
          for (int i = 0; i < nj; ++i) s += Jc[(int64_t)row * nj + i] * av[i];
          v = imp ? (1. + b.r_coeff) * s : s + a0[row];  // impulse: Jc v+ = -r Jc v
        }
        Sx[e] = v;
      }
    });
    ok = gauss_jordan<1>(ex, Sx, nc, nc, 2 * nc + 1, flag, pb) && ok;
    // lambda = -S^-1 r, a = z + Y lambda, H = Y S^-1 (= Kinv top-right)
    ex.run([&](int lane) {
      const double* Sinv = Sx + (int64_t)nc * nc;
      const double* sr = Sx + (int64_t)2 * nc * nc;
      if (lane < nc) lam[lane] = -sr[lane];
      if (lane < nj) {
        double s = av[lane];
        for (int k = 0; k < nc; ++k) s -= Y[(int64_t)k * nj + lane] * sr[k];
        av[lane] = ok ? s : NAN;
      }
      for (int e = lane; e < nj * nc; e += ex.nt) {
        const int k = e / nj, i = e % nj;
        double s = 0.;
        for (int m2 = 0; m2 < nc; ++m2) s += Y[(int64_t)m2 * nj + i] * Sinv[(int64_t)k * nc + m2];
        H[e] = s;
      }
    });
    // Kinv top-left Minv - H Y^T (in place); contact forces per dof (world)
    ex.run([&](int lane) {
      for (int e = lane; e < nj * nj; e += ex.nt) {
        const int c = e / nj, i = e % nj;
        double s = Minv[(int64_t)c * lda + i];
        for (int k = 0; k < nc; ++k) s -= H[(int64_t)k * nj + i] * Y[(int64_t)k * nj + c];
        Minv[(int64_t)c * lda + i] = s;
      }
      if (lane < nj) {
        contact_joint_forces(b, W, lam, fx, lane);
        if (imp) zv[lane] = av[lane] - x[nq + lane];  // v+ - v
      }
    });
  }
  MB_DUMP(5, Minv, nj, nj, lda);  // Kinv top-left (with contacts)
  MB_DUMP(6, av, nj, 1, nj);      // a
  if (nc > 0) {
    MB_DUMP(7, Y, nj, nc, nj);
    MB_DUMP(8, Sx + (int64_t)nc * nc, nc, nc, nc);  // S^-1
    MB_DUMP(9, H, nj, nc, nj);
  }
  // velocities, accelerations and forces at the solved a (the linearisation point
  // of computeABADerivatives / computeRNEADerivatives with fext)
  // (impulse: RNEA(q, 0, v+ - v) without gravity, impulse-fwddyn.hxx:102-104)
  // (the partials in the first half of A in the spilled plan: M is dead, Y too)
  world_rnea(ex, b, WVals{W.base, nj, w + l.pr}, imp ? u : x + nq, imp ? zv : av, nle, nc > 0 ? fx : nullptr);
  if (xnext_out || cost_out) {  // the knot's calc, fused (iteration 0 of a solve, or calc only)
    ex.run([&](int lane) {
      const double dt = b.dt;
      if (xnext_out && lane < nj) {
        if (imp) {
          xnext_out[lane] = x[lane];
          if (lane == nj - 1 && b.ff) xnext_out[nq - 1] = x[nq - 1];
          xnext_out[nq + lane] = av[lane];
        } else if (dt != 0.) {
          euler_step(b, x, av, dt, xnext_out, lane);
        } else {
          xnext_out[lane] = x[lane];
          if (lane == nj - 1 && b.ff) xnext_out[nq - 1] = x[nq - 1];
          xnext_out[nq + lane] = x[nq + lane];
        }
      }
      if (cost_out && !Fx && lane == 0) {  // calc only (with derivatives: from the residuals below)
        double cc = cost_value(b, W, x, u, nu);
        const double* cr = b.C;
        for (int k = 0; k < b.ncost; ++k) {
          const CRec C{cr};
          if (force_cost(C.type())) cc += C.weight() * force_cost_activation(b, C, lam, nu);
          if (C.type() == C_IMPULSE_COM) {  // Jcom (v+ - v) from the bodies' velocities in W.a
            double r[3] = {0., 0., 0.}, mt = 0., a = 0.;
            for (int bb = 0; bb < nj; ++bb) {
              if (!carries_body(b, bb)) continue;
              const double mk = *W.m(bb);
              double t1[3];
              cross3(W.a(bb) + 3, W.c(bb), t1);
              mt += mk;
              for (int e = 0; e < 3; ++e) r[e] += mk * (W.a(bb)[e] + t1[e]);
            }
            const Act act = cost_act(b, C, nu);
            for (int e = 0; e < 3; ++e) a += act.value2(e, r[e] / mt);
            cc += C.weight() * (0.5 * a);
          }
          cr += C.size();
        }
        *cost_out = dt != 0. ? dt * cc : cc;
      }
    });
  }
  if (!Fx) return;  // calc only
  const double dt = b.dt, dt2 = dt * dt;
  const bool integ = dt != 0.;
  const bool ffe = b.ff && integ && !imp;  // Euler on the free-flyer: Jexp6 / Ad(exp6^-1)
  // per-dof Q_k, P_k (lanes < nj) and the jac-cost Jacobians / residuals; the
  // free-flyer Euler step's Jexp6 and Ad(exp6(dq)^-1) (dq = v dt + a dt^2)
  // per-body velocity-product maps, then their subtree sums (DiffLayout nb / ns)
  // (the maps the factorisation's idle waves did not build)
  if (!imp && vp < 1)
    ex.run([&](int lane) {
      if (lane < nj) body_nh_lane(b, W, lane, nbm);
    });
  if (!imp && vp < 2)
    ex.run([&](int lane) {
      const int w = lane >> 6, j = lane & 63;
#if defined(__HIP_DEVICE_COMPILE__)
      (void)j;
      if (spilled)
        subtree_nh_mfma<mb_glb_d>(b, W, nbm, nsub, w, ex.nt >> 6);
      else
        subtree_nh_mfma<mb_lds_d>(b, W, nbm, nsub, w, ex.nt >> 6);
#else
      if (j < nj) {
        if (ex.nt >= 512)
          subtree_nh_lane<6>(b, W, j, nbm, nsub, w, ex.nt >> 6);
        else
          subtree_nh_lane<11>(b, W, j, nbm, nsub, w, ex.nt >> 6);
      }
#endif
    });
  // the velocity-product maps (if still to do) on the lower half of the workgroup, the
  // cost / Euler Jacobians on the rest (independent: they run side by side)
  ex.run([&](int lane) {
    const int h = !imp && vp < 3 ? ex.nt / 2 : 0;
    if (lane < h) {
      for (int j = lane; j < nj; j += h) qp_lane_ns(W, j, nsub, qp);
      return;
    }
    double dq[6];
    if (ffe)
      for (int e = 0; e < 6; ++e) dq[e] = x[nq + e] * dt + av[e] * dt2;
    if (jac_side) {  // the Jacobian columns are done: the free-flyer Euler terms only
      if (ffe && lane - h < 6) jac_lane(b, W, x, lane - h, Jf, jw, rf, dq, Je, Ai, -2);
      return;
    }
    for (int j = lane - h; j < nj; j += ex.nt - h) jac_lane(b, W, x, j, Jf, jw, rf, ffe ? dq : nullptr, Je, Ai);
  });
  if (imp) {  // V = 0 in the impulse RNEA: P_k = 0, Q_k = Ycrb_k S_k
    // (beside it, from the second wave on: the impulse CoM costs' Jacobian slots and residuals,
    // from the bodies' velocities under v+ - v that the RNEA above left in W.a)
    const bool icom = has_impulse_com(b);
    ex.run([&](int lane) {
      if (icom)
        for (int j = lane - 64; j >= 0 && j < nj; j += ex.nt - 64) impulse_com_lane(b, W, j, Jf, jw, rf);
      if (lane >= nj) return;
      comp_mul(W, lane, W.S(lane), qp + 12 * lane);
      for (int e = 0; e < 6; ++e) qp[12 * lane + 6 + e] = 0.;
    });
  }
  // tangent directions: dtau/dx (impulse: q only) and da0/dx side by side: one lane per
  // da0 direction (at most half the workgroup), the rest for dtau
  ex.run([&](int lane) {
    const int hc = (nc > 0 && !imp) ? (L < ex.nt / 2 ? L : ex.nt / 2) : 0;
    const int h = ex.nt - hc;
    if (lane < h) {
      // (direction, row part) per lane: a direction's rows split over up to 3 lanes when
      // the half-workgroup has the lanes for it
      const int nd = imp ? nj : L;
      const int np = h >= 3 * nd ? 3 : (h >= 2 * nd ? 2 : 1);
      for (int id = lane; id < nd * np; id += h)
        dtau_direction(b, W, qp, id % nd, L, dtau, imp ? nullptr : nsub, id / nd, np);
    } else {
      for (int dd = lane - h; dd < L; dd += hc) contact_direction(b, W, dd, L, da0);
    }
  });
  if (imp && nc > 0) {  // velocities at v+, then d(Jc v+)/dq
    ex.run([&](int lane) {
      if (lane < nj) w_velocity(W, av, lane);
    });
    ex.run([&](int lane) {
      for (int j = lane; j < nj; j += ex.nt) impulse_direction(b, W, j, L, da0);
    });
  }
  // d lambda / dx, d lambda / du for CostModelContactForce (contact-fwddyn.hxx:131-137, with
  // enable_force): Kinv bottom-left = H^T, bottom-right = -S^-1; dtau/du = [0; I]
  // (impulse knots, section flag 3: d Lambda / dx = [H^T dtau_dq - S^-1 dv0_dq, -S^-1 Jc], the
  // exact derivative at r_coeff = 0, the restitution terms dropped otherwise as in Fx; no du)
  const bool fd = b.enable_force && nc > 0;
  // (kSpillF: in the knot's Fu block, written last)
  double* dfx = (spill & kSpillF) ? Fu : w + l.dfx;
  double* dfu = (spill & kSpillF) ? Fu + pad2((int64_t)nc * L) : w + l.dfu;
  const double sc = integ ? dt : 1.;
  // cost-derivative area (layout: group table 4 kMaxCosts | Arr, Ar mul, Ar val,
  // source per row | R rows)
  double* cg = w + l.R;
  double* ch = cg + 4 * kMaxCosts;
  double* cam = ch + kMaxCostRows;
  double* cav = cam + kMaxCostRows;
  double* csrc = cav + kMaxCostRows;
  double* cgi = csrc + kMaxCostRows;  // group of each row
  double* cdg = w + l.Rr;             // device: the state / control diagonal terms per column
  double* Rm = cdg + kMaxCostCols;
  const int ldR = cost_rows_ld(nj, nu);
  // da = -Kinv_tl dtau - H da0 (impulse: -G dtau_dq - H dv0_dq on the q columns) on all
  // lanes but the last ncost, which build the cost-derivative table meanwhile (its area may be
  // the world-value area, dead since the tangent-direction phase)
  ex.run([&](int lane) {
    const int nl = ex.nt - (b.ncost > 0 ? b.ncost : 1);
#if defined(__HIP_DEVICE_COMPILE__)
    // on the matrix cores, every wave (the whole workgroup is converged here), the product's
    // epilogue writing the Fx block
    {
      const int mode = (imp ? 1 : 0) | (integ ? 2 : 0) | (ffe ? 4 : 0) | (ok ? 8 : 0);
      const mb_lds_d* SiL = (const mb_lds_d*)lds_ptr(Sx + (int64_t)nc * nc);
      // dtau: LDS (all-LDS plan), or the Lxx block copied into the LDS staging area / read
      // in place (spilled plan without room for the copy)
      // (an explicit flag: the copy's area may sit at LDS address 0)
      const double* dtg = spilled ? dtau : nullptr;
      const bool staged = !spilled || l.dts >= 0;
      mb_lds_d* dts = !spilled ? (mb_lds_d*)lds_ptr(dtau) : (mb_lds_d*)lds_ptr(w + (l.dts >= 0 ? l.dts : 0));
      const mb_lds_d* Z = (const mb_lds_d*)lds_ptr(red + 7);  // (0, set in the first phase)
      if (staged)
        da_fx_mfma<false>((const mb_lds_d*)lds_ptr(Minv), lda, (const mb_lds_d*)lds_ptr(H), dtg, dts,
                          (const mb_lds_d*)lds_ptr(da0), nj, nc, L, mode, dt, SiL, fd ? nc : 0, dfx,
                          (const mb_lds_d*)lds_ptr(Je), (const mb_lds_d*)lds_ptr(Ai), (const mb_lds_d*)lds_ptr(Jc),
                          Fx, Z);
      else
        da_fx_mfma<true>((const mb_lds_d*)lds_ptr(Minv), lda, (const mb_lds_d*)lds_ptr(H), dtg, dts,
                         (const mb_lds_d*)lds_ptr(da0), nj, nc, L, mode, dt, SiL, fd ? nc : 0, dfx,
                         (const mb_lds_d*)lds_ptr(Je), (const mb_lds_d*)lds_ptr(Ai), (const mb_lds_d*)lds_ptr(Jc),
                         Fx, Z);
    }
    constexpr bool dfx_done = true;
    (void)nl;
#else
    constexpr bool dfx_done = false;
    // two entries per lane at a time: two independent dot-product chains, so the LDS
    // loads of one overlap the other's FMAs (each entry's summation order unchanged)
    const int ne = nj * L;
    for (int e0 = lane; e0 < ne && lane < nl; e0 += 2 * nl) {
      const int e1 = e0 + nl < ne ? e0 + nl : e0;
      const int r0 = e0 / L, c0 = e0 % L, r1 = e1 / L, c1 = e1 % L;
      double s0 = 0., s1 = 0.;
      for (int k = 0; k < nj; ++k) {
        s0 += Minv[(int64_t)k * lda + r0] * dtau[(int64_t)k * L + c0];
        s1 += Minv[(int64_t)k * lda + r1] * dtau[(int64_t)k * L + c1];
      }
      for (int k = 0; k < nc; ++k) {
        s0 += H[(int64_t)k * nj + r0] * da0[(int64_t)k * L + c0];
        s1 += H[(int64_t)k * nj + r1] * da0[(int64_t)k * L + c1];
      }
      if (imp && c0 >= nj) s0 = 0.;
      if (imp && c1 >= nj) s1 = 0.;
      da[(int64_t)r0 * Ld + c0] = ok ? -s0 : NAN;
      if (e1 != e0) da[(int64_t)r1 * Ld + c1] = ok ? -s1 : NAN;
    }
#endif
    if (fd) {
      const double* Sinv = Sx + (int64_t)nc * nc;
      for (int e = lane; e < (dfx_done ? 0 : nc * (imp ? nj : L)); e += ex.nt) {
        const int k = e / (imp ? nj : L), c = e % (imp ? nj : L);
        double s = 0.;
        for (int i = 0; i < nj; ++i) s += H[(int64_t)k * nj + i] * dtau[(int64_t)i * L + c];
        for (int m2 = 0; m2 < nc; ++m2) s -= Sinv[(int64_t)m2 * nc + k] * da0[(int64_t)m2 * L + c];
        dfx[(int64_t)k * L + c] = s;
      }
      if (imp) {  // d Lambda / dv = -H^T M = -S^-1 Jc (no dtau / dv0 columns there)
        const double* const SiL = ex.lds(Sinv);
        const double* const JcL = ex.lds(Jc);
        for (int e = lane; e < nc * nj; e += ex.nt) {
          const int k = e / nj, c = e % nj;
          double s = 0.;
          for (int m2 = 0; m2 < nc; ++m2) s -= SiL[(int64_t)m2 * nc + k] * JcL[(int64_t)m2 * nj + c];
          const int64_t o = (int64_t)k * L + nj + c;
          if (spill & kSpillF)  // (the Fu block: a global store; else LDS)
            mb_gstore(dfx + o, s);
          else
            ex.lds(dfx)[o] = s;
        }
      }
      if (!Sa)
        for (int e = lane; e < nc * nj; e += ex.nt) {
          const int k = e / nj, c = e % nj;
          dfu[e] = c < nu ? -H[(int64_t)k * nj + b.nun + c] : 0.;
        }
    }
    // an actuation record: d lambda / du = -H^T S and da / du = Kinv_atau S (what the Fu assembly
    // reads), each formed once per knot (squashed: their columns times ds/du)
    if (Sa) act_products(lane, ex.nt, Sa, ex.lds(Minv), lda, ex.lds(H), nj, nu, nc, fd ? dfu : nullptr, ex.lds(w + l.KS), sqs ? sqs + nu : nullptr);
    // the cost-derivative table: groups in cost (name) order, each the rows of one cost
    // with a dense residual Jacobian, or the diagonal of a state / control cost; per row
    // Arr (hess), and Ar as amul * aval (the quadratic kinds' (w, r), so the gradient
    // keeps the order (X w) r of the reference's R^T (w r)). Cost k on lane
    // spread_lane(k) after the da tiles (host: lane nt-1-k, which has no da entries), from
    // its group / row / jac-cost offsets, prefix-counted.
#if defined(__HIP_DEVICE_COMPILE__)
    const int kk = spread_item(lane, ex.nt);  // (every lane ran the da tiles)
    if (kk < (b.ncost > 0 ? b.ncost : 1)) {
#else
    if (lane >= nl) {
      const int kk = ex.nt - 1 - lane;
#endif
      int g = 0, row = 0, f = 0;
      const double* cr = b.C;
      for (int k = 0; k < kk; ++k) {  // offsets of record kk
        const CRec C{cr};
        const int t = C.type();
        if (jac_cost(b, t)) {
          row += jac_rows(t);
          ++g;
          ++f;
        }
        if (t == C_STATE || t == C_CONTROL) ++g;
        if (fd && force_cost(t) && (int)C.d()[0] >= 0) {
          row += cost_act(b, C, nu).nr;
          ++g;
        }
        cr += C.size();
      }
      if (kk < b.ncost) {
        const CRec C{cr};
        const int t = C.type();
        const Act act = cost_act(b, C, nu);
        const double co = (double)(cr - P);
        if (jac_cost(b, t)) {
          const int r0 = row;
          for (int e = 0; e < jac_rows(t); ++e, ++row) {
            const double rv = rf[6 * f + e];
            ch[row] = act.hess(e, rv);
            cam[row] = act.kind <= A_WEIGHTED_QUAD ? act.p[e] : 1.;
            cav[row] = act.kind <= A_WEIGHTED_QUAD ? rv : act.sgrad(e, rv, 1.);
            // (the impulse CoM cost's rows marked in the source itself: the rows phase tells
            // them apart without a look at the group table)
            csrc[row] = (double)((t == C_IMPULSE_COM ? kImpulseComSrc : 0) + f * 8 + e);
            cgi[row] = g;
          }
          cg[4 * g] = r0;
          cg[4 * g + 1] = row;
          cg[4 * g + 2] = co;
          // 0: q columns only, 1: x columns
          cg[4 * g + 3] = (t == C_FRAME_VELOCITY || t == C_CENTROIDAL_MOMENTUM) ? 1. : 0.;
          ++g;
          ++f;
        }
        if (t == C_STATE || t == C_CONTROL) {  // diagonal part (state: beyond the free-flyer block)
          cg[4 * g] = -1.;
          cg[4 * g + 1] = t == C_STATE ? 0. : 1.;
          cg[4 * g + 2] = co;
          cg[4 * g + 3] = 0.;
          ++g;
        }
        if (fd && force_cost(t) && (int)C.d()[0] >= 0) {
          const int r0 = row;
          for (int e = 0; e < act.nr; ++e, ++row) {
            const double rv = force_res(C, lam, e);
            ch[row] = act.hess(e, rv);
            cam[row] = act.kind <= A_WEIGHTED_QUAD ? act.p[e] : 1.;
            cav[row] = act.kind <= A_WEIGHTED_QUAD ? rv : act.sgrad(e, rv, 1.);
            csrc[row] = -1. - e;
            cgi[row] = g;
          }
          cg[4 * g] = r0;
          cg[4 * g + 1] = row;
          cg[4 * g + 2] = co;
          cg[4 * g + 3] = 2.;  // x and u columns
          ++g;
        }
      }
      if (kk == (b.ncost > 0 ? b.ncost - 1 : 0)) cg[4 * kMaxCosts - 1] = g;  // the group count
    }
#if defined(__HIP_DEVICE_COMPILE__)
    MB_GJ_MARK(24);
#endif
  });
  // Output blocks in row pairs over all lanes: consecutive lanes write consecutive
  // 16-B pairs of the column-major blocks (n even, blocks 16-B aligned); the lane's
  // (column, row pair) advances by nt pairs without a division. Columns c0.. of [Fx | Fu],
  // after the residual rows (DiffLayout kSpillF): the host's last phase writes both; on the
  // device the da product wrote Fx, and Fu is written at the end of the last phase.
  auto assemble = [&](int lane, int c0) __attribute__((always_inline)) {
    // the operands re-asserted as LDS here: without it the inference lost them and they
    // were flat loads, each waiting (vmcnt) for the output stores issued before it
    const double* const daL = ex.lds(da);
    // (with an actuation record: Kinv_atau S, its column c where the other path reads column
    // nun + c of Kinv_atau)
    const double* const MinvL = ex.lds(Sa ? w + l.KS : Minv);
    const double* const HL = ex.lds(H);
    const double* const JcL = ex.lds(Jc);
    const double* const JeL = ex.lds(Je);
    const double* const AiL = ex.lds(Ai);
    // this phase's invariants laundered into fresh registers: kept in spill slots across
    // the kernel they were reloaded in every iteration, and a scratch reload after an
    // output store waits (vmcnt, in order) for that store to reach memory
    const int NJ = mb_launder(nj), NC = mb_launder(nc), LD = mb_launder(Ld), NU = mb_launder(nu);
    const int LDA = mb_launder(lda), NUN = mb_launder(Sa ? 0 : b.nun), N = mb_launder(n), M = mb_launder(m);
    const double DT = mb_launder(dt), DT2 = mb_launder(dt2);
    const int flags = mb_launder((imp ? 1 : 0) | (integ ? 2 : 0) | (ffe ? 4 : 0) | (ok ? 8 : 0));
    const bool IMP = flags & 1, INTEG = flags & 2, FFE = flags & 4, OK = flags & 8;
    double* const FX = Fx;
    double* const FU = Fu;
    // Fx(i, c): Euler assembly (euler.hxx:100-112) with JintegrateTransport / Jintegrate
    // (both inlined, capturing copies: a closure left in scratch made every captured value a
    // scratch load of its address and a flat load of the value)
    auto fx_at = [=](int i, int c) __attribute__((always_inline)) -> double {
      if (IMP) {  // [[I, 0], [-G dtau_dq - H dv0_dq, G M = I - H Jc]] (impulse-fwddyn.hxx:111-115)
        if (i < NJ) return c == i ? 1. : 0.;
        if (c < NJ) return daL[(int64_t)(i - NJ) * LD + c];
        double s = 0.;
        for (int k = 0; k < NC; ++k) s += HL[(int64_t)k * NJ + (i - NJ)] * JcL[(int64_t)k * NJ + (c - NJ)];
        return OK ? (c - NJ == i - NJ ? 1. : 0.) - s : NAN;
      }
      if (!INTEG) return c == i ? 1. : 0.;
      if (i < NJ && FFE && i < 6) {  // Jexp6(dq) (da dt^2 + [0 dt I]) + Ad(exp6(dq)^-1)
        double s = c < 6 ? AiL[c * 6 + i] : 0.;
        for (int r = 0; r < 6; ++r) s += JeL[r * 6 + i] * (daL[(int64_t)r * LD + c] * DT2 + (c == NJ + r ? DT : 0.));
        return s;
      }
      if (i < NJ) return daL[(int64_t)i * LD + c] * DT2 + (c == NJ + i ? DT : 0.) + (c == i ? 1. : 0.);
      return daL[(int64_t)(i - NJ) * LD + c] * DT + (c == i ? 1. : 0.);
    };
    // Fu(i, c) = Kinv_tl(i mod nj, nun + c) dt^2 | dt (dtau/du = [0; I]; with an actuation
    // record (Kinv_tl S)(i mod nj, c)), Jexp6 on the free-flyer rows
    auto fu_at = [=](int i, int c) __attribute__((always_inline)) -> double {
      if (!(INTEG && c < NU && !IMP)) return 0.;
      if (i < NJ && FFE && i < 6) {
        double s = 0.;
        for (int r = 0; r < 6; ++r) s += JeL[r * 6 + i] * MinvL[(int64_t)(NUN + c) * LDA + r];
        return OK ? s * DT2 : NAN;
      }
      const double mi = OK ? MinvL[(int64_t)(NUN + c) * LDA + (i < NJ ? i : i - NJ)] : NAN;
      return i < NJ ? mi * DT2 : mi * DT;
    };
    // the free-flyer Euler rows (Jexp6 products, 6 terms each) on lanes of their own,
    // so the row pairs below all take the short path (a wave pays for its slowest lane)
    const int r6 = FFE ? 6 : 0;
    for (int e = lane + r6 * c0; e < r6 * (N + M); e += ex.nt) {
      const int c = e / 6, i = e - 6 * c;
      if (c < N)
        mb_gstore(FX + (int64_t)c * N + i, fx_at(i, c));
      else
        mb_gstore(FU + (int64_t)(c - N) * N + i, fu_at(i, c - N));
    }
    const int p0 = r6 >> 1, hp = (N >> 1) - p0, dq = ex.nt / hp, dr = ex.nt % hp;
    for (int c = c0 + lane / hp, ip = lane % hp; c < N + M;) {
      const int i = 2 * (p0 + ip);
      if (c < N)
        mb_gstore2(FX + (int64_t)c * N + i, fx_at(i, c), fx_at(i + 1, c));
      else
        mb_gstore2(FU + (int64_t)(c - N) * N + i, fu_at(i, c - N), fu_at(i + 1, c - N));
      c += dq;
      ip += dr;
      if (ip >= hp) ip -= hp, ++c;
    }
  };
  // the stacked residual Jacobians R (nrows x (L + nu), ld ldR): jac-cost rows from
  // their q (or x) columns, force-cost rows from d lambda / dx, du
  const int ngr = (int)cg[4 * kMaxCosts - 1];
  ex.run([&](int lane) {
    // entry e of the rows (the Jacobians and d lambda / dx, du may be in global memory:
    // four entries' loads issued before their stores)
    auto rentry = [&](int e) __attribute__((always_inline)) -> double {
      const int row = e / ldR, c = e % ldR;
      const int src = (int)csrc[row];
      double v = 0.;
      if (src >= 0) {  // jac cost f, row e2
        // (an impulse CoM cost's row, src >= kImpulseComSrc: its slot's first rows as a
        // placeholder here, the row itself formed after these, below)
        const int f = (src & (kImpulseComSrc - 1)) >> 3, e2 = src & 7;
        const bool xc = c < nj || (c < L && jw == L);
        v = xc ? Jf[((int64_t)f * 6 + e2) * jw + c] : 0.;
        // a q-only cost stored with jw = L carries zeros in its velocity columns
        if (c >= nj && c < L && jw == L && cg[4 * (int)cgi[row] + 3] == 0.) v = 0.;
      } else {  // force cost row -1 - src of its group
        const CRec C{P + (int64_t)cg[4 * (int)cgi[row] + 2]};
        const int e2 = -1 - src;
        if (c < L)
          v = force_jac(C, dfx + c, L, e2);
        else if (c - L < nu)
          v = force_jac(C, dfu + (c - L), nj, e2);
      }
      return c < L + nu ? v : 0.;
    };
    const int ne = nrows * ldR;
    for (int e0 = lane; e0 < ne; e0 += 2 * ex.nt) {
      double v4[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) v4[u] = e0 + u * ex.nt < ne ? rentry(e0 + u * ex.nt) : 0.;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = e0 + u * ex.nt;
        if (e >= ne) break;
        Rm[e] = v4[u];
#if defined(__HIP_DEVICE_COMPILE__)
        // the matrix-core GEMM takes each row's weight times its activation Hessian (w h)
        if (e % ldR == 0) {
          const int row = e / ldR;
          const CRec C{P + (int64_t)cg[4 * (int)cgi[row] + 2]};
          ch[row] *= C.weight();
        }
#endif
      }
    }
    // the rows of the impulse CoM costs, after the others and only on a knot that has one (the
    // branch is uniform); each entry on the lane that stored its placeholder above
    if (imp && has_impulse_com(b)) impulse_com_rows(lane, ex.nt, csrc, Jf, jw, Rm, ldR, nrows, nj, nc, Fx, da, Ld, H, Jc, ok);
#if defined(__HIP_DEVICE_COMPILE__)
    // the diagonal terms of the state / control costs (beyond the free-flyer block), per
    // column of [x tangent | u], in cost order
    for (int i = lane; i < L + m; i += ex.nt) {
      double d = 0.;
      for (int g = 0; g < ngr; ++g) {
        if ((int)cg[4 * g] >= 0) continue;
        const CRec C{P + (int64_t)cg[4 * g + 2]};
        if (cg[4 * g + 1] == 0. && i < L && !(b.ff && i < 6))
          d += C.weight() * cost_act(b, C, nu).hess(i, state_res(b, C.d(), x, i));
        else if (cg[4 * g + 1] == 1. && i >= L && i - L < nu)
          d += C.weight() * cost_act(b, C, nu).hess(i - L, u[i - L] - C.d()[i - L]);
      }
      cdg[i] = d;
    }
#endif
  });
  const double *const Rm_ = Rm, *const ch_ = ch, *const cg_ = cg, *const cam_ = cam, *const cav_ = cav, *const P_ = P,
                      *const x_ = x, *const u_ = u, *const cdg_ = cdg;
  // Gauss-Newton blocks (cost-sum.hxx:122-160) as a small GEMM over the rows, in
  // cost order: Lxx / Lxu / Luu entries four rows i at a time, then Lx / Lu.
  ex.run([&](int lane) {
    // the operands re-asserted as LDS where they are used (the inference does not carry
    // the entry's assumption this far: the loads were flat, each one a full round trip)
    const double* const Rm = ex.lds(Rm_);
    const double* const ch = ex.lds(ch_);
    const double* const cg = ex.lds(cg_);
    const double* const cam = ex.lds(cam_);
    const double* const cav = ex.lds(cav_);
    const double* const P = ex.lds(P_);
    const double* const x = ex.lds(x_);
    const double* const u = ex.lds(u_);
#if defined(__HIP_DEVICE_COMPILE__)
    gn_blocks_mfma(Rm, ldR, ch, nrows, L, nu, m, sc, Lxx, Lxu, Luu, cdg_);
    MB_GJ_MARK(26);
#else
    const int n4 = (n + 3) / 4, m4 = (m + 3) / 4;
    // Lxx is symmetric: only its row blocks i0 <= j are tasks (column j has j / 4 + 1 of
    // them; columns 4a .. 4a+3 follow 2a(a+1) tasks), each entry above the diagonal also
    // stored mirrored
    int tx = 0;
    for (int jj = 0; jj < n; ++jj) tx += jj / 4 + 1;
    const int txu = n4 * m, tuu = m4 * m;
    for (int task = lane; task < tx + txu + tuu; task += ex.nt) {
      int blk, i0, j;
      if (task < tx) {
        int a = (int)((sqrt(1. + 2. * task) - 1.) * 0.5);
        while (2 * (a + 1) * (a + 2) <= task) ++a;
        while (a > 0 && 2 * a * (a + 1) > task) --a;
        const int rem = task - 2 * a * (a + 1);
        blk = 0, j = 4 * a + rem / (a + 1), i0 = 4 * (rem % (a + 1));
      } else if (task < tx + txu) {
        blk = 1, i0 = 4 * ((task - tx) % n4), j = (task - tx) / n4;
      } else {
        blk = 2, i0 = 4 * ((task - tx - txu) % m4), j = (task - tx - txu) / m4;
      }
      // R columns of the rows (i) and of the column (j): x tangent or u (L + c)
      const int ci = blk == 2 ? L + i0 : i0;
      const int cj = blk == 0 ? j : L + j;
      const bool jin = blk == 0 || j < nu;
      double lv[4] = {0., 0., 0., 0.};
      for (int g = 0; g < ngr; ++g) {
        const int r0 = (int)cg[4 * g];
        const CRec C{P + (int64_t)cg[4 * g + 2]};
        if (r0 >= 0) {
          const int r1 = (int)cg[4 * g + 1];
          double s2[4] = {0., 0., 0., 0.};
          // rows in guarded batches of 4, loads first: a group (3-6 rows here) costs one
          // or two LDS round trips instead of one per row (the sums keep row order)
#pragma unroll 1
          for (int rb = r0; rb < r1; rb += 4) {
            double2 a01[4], a23[4];
            double hr[4], rj[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int r = rb + q < r1 ? rb + q : r0;
              const double* Rr = Rm + (int64_t)r * ldR;
              // rows are 16-B aligned (ldR even) and ci is a multiple of 4 (blk 2: L even)
              a01[q] = *reinterpret_cast<const double2*>(Rr + ci);
              a23[q] = *reinterpret_cast<const double2*>(Rr + ci + 2);
              hr[q] = ch[r];
              rj[q] = jin ? Rr[cj] : 0.;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (rb + q >= r1) break;
              s2[0] += a01[q].x * hr[q] * rj[q];
              s2[1] += a01[q].y * hr[q] * rj[q];
              s2[2] += a23[q].x * hr[q] * rj[q];
              s2[3] += a23[q].y * hr[q] * rj[q];
            }
          }
          const double wt = C.weight();
#pragma unroll
          for (int q = 0; q < 4; ++q) lv[q] += wt * s2[q];
        } else if ((cg[4 * g + 1] == 0.) == (blk == 0) && blk != 1) {  // state (Lxx) / control (Luu) diagonal
          const Act act = cost_act(b, C, nu);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            if (i != j) continue;
            if (blk == 0 && !(b.ff && j < 6)) lv[q] += C.weight() * act.hess(j, state_res(b, C.d(), x, j));
            if (blk == 2 && j < nu) lv[q] += C.weight() * act.hess(j, u[j] - C.d()[j]);
          }
        }
      }
      const int rows = blk == 2 ? m : n;
      double* out = blk == 0 ? Lxx : (blk == 1 ? Lxu : Luu);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q;
        if (i >= rows || (blk == 0 && i > j)) continue;
        const bool zero = (blk == 1 && j >= nu) || (blk == 2 && (i >= nu || j >= nu));
        const double v = zero ? 0. : (blk == 1 || integ ? sc * lv[q] : lv[q]);
        mb_gstore(out + (int64_t)j * rows + i, v);
        if (blk == 0 && i < j) mb_gstore(out + (int64_t)i * rows + j, v);
      }
    }
#endif
    // Lx (x columns) and Lu (u columns): R^T Ar in cost order
    for (int c = lane; c < n + m; c += ex.nt) {
      const bool isu = c >= n;
      const int j = isu ? c - n : c;
      double acc = 0.;
      if (!isu || j < nu) {
        const int cc = isu ? L + j : j;
        for (int g = 0; g < ngr; ++g) {
          const int r0 = (int)cg[4 * g];
          const CRec C{P + (int64_t)cg[4 * g + 2]};
          const double wt = C.weight();
          if (r0 >= 0) {
            const int r1 = (int)cg[4 * g + 1];
#pragma unroll 1
            for (int rb = r0; rb < r1; rb += 4) {  // guarded batches of 4 (as above)
              double rv[4], am[4], av[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int r = rb + q < r1 ? rb + q : r0;
                rv[q] = Rm[(int64_t)r * ldR + cc];
                am[q] = cam[r];
                av[q] = cav[r];
              }
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                if (rb + q >= r1) break;
                acc += wt * rv[q] * am[q] * av[q];
              }
            }
          } else if (!isu && cg[4 * g + 1] == 0. && !(b.ff && j < 6)) {
            acc += cost_act(b, C, nu).sgrad(j, state_res(b, C.d(), x, j), wt);
          } else if (isu && cg[4 * g + 1] == 1.) {
            acc += cost_act(b, C, nu).sgrad(j, u[j] - C.d()[j], wt);
          }
        }
      }
      mb_gstore((isu ? Lu : Lx) + j, integ ? sc * acc : acc);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    MB_GJ_MARK(27);
    assemble(lane, n);  // Fu
    MB_GJ_MARK(28);
#else
    (void)lane;
#endif
    // the fused calc's cost (cost-sum.hxx:89-117): record k's weighted activation on
    // lane spread_lane(k) (one record per wave first), into the dead pivot buffer
    // (pb[0, 64)); jac-cost residuals from the Jacobian phase.
    // The wide records (state / control, wide_cost) row-parallel instead: 32 lanes each
    // from lane 128 on (from lane 0 in a 128-thread workgroup), their partials into
    // pb[64 + 32 w + l], summed below.
    if (cost_out) {
      const double* cr = b.C;
      const int wbase = ex.nt >= 256 ? 128 : 0;
      int f = 0, nw = 0;
      for (int k = 0; k < b.ncost; ++k) {
        const CRec C{cr};
        const int t = C.type();
        const bool wide = wide_cost(C, nw);
        const int wl = lane - wbase - 32 * nw;  // this lane's share of wide record nw
        if (wide ? (wl >= 0 && wl < 32) : lane == spread_lane(k, ex.nt)) {
          const Act act = cost_act(b, C, nu);
          double a = 0.;
          if (jac_cost(b, t) && (!wide || wl == 0)) {
            const int nr = jac_rows(t);
            for (int i = 0; i < nr; ++i) a += act.value2(i, rf[6 * f + i]);
          }
          if (t == C_STATE) {
            for (int i = (b.ff ? 6 : 0) + (wide ? wl : 0); i < n; i += wide ? 32 : 1)
              a += act.value2(i, state_res(b, C.d(), x, i));
          } else if (t == C_CONTROL) {
            for (int i = wide ? wl : 0; i < nu; i += wide ? 32 : 1) a += act.value2(i, u[i] - C.d()[i]);
          } else if (force_cost(t)) {
            a = 2. * force_cost_activation(b, C, lam, nu);
          }
          if (wide)
            pb[64 + 32 * nw + wl] = a;
          else
            pb[k] = C.weight() * (0.5 * a);
        }
        f += jac_cost(b, t) ? 1 : 0;
        nw += wide ? 1 : 0;
        cr += C.size();
      }
    }
  });
  if (cost_out)  // summed in cost order
    ex.run([&](int lane) {
      if (lane != 0) return;
      double total = 0.;
      const double* cr = b.C;
      int nw = 0;
      for (int k = 0; k < b.ncost; ++k) {
        const CRec C{cr};
        if (wide_cost(C, nw)) {
          double a = 0.;
          for (int l = 0; l < 32; ++l) a += pb[64 + 32 * nw + l];
          total += C.weight() * (0.5 * a);
          ++nw;
        } else {
          total += pb[k];
        }
        cr += C.size();
      }
      *cost_out = integ ? dt * total : total;
    });
#if !defined(__HIP_DEVICE_COMPILE__)
  ex.run([&](int lane) { assemble(lane, 0); });  // Fx, Fu (after the residual rows: kSpillF)
#endif
  (void)nx;
}

template <int NT, int SP>
__device__ __forceinline__ void knot_calc_diff(const double* P, int nx, int m, const double* xg, const double* ug, bool use_u,
                                      double* w, double* Fx, double* Fu, double* Lxx, double* Lxu, double* Luu,
                                      double* Lx, double* Lu, double* xnext_out, double* cost_out,
                                      const double* xu_pre = nullptr, int spill = 0) {
  static_assert(NT >= 128 && NT % 64 == 0, "the calcDiff phases take >= 2 waves");
  knot_calc_diff_x<DevExec, SP>(DevExec{NT}, P, nx, m, xg, ug, use_u, w, Fx, Fu, Lxx, Lxu, Luu, Lx, Lu, xnext_out,
                                cost_out, xu_pre, spill);
}

}  // namespace mb
}  // namespace fddp
