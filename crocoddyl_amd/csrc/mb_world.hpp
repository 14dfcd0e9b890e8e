// Multibody knots, world-frame values (WVals) and the RNEA / CRBA recursions as ancestor and
// subtree sums, with their per-wave partial sums.
#pragma once

#include "mb_spatial.hpp"

namespace fddp {
namespace mb {

// ---------------------------------------------------------------------------
// World-frame values. Spatial quantities are expressed at the world origin in
// world axes, so every recursion of RNEA/CRBA becomes a sum over the ancestors or
// the subtree of a dof
//   v_i = sum_{k in anc(i)} S_k qd_k,  a_i = -g + sum_{k in anc(i)} (S_k qdd_k + v_k x S_k qd_k),
//   tau_i = S_i . sum_{k in sub(i)} f_k,  Ic_i = sum_{k in sub(i)} I_k,
//   M_ij = S_i . (Ic_j S_j)  (i in anc(j)),
// which each lane evaluates for its own dof: no serial chain through LDS.
// anc(i) holds every dof of the ancestor-or-self bodies (all six free-flyer
// dofs for the base), so v_k is the full body velocity. The placements
// oMi = oMparent * liMi are composed by each lane walking its ancestors (w_walk).
// ---------------------------------------------------------------------------
// The world values of a dof in two records of kWRec doubles (40 used, 2 of padding): the
// L record holds what outlives the recursions (placement oMi, motion subspace, velocity,
// acceleration, composite inertia), the D record what the recursions alone use (the local
// placement, body mass / CoM / inertia, the RNEA's forces and terms). The workgroup's lanes
// read and write their own dof's records (lane stride kWRec): at a multiple of 32 doubles
// every lane of a 64-bit access would map to the same bank pair; at 42 (84 dwords) the lanes
// spread over 16 bank pairs (2-way) with the records 16-byte aligned. (One 80-double record
// per dof, its round-5 layout, was a 16-way conflict: C5 rollout 28.55 -> 26.81 ms,
// calcDiff 25.60 -> 25.26 ms when padded.) The D records may lie apart from the L records
// (`aux`): the rollout's calc puts its factorisation over them once the recursions are done
// (knot_calc_dense_x); by default they follow the L records, the ancestor masks and root_a.
constexpr int kWRec = 42;
constexpr int kMaxCosts = 64;
struct WVals {
  double* base;
  int nj;
  double* parts;  // per-wave partial sums of the recursions: 4 x 6 per dof (kPartDoubles)
  double* aux;    // the D records
  MB_HD WVals(double* b, int n, double* p, double* a = nullptr)
      : base(b), nj(n), parts(p), aux(a ? a : b + lsize(n)) {}
  MB_HD double* L(int i) const { return mb_lds(base + kWRec * i); }
  MB_HD double* Dr(int i) const { return mb_lds(aux + kWRec * i); }
  MB_HD double* oR(int i) const { return L(i); }  // oMi
  MB_HD double* op(int i) const { return L(i) + 9; }
  MB_HD double* S(int i) const { return L(i) + 12; }   // dof motion subspace (world)
  MB_HD double* v(int i) const { return L(i) + 18; }
  MB_HD double* a(int i) const { return L(i) + 24; }
  MB_HD double* cm(int i) const { return L(i) + 30; }  // composite inertia, origin form: m, h = m c, I_O (6)
  MB_HD double* ch(int i) const { return L(i) + 31; }
  MB_HD double* cI(int i) const { return L(i) + 34; }
  MB_HD double* R(int i) const { return Dr(i); }  // liMi rotation
  MB_HD double* p(int i) const { return Dr(i) + 9; }
  MB_HD double* m(int i) const { return Dr(i) + 12; }   // body mass (0 on the massless free-flyer dofs)
  MB_HD double* c(int i) const { return Dr(i) + 13; }   // body CoM (world)
  MB_HD double* Ic(int i) const { return Dr(i) + 16; }  // body inertia about its CoM, world axes (6)
  MB_HD double* F(int i) const { return Dr(i) + 22; }   // body force, then accumulated joint force
  MB_HD double* cq(int i) const { return Dr(i) + 28; }  // S_i qdd_i + v_i x S_i qd_i
  MB_HD double* fb(int i) const { return Dr(i) + 34; }  // body force I a + v x* I v
  // per-wave partial sums of the ancestor / subtree recursions (wave w's share of the dofs)
  MB_HD double* part(int w, int i) const { return mb_lds(parts + 6 * ((int64_t)w * nj + i)); }
  MB_HD Mask* anc(int i) const { return (Mask*)(base + kWRec * nj) + i; }  // ancestors-or-self dofs
  MB_HD double* root_a() const { return mb_lds(base + kWRec * nj + nj); }
  // the L records, the masks and root_a; the D records
  MB_HD static int64_t lsize(int nj) { return pad2((int64_t)kWRec * nj + nj + 6); }
  MB_HD static int64_t dsize(int nj) { return (int64_t)kWRec * nj; }
  MB_HD static int64_t doubles(int nj) { return lsize(nj) + dsize(nj); }
};

// The per-wave partial sums (RNEA recursions: 6 per dof, composites: 10 per dof) come
// from at most kPartWaves waves (their LDS areas are sized for that); larger workgroups
// leave the other waves idle in those phases.
constexpr int kPartWaves = 4;
MB_HD __forceinline__ int part_waves(int nt) { return (nt >> 6) < kPartWaves ? (nt >> 6) : kPartWaves; }
// (6 per dof for the RNEA sums, 10 for the composites)
MB_HD __forceinline__ int64_t part_doubles(int nj) { return (int64_t)kPartWaves * 10 * nj; }

// lane i < nj: local placement (buffer A starts as liMi), ancestor bits.
MB_HD inline void w_joint_local(const Blk& b, const WVals& W, const double* q, int i) {
  double R[9], p[3];
  if (b.ff && i < 6) {
    if (i == 0) {  // base pose: root placement * (R(quat), p)
      const JRec J(b, 0);
      double Rq[9], t[3];
      quat_to_R(q + 3, Rq);
      matmul3(J.Rpl(), Rq, R);
      matvec3(J.Rpl(), q, t);
      for (int e = 0; e < 3; ++e) p[e] = J.ppl()[e] + t[e];
    } else {
      for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0) ? 1. : 0.;
      for (int e = 0; e < 3; ++e) p[e] = 0.;
    }
  } else {
    const JRec J(b, rec_of(b, i));
    double ax[3], Rpl[9];
    for (int e = 0; e < 3; ++e) ax[e] = J.axis()[e];
    for (int e = 0; e < 9; ++e) Rpl[e] = J.Rpl()[e];
#if MB_PRISMATIC
    if (dof_prismatic(b, i)) {  // liMi = (Rpl, ppl + Rpl axis q)
      double t[3];
      matvec3(Rpl, ax, t);
      const double qi = q[qof(b, i)];
      for (int e = 0; e < 9; ++e) R[e] = Rpl[e];
      for (int e = 0; e < 3; ++e) p[e] = J.ppl()[e] + t[e] * qi;
    } else
#endif
    {
      joint_rotation(Rpl, ax, q[qof(b, i)], R);
      for (int e = 0; e < 3; ++e) p[e] = J.ppl()[e];
    }
  }
  for (int e = 0; e < 9; ++e) {
    W.R(i)[e] = R[e];
    W.oR(i)[e] = R[e];
  }
  for (int e = 0; e < 3; ++e) {
    W.p(i)[e] = p[e];
    W.op(i)[e] = p[e];
  }
  if (i == 0) {
    for (int e = 0; e < 6; ++e) W.root_a()[e] = e < 3 ? -b.g[e] : 0.;
  }
  *W.anc(i) = anc_mask(b, i);
}

// lane i < nj: oMi = L_root ... L_i, the local placements of i's ancestors composed
// by walking its ancestor mask from i towards the root (parents precede children):
// one phase, no barrier per level, and the loads do not wait on the products (the
// pointer-jumping rounds this replaced took ceil(log2 nj) barrier phases). The free-flyer's
// dofs 1..5 carry identity placements and are skipped (exact).
MB_HD inline void w_walk(const Blk& b, const WVals& W, int i) {
  double R[9], p[3];
  for (int e = 0; e < 9; ++e) R[e] = W.R(i)[e];
  for (int e = 0; e < 3; ++e) p[e] = W.p(i)[e];
  Mask m = *W.anc(i) & ~(1ull << i);
  if (b.ff) m &= ~0x3Eull;
  while (m) {
    const int k = 63 - __builtin_clzll(m);
    m &= ~(1ull << k);
    double Rk[9], pk[3], Rn[9], t[3];
    for (int e = 0; e < 9; ++e) Rk[e] = W.R(k)[e];
    for (int e = 0; e < 3; ++e) pk[e] = W.p(k)[e];
    matmul3(Rk, R, Rn);
    matvec3(Rk, p, t);
    for (int e = 0; e < 9; ++e) R[e] = Rn[e];
    for (int e = 0; e < 3; ++e) p[e] = pk[e] + t[e];
  }
  for (int e = 0; e < 9; ++e) W.oR(i)[e] = R[e];
  for (int e = 0; e < 3; ++e) W.op(i)[e] = p[e];
}

// lane i < nj: world motion subspace and body inertia from oMi (oR/op).
MB_HD inline void w_joint_world(const Blk& b, const WVals& W, int i) {
  double oR[9], op[3], w[3], ax[3];
  for (int e = 0; e < 9; ++e) oR[e] = W.oR(i)[e];
  for (int e = 0; e < 3; ++e) op[e] = W.op(i)[e];
  dof_axis(b, i, ax);
  matvec3(oR, ax, w);
  if (dof_prismatic(b, i)) {
    for (int e = 0; e < 3; ++e) {
      W.S(i)[e] = w[e];
      W.S(i)[3 + e] = 0.;
    }
  } else {
    double vl[3];
    cross3(op, w, vl);  // velocity of the world origin: w x (0 - op) = op x w
    for (int e = 0; e < 3; ++e) {
      W.S(i)[e] = vl[e];
      W.S(i)[3 + e] = w[e];
    }
  }
  double* o = W.Ic(i);
  if (!carries_body(b, i)) {
    *W.m(i) = 0.;
    for (int e = 0; e < 3; ++e) W.c(i)[e] = op[e];
    for (int e = 0; e < 6; ++e) o[e] = 0.;
    return;
  }
  const JRec J(b, rec_of(b, i));
  double c[3], t[3];
  matvec3(oR, J.com(), t);
  for (int e = 0; e < 3; ++e) c[e] = op[e] + t[e];
  // Ic_w = oR Ic oR^T
  const double* s = J.I6();
  const double Is[9] = {s[0], s[3], s[4], s[3], s[1], s[5], s[4], s[5], s[2]};
  double tmp[9], Iw[9];
  matmul3(oR, Is, tmp);
  for (int r = 0; r < 3; ++r)
    for (int cc = 0; cc < 3; ++cc) Iw[cc * 3 + r] = tmp[r] * oR[cc] + tmp[3 + r] * oR[3 + cc] + tmp[6 + r] * oR[6 + cc];
  for (int e = 0; e < 3; ++e) W.c(i)[e] = c[e];
  *W.m(i) = J.mass();
  o[0] = Iw[0];
  o[1] = Iw[4];
  o[2] = Iw[8];
  o[3] = Iw[3];
  o[4] = Iw[6];
  o[5] = Iw[7];
}

// wave w's contiguous share [w c, (w + 1) c), c = ceil(nj / nw), of nj dofs
MB_HD __forceinline__ void k_range(int nj, int w, int nw, int& k0, int& k1) {
  const int c = (nj + nw - 1) / nw;
  k0 = w * c;
  k1 = k0 + c < nj ? k0 + c : nj;
}
// Per-record work on one lane each, from the top of the workgroup down: record k on
// lane nt - 1 - 64 (k mod W) - k / W (W waves), i.e. one record per wave before any wave
// takes a second (a wave runs its divergent lanes' paths one after another).
MB_HD __forceinline__ int spread_lane(int k, int nt) {
  const int nwv = nt >> 6;
  return nt - 1 - 64 * (k % nwv) - k / nwv;
}
MB_HD __forceinline__ int spread_item(int lane, int nt) {
  const int u = nt - 1 - lane, nwv = nt >> 6;
  return (u & 63) * nwv + (u >> 6);
}
// composite inertia of dof i's subtree times a motion x: (m v - h x w, I_O w + h x v)
MB_HD __forceinline__ void comp_mul(const WVals& W, int i, const double* x, double* o) {
  const double m = *W.cm(i);
  const double* h = W.ch(i);
  const double* I = W.cI(i);
  double t[3];
  cross3(h, x + 3, t);
  for (int e = 0; e < 3; ++e) o[e] = m * x[e] - t[e];
  cross3(h, x, t);
  o[3] = I[0] * x[3] + I[3] * x[4] + I[4] * x[5] + t[0];
  o[4] = I[3] * x[3] + I[1] * x[4] + I[5] * x[5] + t[1];
  o[5] = I[4] * x[3] + I[5] * x[4] + I[2] * x[5] + t[2];
}

// lane i < nj: v_i = sum over ancestors-or-self of S_k qd_k
MB_HD inline void w_velocity(const WVals& W, const double* qd, int i) {
  double v[6] = {0., 0., 0., 0., 0., 0.};
  const Mask am = *W.anc(i);
  // every dof's terms loaded, the others' selected away (not branched around), so the
  // unrolled iterations' LDS loads overlap; the sums keep their order
#pragma unroll 2
  for (int k = 0; k < W.nj; ++k) {
    const bool in = (am >> k) & 1ull;
    const double w = qd[k];
    for (int e = 0; e < 6; ++e) {
      const double t = W.S(k)[e] * w;
      v[e] += in ? t : 0.;
    }
  }
  for (int e = 0; e < 6; ++e) W.v(i)[e] = v[e];
}

// lane i < nj: cq_i = S_i qdd_i + v_i x (S_i qd_i)
MB_HD inline void w_accel_term(const WVals& W, const double* qd, const double* qdd, int i) {
  double S[6], v[6], Sw[6], t6[6];
  const double w = qd[i], qa = qdd ? qdd[i] : 0.;
  for (int e = 0; e < 6; ++e) {
    S[e] = W.S(i)[e];
    v[e] = W.v(i)[e];
    Sw[e] = S[e] * w;
  }
  cross_m(v, Sw, t6);
  for (int e = 0; e < 6; ++e) W.cq(i)[e] = S[e] * qa + t6[e];
}

// lane i < nj: a_i = -g + sum over ancestors-or-self of cq_k, then the body
// force f_i = I_i a_i + v_i x* (I_i v_i) - fext_i
MB_HD inline void w_accel_force(const WVals& W, int i, const double* fx = nullptr) {
  double a[6];
  for (int e = 0; e < 6; ++e) a[e] = W.root_a()[e];
  const Mask am = *W.anc(i);
#pragma unroll 2
  for (int k = 0; k < W.nj; ++k) {  // (selected, not branched: as w_velocity)
    const bool in = (am >> k) & 1ull;
    for (int e = 0; e < 6; ++e) {
      const double t = W.cq(k)[e];
      a[e] += in ? t : 0.;
    }
  }
  double v[6], f[6], Iv[6], t6[6], c[3], I6[6];
  for (int e = 0; e < 6; ++e) {
    W.a(i)[e] = a[e];
    v[e] = W.v(i)[e];
    I6[e] = W.Ic(i)[e];
  }
  for (int e = 0; e < 3; ++e) c[e] = W.c(i)[e];
  const double m = *W.m(i);
  inertia_mul(m, c, I6, a, f);
  inertia_mul(m, c, I6, v, Iv);
  cross_f(v, Iv, t6);
  for (int e = 0; e < 6; ++e) W.fb(i)[e] = f[e] + t6[e] - (fx ? fx[6 * i + e] : 0.);
}

// lane i < nj: F_i = sum over the subtree of the body forces, tau_i = S_i . F_i
MB_HD inline void w_joint_force(const Blk& b, const WVals& W, double* tau, int i) {
  double F[6] = {0., 0., 0., 0., 0., 0.};
#pragma unroll 2
  for (int k = 0; k < b.nj; ++k) {  // (selected, not branched: as w_velocity)
    const bool in = (*W.anc(k) >> i) & 1ull;
    for (int e = 0; e < 6; ++e) {
      const double t = W.fb(k)[e];
      F[e] += in ? t : 0.;
    }
  }
  for (int e = 0; e < 6; ++e) W.F(i)[e] = F[e];
  tau[i] = dot6(W.S(i), F);
}

// lane j < nj of wave w (of nw): CRBA column j in world frame, F = Ic_j S_j, M_ij = S_i . F
// for the ancestors-or-self i < j of j (+ armature on the diagonal), the rows i < j split
// in nw contiguous ranges, one per wave (the waves run side by side: the per-lane chain
// of LDS loads is a quarter as long). A: ld lda, zeroed.
// The column is formed about the point P = joint j's origin, not the world origin: the
// subtree's composite inertia is summed from the bodies' offsets c_b - P, and the motion
// subspaces are shifted to P (S_i at P: [w_i x (P - p_i); w_i], a prismatic dof [w_i; 0]).
// About the world origin the entries of a light distal link (a gripper, 1e-4 kg m^2, 1 m
// from the origin) are the difference of terms ~ m |c|^2 ~ 0.3, which cost ~3 digits of
// M and, through cond(M) ~ 1e6, of M^-1 and Fu (the round-4 parity trace); at P the
// lever arms are the link's own size.
// Phase 1 (lane j of wave w < nw): wave w's share of j's subtree bodies into its
// partial (W.parts, 10 per dof: m, h, I about P_j), as w_composite.
MB_HD inline void w_crba_composite_part(const Blk& b, const WVals& W, int j, int w, int nw) {
  double P[3], m = 0., h[3] = {0., 0., 0.}, I[6] = {0., 0., 0., 0., 0., 0.};
  for (int e = 0; e < 3; ++e) P[e] = W.op(j)[e];
  int k0 = b.ff ? 5 : 0, k1 = b.nj;
  if (nw > 1) k_range(b.nj, w, nw, k0, k1);
  if (b.ff && k0 < 5) k0 = 5;
  // (every body of the share read, the others weighted 0: the loads overlap)
#pragma unroll 2
  for (int k = k0; k < k1; ++k) {
    const double sel = ((*W.anc(k) >> j) & 1ull) ? 1. : 0.;
    const double mk = *W.m(k);
    double c[3], Ic[6];
    for (int e = 0; e < 3; ++e) c[e] = W.c(k)[e] - P[e];
    for (int e = 0; e < 6; ++e) Ic[e] = W.Ic(k)[e];
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    m += sel * mk;
    for (int e = 0; e < 3; ++e) h[e] += sel * (mk * c[e]);
    I[0] += sel * (Ic[0] + mk * (cc - c[0] * c[0]));
    I[1] += sel * (Ic[1] + mk * (cc - c[1] * c[1]));
    I[2] += sel * (Ic[2] + mk * (cc - c[2] * c[2]));
    I[3] += sel * (Ic[3] - mk * c[0] * c[1]);
    I[4] += sel * (Ic[4] - mk * c[0] * c[2]);
    I[5] += sel * (Ic[5] - mk * c[1] * c[2]);
  }
  double* o = mb_lds(W.parts + 10 * ((int64_t)w * b.nj + j));
  o[0] = m;
  for (int e = 0; e < 3; ++e) o[1 + e] = h[e];
  for (int e = 0; e < 6; ++e) o[4 + e] = I[e];
}
// Phase 2 (lane j of wave w of nw): the partials of the npw waves combined in wave order,
// F = Ic_j S_j about P_j, M_ij = S_i(P_j) . F for the ancestors-or-self i < j of j (+
// armature on the diagonal), the rows i < j split in nw contiguous ranges, one per wave.
// A: ld lda, zeroed.
// store_world: wave 0 also stores the subtree composite about the world origin (W.cm /
// ch / cI, the calcDiff's recursions): h_O = h + m P, I_O = I + 2 (h.P) 1 - (h P^T +
// P h^T) + m (|P|^2 1 - P P^T) (the same terms as summing the bodies about the origin).
// (the partials of the npw waves combined in wave order)
MB_HD __forceinline__ void w_crba_combine(const WVals& W, int nj, int j, int npw, double* v) {
  const double* p0 = mb_lds(W.parts + 10 * (int64_t)j);
  for (int e = 0; e < 10; ++e) v[e] = p0[e];
  for (int ww = 1; ww < npw; ++ww) {
    const double* p = mb_lds(W.parts + 10 * ((int64_t)ww * nj + j));
    for (int e = 0; e < 10; ++e) v[e] += p[e];
  }
}
// combined: the composite about P_j already in W.cm / ch / cI (w_crba_store_local; the
// partials may be overwritten meanwhile)
MB_HD inline void w_crba_column(const Blk& b, const WVals& W, int j, double* A, int lda, int w, int nw, int npw,
                                bool store_world = false, bool combined = false) {
  double P[3], v[10];
  for (int e = 0; e < 3; ++e) P[e] = W.op(j)[e];
  if (combined) {
    v[0] = *W.cm(j);
    for (int e = 0; e < 3; ++e) v[1 + e] = W.ch(j)[e];
    for (int e = 0; e < 6; ++e) v[4 + e] = W.cI(j)[e];
  } else {
    w_crba_combine(W, b.nj, j, npw, v);
  }
  const double m = v[0];
  const double* h = v + 1;
  const double* I = v + 4;
  if (store_world && w == 0) {
    const double hp = h[0] * P[0] + h[1] * P[1] + h[2] * P[2], pp = P[0] * P[0] + P[1] * P[1] + P[2] * P[2];
    *W.cm(j) = m;
    for (int e = 0; e < 3; ++e) W.ch(j)[e] = h[e] + m * P[e];
    // (I ordering: xx, yy, zz, xy, xz, yz)
    W.cI(j)[0] = I[0] + 2. * (hp - h[0] * P[0]) + m * (pp - P[0] * P[0]);
    W.cI(j)[1] = I[1] + 2. * (hp - h[1] * P[1]) + m * (pp - P[1] * P[1]);
    W.cI(j)[2] = I[2] + 2. * (hp - h[2] * P[2]) + m * (pp - P[2] * P[2]);
    W.cI(j)[3] = I[3] - (h[0] * P[1] + P[0] * h[1]) - m * P[0] * P[1];
    W.cI(j)[4] = I[4] - (h[0] * P[2] + P[0] * h[2]) - m * P[0] * P[2];
    W.cI(j)[5] = I[5] - (h[1] * P[2] + P[1] * h[2]) - m * P[1] * P[2];
  }
  // S_i shifted to P: [S_i.lin + S_i.ang x P; S_i.ang] (a revolute dof's axis w through
  // p_i moves P at w x (P - p_i) = S_i.lin + w x P; a prismatic dof has S_i.ang = 0).
  // The products are dimension-one in the lever arms, so forming them from the world-origin
  // S_i costs only the rounding of the placements (unlike the quadratic m |c|^2 terms).
  // Scalars throughout: a shifted-S array written under a branch lands in scratch memory.
  const double* Sjw = W.S(j);
  const double sj3 = Sjw[3], sj4 = Sjw[4], sj5 = Sjw[5];
  const double sj0 = Sjw[0] + (sj4 * P[2] - sj5 * P[1]);
  const double sj1 = Sjw[1] + (sj5 * P[0] - sj3 * P[2]);
  const double sj2 = Sjw[2] + (sj3 * P[1] - sj4 * P[0]);
  // F = Ic_j S_j about P: (m v - h x w, I w + h x v)
  const double F0 = m * sj0 - (h[1] * sj5 - h[2] * sj4);
  const double F1 = m * sj1 - (h[2] * sj3 - h[0] * sj5);
  const double F2 = m * sj2 - (h[0] * sj4 - h[1] * sj3);
  const double F3 = I[0] * sj3 + I[3] * sj4 + I[4] * sj5 + (h[1] * sj2 - h[2] * sj1);
  const double F4 = I[3] * sj3 + I[1] * sj4 + I[5] * sj5 + (h[2] * sj0 - h[0] * sj2);
  const double F5 = I[4] * sj3 + I[5] * sj4 + I[2] * sj5 + (h[0] * sj1 - h[1] * sj0);
  if (w == 0) A[(int64_t)j * lda + j] = (sj0 * F0 + sj1 * F1 + sj2 * F2) + (sj3 * F3 + sj4 * F4 + sj5 * F5) + b.arm[j];
  const Mask am = *W.anc(j);
  const int ch = (j + nw - 1) / nw, i0 = w * ch, i1 = i0 + ch < j ? i0 + ch : j;
  // every i < j visited, the non-ancestors storing their zero (only lane j writes the
  // pair {i, j}), so the loop has no branch and the unrolled loads overlap
#pragma unroll 2
  for (int i = i0; i < i1; ++i) {
    const double* Si = W.S(i);
    const double a3 = Si[3], a4 = Si[4], a5 = Si[5];
    const double l0 = Si[0] + (a4 * P[2] - a5 * P[1]);
    const double l1 = Si[1] + (a5 * P[0] - a3 * P[2]);
    const double l2 = Si[2] + (a3 * P[1] - a4 * P[0]);
    const double d = (l0 * F0 + l1 * F1 + l2 * F2) + (a3 * F3 + a4 * F4 + a5 * F5);
    const double Mij = ((am >> i) & 1ull) ? d : 0.;
    A[(int64_t)j * lda + i] = Mij;
    A[(int64_t)i * lda + j] = Mij;
  }
}

// lane j: the subtree composite about P_j (the combined partials) into W.cm / ch / cI, so
// that the columns can overwrite the partials (the rollout's calc, knot_calc_dense_x)
MB_HD inline void w_crba_store_local(const WVals& W, int nj, int j, int npw) {
  double v[10];
  w_crba_combine(W, nj, j, npw, v);
  *W.cm(j) = v[0];
  for (int e = 0; e < 3; ++e) W.ch(j)[e] = v[1 + e];
  for (int e = 0; e < 6; ++e) W.cI(j)[e] = v[4 + e];
}

// ---- the RNEA recursions split over the waves ---------------------------------
// Each ancestor (or subtree) sum of lane i runs over the dofs k in wave w's contiguous
// range [w c, (w + 1) c), c = ceil(nj / nw), into part(w, i); the next phase combines
// the nw partials in wave order. (The sums' association changes, not their terms.)
MB_HD __forceinline__ void combine6(const WVals& W, int i, int nw, double* o) {
  for (int e = 0; e < 6; ++e) o[e] = W.part(0, i)[e];
  for (int w = 1; w < nw; ++w)
    for (int e = 0; e < 6; ++e) o[e] += W.part(w, i)[e];
}
// lane i, wave w: sum over ancestors-or-self k in w's range of S_k qd_k
MB_HD inline void w_velocity_part(const WVals& W, const double* qd, int i, int w, int nw) {
  double v[6] = {0., 0., 0., 0., 0., 0.};
  const Mask am = *W.anc(i);
  int k0, k1;
  k_range(W.nj, w, nw, k0, k1);
#pragma unroll 2
  for (int k = k0; k < k1; ++k) {
    const bool in = (am >> k) & 1ull;
    const double qk = qd[k];
    for (int e = 0; e < 6; ++e) {
      const double t = W.S(k)[e] * qk;
      v[e] += in ? t : 0.;
    }
  }
  for (int e = 0; e < 6; ++e) W.part(w, i)[e] = v[e];
}
// lane i, wave w: sum over ancestors-or-self k in w's range of cq_k
MB_HD inline void w_accel_part(const WVals& W, int i, int w, int nw) {
  double a[6] = {0., 0., 0., 0., 0., 0.};
  const Mask am = *W.anc(i);
  int k0, k1;
  k_range(W.nj, w, nw, k0, k1);
#pragma unroll 2
  for (int k = k0; k < k1; ++k) {
    const bool in = (am >> k) & 1ull;
    for (int e = 0; e < 6; ++e) {
      const double t = W.cq(k)[e];
      a[e] += in ? t : 0.;
    }
  }
  for (int e = 0; e < 6; ++e) W.part(w, i)[e] = a[e];
}
// lane i, wave w: sum over the subtree bodies k in w's range of the body forces
MB_HD inline void w_force_part(const WVals& W, int i, int w, int nw) {
  double F[6] = {0., 0., 0., 0., 0., 0.};
  int k0, k1;
  k_range(W.nj, w, nw, k0, k1);
#pragma unroll 2
  for (int k = k0; k < k1; ++k) {
    const bool in = (*W.anc(k) >> i) & 1ull;
    for (int e = 0; e < 6; ++e) {
      const double t = W.fb(k)[e];
      F[e] += in ? t : 0.;
    }
  }
  for (int e = 0; e < 6; ++e) W.part(w, i)[e] = F[e];
}
// lane i: v_i from the partials, then cq_i = S_i qdd_i + v_i x (S_i qd_i)
MB_HD inline void w_velocity_accel_term(const WVals& W, const double* qd, const double* qdd, int i, int nw) {
  double v[6];
  combine6(W, i, nw, v);
  for (int e = 0; e < 6; ++e) W.v(i)[e] = v[e];
  double S[6], Sw[6], t6[6];
  const double wq = qd[i], qa = qdd ? qdd[i] : 0.;
  for (int e = 0; e < 6; ++e) {
    S[e] = W.S(i)[e];
    Sw[e] = S[e] * wq;
  }
  cross_m(v, Sw, t6);
  for (int e = 0; e < 6; ++e) W.cq(i)[e] = S[e] * qa + t6[e];
}
// lane i: a_i = -g + the partials, then the body force f_i = I_i a_i + v_i x* (I_i v_i) - fext_i
MB_HD inline void w_accel_body_force(const WVals& W, int i, int nw, const double* fx) {
  double a[6], p[6];
  combine6(W, i, nw, p);
  for (int e = 0; e < 6; ++e) a[e] = W.root_a()[e] + p[e];
  double v[6], f[6], Iv[6], t6[6], c[3], I6[6];
  for (int e = 0; e < 6; ++e) {
    W.a(i)[e] = a[e];
    v[e] = W.v(i)[e];
    I6[e] = W.Ic(i)[e];
  }
  for (int e = 0; e < 3; ++e) c[e] = W.c(i)[e];
  const double m = *W.m(i);
  inertia_mul(m, c, I6, a, f);
  inertia_mul(m, c, I6, v, Iv);
  cross_f(v, Iv, t6);
  for (int e = 0; e < 6; ++e) W.fb(i)[e] = f[e] + t6[e] - (fx ? fx[6 * i + e] : 0.);
}
// lane i: F_i from the partials, tau_i = S_i . F_i
MB_HD inline void w_joint_force_comb(const WVals& W, double* tau, int i, int nw) {
  double F[6];
  combine6(W, i, nw, F);
  for (int e = 0; e < 6; ++e) W.F(i)[e] = F[e];
  tau[i] = dot6(W.S(i), F);
}

}  // namespace mb
}  // namespace fddp
