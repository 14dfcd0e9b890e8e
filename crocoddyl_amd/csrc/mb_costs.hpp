// Multibody knots, cost and contact records: CRec, the activations (Act), residuals and
// their Jacobians, the cost counts that size the calcDiff's plan, the contact rows.
#pragma once

#include "mb_se3.hpp"
#include "mb_world.hpp"

namespace fddp {
namespace mb {

// Cost records
struct CRec {
  const double* r;
  MB_HD int type() const { return (int)mb_lds(r)[0]; }
  MB_HD double weight() const { return mb_lds(r)[1]; }
  MB_HD int size() const { return (int)mb_lds(r)[3]; }
  MB_HD const double* d() const { return mb_lds(r + kCHdr); }
};

// dof carrying the frame of a frame / contact payload d = [joint record, R 9, p 3, ...]
MB_HD __forceinline__ int frame_dof(const Blk& b, const double* d) { return dof_of_rec(b, (int)d[0]); }

// oMf of a frame payload
MB_HD inline void frame_placement(const Blk& b, const WVals& V, const double* d, double* R, double* p) {
  const int j = frame_dof(b, d);
  matmul3(V.oR(j), d + 1, R);
  matvec3(V.oR(j), d + 10, p);
  p[0] += V.op(j)[0];
  p[1] += V.op(j)[1];
  p[2] += V.op(j)[2];
}

// Residual of a frame cost and, with S != null (the world motion of a dof that
// moves the frame), its Jacobian column. Returns the residual size (6 placement,
// 3 translation, 3 rotation: log3(Rref^T oRf), the angular half of log6 with no
// translation, so that Jc is Jlog3(r) times the frame's LOCAL angular Jacobian column).
MB_HD inline int frame_residual(const Blk& b, const WVals& V, const CRec& C, const double* S, double* r, double* Jc) {
  const double* d = C.d();
  double Rf[9], pf[3];
  frame_placement(b, V, d, Rf, pf);
  double dR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.}, dp[3] = {0., 0., 0.};
  if (S) {  // motion of oMf under S: dp = S_lin + S_ang x pf, dR = [S_ang]x Rf
    double t[3];
    cross3(S + 3, pf, t);
    for (int e = 0; e < 3; ++e) dp[e] = S[e] + t[e];
    for (int c = 0; c < 3; ++c) cross3(S + 3, Rf + 3 * c, dR + 3 * c);
  }
  if (C.type() == C_FRAME_TRANSLATION || C.type() == C_CONTACT_3D) {
    const double* pref = d + 13;
    for (int e = 0; e < 3; ++e) {
      r[e] = pf[e] - pref[e];
      if (Jc) Jc[e] = dp[e];
    }
    for (int e = 3; e < 6; ++e) {
      r[e] = 0.;
      if (Jc) Jc[e] = 0.;
    }
    return 3;
  }
  // rMf = Mref^-1 oMf
  // a rotation cost: the same log6 on (Rref^T oRf, 0), whose linear half is zero and whose
  // angular half is log3 (one instance of log6_t in the kernel); its record has no
  // translation slot, so pr, unused then, adds three elements of Rref^T instead
  const bool rot = C.type() == C_FRAME_ROTATION;
  const double* Rri = d + 13;
  const double* pri = rot ? d + 13 : d + 22;
  double Rr[9], pr[3], dRr[9], dpr[3];
  matmul3(Rri, Rf, Rr);
  matvec3(Rri, pf, pr);
  pr[0] += pri[0];
  pr[1] += pri[1];
  pr[2] += pri[2];
  matmul3(Rri, dR, dRr);
  matvec3(Rri, dp, dpr);
  Dual RD[9], PD[3], o[6];
  for (int e = 0; e < 9; ++e) RD[e] = Dual{Rr[e], dRr[e]};
  for (int e = 0; e < 3; ++e) PD[e] = rot ? Dual{0., 0.} : Dual{pr[e], dpr[e]};
  log6_t<Dual>(RD, PD, o);
  for (int e = 0; e < 3; ++e) {
    const Dual lo = rot ? o[3 + e] : o[e], hi = rot ? Dual{0., 0.} : o[3 + e];
    r[e] = lo.v;
    r[3 + e] = hi.v;
    if (Jc) Jc[e] = S ? lo.d : 0.;
    if (Jc) Jc[3 + e] = S ? hi.d : 0.;
  }
  return rot ? 3 : 6;
}

// Residual size of a cost record.
MB_HD inline int cost_nr(const Blk& b, const CRec& C, int nu) {
  const int t = C.type();
  if (t == C_CONTACT_FORCE) return (int)C.d()[1];
  if (t == C_FRICTION_CONE || t == C_COP_POSITION) return (int)C.d()[2];
  if (t == C_STATE) return 2 * b.nj;
  if (t == C_CONTROL) return nu;
  return (t == C_FRAME_PLACEMENT || t == C_FRAME_VELOCITY || t == C_CENTROIDAL_MOMENTUM) ? 6 : 3;
}
// The activation of a cost record (its parameters end the record):
//   Quad / WeightedQuad (quadratic.hpp, weighted-quadratic.hpp:42-71): w (ones if
//     unweighted); a = 0.5 w r^2, Ar = w r, Arr = w
//   QuadraticBarrier (quadratic-barrier.hpp:88-117): lb, ub; with rl = min(r - lb, 0),
//     ru = max(r - ub, 0): a = 0.5 (rl^2 + ru^2), Ar = rl + ru, Arr = [r <= lb or r >= ub]
//   WeightedQuadraticBarrier (weighted-quadratic-barrier.hpp:35-70): lb, ub, w;
//     a = 0.5 w^2 (rl^2 + ru^2), Ar = w^2 (rl + ru), Arr = w [r <= lb or r >= ub]
// Per residual row i: value2 (twice its share of a: callers sum the rows, then
// halve), sgrad (X * Ar_i, as (X w) r for the quadratic kinds), hess (Arr_ii).
struct Act {
  int kind, nr;
  const double* p;
  MB_HD __forceinline__ double value2(int i, double r) const {
    const double* p = mb_lds(this->p);
    if (kind <= A_WEIGHTED_QUAD) return p[i] * r * r;
    const double rl = fmin(r - p[i], 0.), ru = fmax(r - p[nr + i], 0.);
    const double v = rl * rl + ru * ru;
    return kind == A_WEIGHTED_QUAD_BARRIER ? p[2 * nr + i] * p[2 * nr + i] * v : v;
  }
  MB_HD __forceinline__ double sgrad(int i, double r, double X) const {
    const double* p = mb_lds(this->p);
    if (kind <= A_WEIGHTED_QUAD) return X * p[i] * r;
    const double g = fmin(r - p[i], 0.) + fmax(r - p[nr + i], 0.);
    return X * (kind == A_WEIGHTED_QUAD_BARRIER ? p[2 * nr + i] * p[2 * nr + i] * g : g);
  }
  MB_HD __forceinline__ double hess(int i, double r) const {
    const double* p = mb_lds(this->p);
    if (kind <= A_WEIGHTED_QUAD) return p[i];
    const double h = (r - p[i] <= 0.) ? 1. : ((r - p[nr + i] >= 0.) ? 1. : 0.);
    return kind == A_WEIGHTED_QUAD_BARRIER ? p[2 * nr + i] * h : h;
  }
};
MB_HD inline Act cost_act(const Blk& b, const CRec& C, int nu) {
  const int nr = cost_nr(b, C, nu), kind = (int)C.r[2];
  const int np = kind <= A_WEIGHTED_QUAD ? nr : (kind == A_QUAD_BARRIER ? 2 * nr : 3 * nr);
  return Act{kind, nr, C.r + C.size() - np};
}
// costs whose residual Jacobian is dense over the configuration tangent (stored
// per cost: rows x jw, jw = nj, or 2 nj when a frame-velocity cost needs the
// velocity columns too; so does a centroidal-momentum cost): frame costs, CoM, frame velocity,
// centroidal momentum, the free-flyer block of a state cost, and the impulse CoM cost (its slot
// holds d(Jcom w)/dq and Jcom, three rows each: the rows of R are formed from them and Fx,
// knot_calc_diff_x)
MB_HD __forceinline__ bool jac_cost(const Blk& b, int type) {
  return type == C_FRAME_PLACEMENT || type == C_FRAME_TRANSLATION || type == C_COM_POSITION ||
         type == C_FRAME_VELOCITY || type == C_FRAME_ROTATION || type == C_IMPULSE_COM ||
         type == C_CENTROIDAL_MOMENTUM || (type == C_STATE && b.ff);
}
MB_HD __forceinline__ int jac_rows(int type) {
  const bool three =
      type == C_FRAME_TRANSLATION || type == C_COM_POSITION || type == C_FRAME_ROTATION || type == C_IMPULSE_COM;
  return three ? 3 : 6;
}
MB_HD inline int count_jac_costs(const Blk& b, bool* vel_cols = nullptr) {
  int n = 0;
  bool fv = false;
  const double* cr = b.C;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    if (jac_cost(b, C.type())) ++n;
    if (C.type() == C_FRAME_VELOCITY || C.type() == C_CENTROIDAL_MOMENTUM) fv = true;
    cr += C.size();
  }
  if (vel_cols) *vel_cols = fv;
  return n;
}
// costs on the contact multipliers: CostModelContactForce, CostModelContactFrictionCone,
// CostModelContactCoPPosition
MB_HD __forceinline__ bool force_cost(int type) {
  return type == C_CONTACT_FORCE || type == C_FRICTION_CONE || type == C_COP_POSITION;
}
// columns of the matrix A of a cone / CoP record: the multipliers its rows read (the
// linear three of the contact, or the whole wrench of a 6D one)
MB_HD __forceinline__ int force_cols(int type) { return type == C_COP_POSITION ? 6 : 3; }
// Residual rows with a dense Jacobian (jac costs; force costs on an active contact or
// impulse when the multiplier Jacobians are computed): the rows of the stacked R of calcDiff.
MB_HD inline int count_cost_rows(const Blk& b, int nu) {
  int n = 0;
  const bool fd = b.enable_force && b.nc > 0;
  const double* cr = b.C;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    if (jac_cost(b, C.type())) n += jac_rows(C.type());
    if (fd && force_cost(C.type()) && (int)C.d()[0] >= 0) n += cost_nr(b, C, nu);
    cr += C.size();
  }
  return n;
}
// row i of a force cost's residual from the multipliers lam of the contact rows
// [row0, row0 + nc) (lam unread for an inactive contact: lambda = 0):
//   contact force: lambda_i - fref_i (contact-force.hxx:33-50: jMf.actInv(f) is the multiplier);
//   friction cone: A_i . lambda_lin (contact-friction-cone.hxx:58)
//   CoP position: A_i . lambda (contact-cop-position.hpp), the cone's sum carried on
//     over the three torque multipliers
// (lam(k): multiplier k, so that the calc reads it where it lies, sign applied at the use)
template <class L>
MB_HD __forceinline__ double force_res_at(const CRec& C, L lam, int i) {
  const double* d = C.d();
  const int row0 = (int)d[0];
  if (C.type() == C_CONTACT_FORCE) return (row0 >= 0 ? lam(row0 + i) : 0.) - d[2 + i];
  if (row0 < 0) return 0.;
  const int nw = force_cols(C.type());
  const double* A = d + 3 + nw * i;
  double s = A[0] * lam(row0) + A[1] * lam(row0 + 1) + A[2] * lam(row0 + 2);
  for (int k = 3; k < nw; ++k) s += A[k] * lam(row0 + k);
  return s;
}
MB_HD __forceinline__ double force_res(const CRec& C, const double* lam, int i) {
  return force_res_at(C, [lam](int k) { return lam[k]; }, i);
}
// row i of a force cost's Jacobian column from the multiplier Jacobian column
// dl[row * ld] (the same linear map as force_res, without the offset)
MB_HD __forceinline__ double force_jac(const CRec& C, const double* dl, int64_t ld, int i) {
  const double* d = C.d();
  const int row0 = (int)d[0];
  if (C.type() == C_CONTACT_FORCE) return dl[(int64_t)(row0 + i) * ld];
  const int nw = force_cols(C.type());
  const double* A = d + 3 + nw * i;
  double s = A[0] * dl[(int64_t)row0 * ld] + A[1] * dl[(int64_t)(row0 + 1) * ld] + A[2] * dl[(int64_t)(row0 + 2) * ld];
  for (int k = 3; k < nw; ++k) s += A[k] * dl[(int64_t)(row0 + k) * ld];
  return s;
}
// activation value of a force cost (inactive contact: lambda = 0)
template <class L>
MB_HD __forceinline__ double force_cost_activation_at(const Blk& b, const CRec& C, L lam, int nu) {
  const Act act = cost_act(b, C, nu);
  double a = 0.;
  for (int e = 0; e < act.nr; ++e) a += act.value2(e, force_res_at(C, lam, e));
  return 0.5 * a;
}
MB_HD inline double force_cost_activation(const Blk& b, const CRec& C, const double* lam, int nu) {
  return force_cost_activation_at(b, C, [lam](int k) { return lam[k]; }, nu);
}

// Residual of a frame cost, value only (calc). Returns the residual size.
MB_HD __forceinline__ int frame_residual_value(const Blk& b, const WVals& V, const CRec& C, double* r) {
  const double* d = C.d();
  double Rf[9], pf[3];
  frame_placement(b, V, d, Rf, pf);
  if (C.type() == C_FRAME_TRANSLATION || C.type() == C_CONTACT_3D) {
    for (int e = 0; e < 3; ++e) r[e] = pf[e] - d[13 + e];
    return 3;
  }
  double Rr[9], pr[3];
  matmul3(d + 13, Rf, Rr);
  if (C.type() == C_FRAME_ROTATION) {  // log3(Rref^T oRf): log6's angular half, no translation
    for (int e = 0; e < 3; ++e) pr[e] = 0.;
    log6_t<double>(Rr, pr, r);
    for (int e = 0; e < 3; ++e) r[e] = r[3 + e];
    return 3;
  }
  matvec3(d + 13, pf, pr);
  for (int e = 0; e < 3; ++e) pr[e] += d[22 + e];
  log6_t<double>(Rr, pr, r);
  return 6;
}

// Centre of mass (pinocchio::centerOfMass) from the world body CoMs
MB_HD inline void com_value(const Blk& b, const WVals& W, double* c) {
  double m = 0., h[3] = {0., 0., 0.};
  for (int k = 0; k < b.nj; ++k) {
    if (!carries_body(b, k)) continue;
    const double mk = *W.m(k);
    m += mk;
    for (int e = 0; e < 3; ++e) h[e] += mk * W.c(k)[e];
  }
  for (int e = 0; e < 3; ++e) c[e] = h[e] / m;
}

// ---- CostModelCentroidalMomentum: r = hg(q, v) - href -----------------------------------
// The momentum about the world origin of the bodies below dof j (j < 0: of every body),
// h = sum I_b v_b, from the bodies' world velocities (W.v: after the velocity pass) and their
// mass, CoM and inertia in the D records.
MB_HD inline void subtree_momentum(const Blk& b, const WVals& W, int j, double* h) {
  for (int e = 0; e < 6; ++e) h[e] = 0.;
  for (int k = 0; k < b.nj; ++k) {
    if (!carries_body(b, k)) continue;
    if (j >= 0 && !((*W.anc(k) >> j) & 1ull)) continue;
    const double mk = *W.m(k);
    double c[3], I6[6], V[6], f[6];
    for (int e = 0; e < 3; ++e) c[e] = W.c(k)[e];
    for (int e = 0; e < 6; ++e) {
      I6[e] = W.Ic(k)[e];
      V[e] = W.v(k)[e];
    }
    inertia_mul(mk, c, I6, V, f);
    for (int e = 0; e < 6; ++e) h[e] += f[e];
  }
}
// hg of pinocchio::computeCentroidalMomentum: [l; k_O - c x l], world axes, about the CoM c
MB_HD inline void centroidal_momentum(const Blk& b, const WVals& W, double* hg) {
  double h[6], c[3], t[3];
  subtree_momentum(b, W, -1, h);
  com_value(b, W, c);
  cross3(c, h, t);
  for (int e = 0; e < 3; ++e) {
    hg[e] = h[e];
    hg[3 + e] = h[3 + e] - t[e];
  }
}

// ---- CostModelImpulseCoM: r = Jcom(q) (v+ - v), the change of the CoM velocity ----------
// lane i < nj: the mass of dof i's body times the velocity of its CoM under the generalised
// velocity w (wq(k): its entry k), o[0..2]; from the L records (oMi, S) and the block alone,
// so the rollout's calc can run it after its factorisation has overwritten the D records.
template <class Wq>
MB_HD inline void impulse_com_body(const Blk& b, const WVals& W, Wq wq, int i, double* o) {
  double v0 = 0., v1 = 0., v2 = 0., v3 = 0., v4 = 0., v5 = 0.;
  const Mask am = *W.anc(i);
  for (int k = 0; k < b.nj; ++k) {  // (selected, not branched: as w_velocity)
    const double wk = ((am >> k) & 1ull) ? wq(k) : 0.;
    const double* S = W.S(k);
    v0 += S[0] * wk;
    v1 += S[1] * wk;
    v2 += S[2] * wk;
    v3 += S[3] * wk;
    v4 += S[4] * wk;
    v5 += S[5] * wk;
  }
  const JRec J(b, rec_of(b, i));
  const double* R = W.oR(i);  // (column-major, as matvec3 reads it)
  const double* cl = J.com();
  const double c0 = W.op(i)[0] + (R[0] * cl[0] + R[3] * cl[1] + R[6] * cl[2]);
  const double c1 = W.op(i)[1] + (R[1] * cl[0] + R[4] * cl[1] + R[7] * cl[2]);
  const double c2 = W.op(i)[2] + (R[2] * cl[0] + R[5] * cl[1] + R[8] * cl[2]);
  const double m = carries_body(b, i) ? J.mass() : 0.;
  o[0] = m * (v0 + (v4 * c2 - v5 * c1));
  o[1] = m * (v1 + (v5 * c0 - v3 * c2));
  o[2] = m * (v2 + (v3 * c1 - v4 * c0));
}
// one lane: the residual from the bodies' terms p[stride * i + e] (impulse_com_body), summed in
// dof order and divided by the total mass
MB_HD inline void impulse_com_sum(const Blk& b, const double* p, int stride, double* r) {
  double mt = 0., h[3] = {0., 0., 0.};
  for (int i = 0; i < b.nj; ++i) {
    if (!carries_body(b, i)) continue;
    mt += JRec(b, rec_of(b, i)).mass();
    for (int e = 0; e < 3; ++e) h[e] += p[(int64_t)stride * i + e];
  }
  for (int e = 0; e < 3; ++e) r[e] = h[e] / mt;
}
// whether the block has an impulse CoM cost (impulse knots only: the plan refuses it elsewhere)
MB_HD inline bool has_impulse_com(const Blk& b) {
  if (!b.impulse) return false;
  bool found = false;
  const double* cr = b.C;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    found = found || C.type() == C_IMPULSE_COM;
    cr += C.size();
  }
#if MB_BLK_UNIFORM && defined(__HIP_DEVICE_COMPILE__)
  found = mb_uniform(found);  // the same in every lane: the phases it selects end in barriers
#endif
  return found;
}
// (out of line on the device: inlined they changed the inlining of the rollout kernel around
// them, and its split gains loop's arrays went to scratch)
#if defined(__HIP_DEVICE_COMPILE__)
#define MB_NOINLINE_DEV __attribute__((noinline))
#else
#define MB_NOINLINE_DEV inline
#endif
// The rollout's calc, after v+ (vp; nc == 0: v+ = v): two phases on every lane of the
// workgroup. First the bodies' terms into the velocity slots of the L records (unused on an
// impulse knot's calc), then record k's weighted value on lane 64 + k into cv[k].
MB_HD MB_NOINLINE_DEV void impulse_com_calc_bodies(const Blk& b, const WVals& W, const double* x, const double* vp, int lane) {
  if (lane >= b.nj) return;
  const double* v = x + b.nq;
  const bool act = b.nc > 0;
  double o[3];
  impulse_com_body(b, W, [=](int k) { return act ? vp[k] - v[k] : 0.; }, lane, o);
  for (int e = 0; e < 3; ++e) W.v(lane)[e] = o[e];
}
MB_HD MB_NOINLINE_DEV void impulse_com_calc_value(const Blk& b, const WVals& W, double* cv, int lane) {
  const int kf = lane - 64;
  if (kf < 0 || kf >= b.ncost) return;
  const double* cr = b.C;
  for (int k = 0; k < kf; ++k) cr += CRec{cr}.size();
  const CRec C{cr};
  if (C.type() != C_IMPULSE_COM) return;
  double r[3];
  impulse_com_sum(b, W.v(0), kWRec, r);
  const Act act = cost_act(b, C, 0);
  double a = 0.;
  for (int e = 0; e < 3; ++e) a += act.value2(e, r[e]);
  cv[kf] = C.weight() * (0.5 * a);
}
// The calc's value of a centroidal-momentum record: twice its activation. Out of line in the
// rollout's objects for the same reason (MB_MOMENTUM_OUTLINE, k_fwd.hip); inlined in the
// others, where a call would cost the calcDiff kernels spills around it.
#ifndef MB_MOMENTUM_OUTLINE
#define MB_MOMENTUM_OUTLINE 0
#endif
#if MB_MOMENTUM_OUTLINE
#define MB_MOMENTUM_INLINE MB_NOINLINE_DEV
#else
#define MB_MOMENTUM_INLINE inline
#endif
MB_HD MB_MOMENTUM_INLINE double momentum_calc_value2(const Blk& b, const WVals& W, const CRec& C) {
  double r[6];
  centroidal_momentum(b, W, r);
  const Act act = cost_act(b, C, 0);
  double a = 0.;
  for (int i = 0; i < 6; ++i) a += act.value2(i, r[i] - C.d()[i]);
  return a;
}
// whether the block has a centroidal-momentum cost
MB_HD inline bool has_momentum(const Blk& b) {
  bool found = false;
  const double* cr = b.C;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    found = found || C.type() == C_CENTROIDAL_MOMENTUM;
    cr += C.size();
  }
  return found;
}

// free-flyer block of a state residual: log6(Mref^-1 M) (multibody.hxx:69)
MB_HD inline void ff_rel(const double* xref, const double* x, double* Rr, double* pr) {
  double R0[9], R1[9], dp[3];
  quat_to_R(xref + 3, R0);
  quat_to_R(x + 3, R1);
  matTmul3(R0, R1, Rr);
  for (int e = 0; e < 3; ++e) dp[e] = x[e] - xref[e];
  matTvec3(R0, dp, pr);
}

// entry i of the state residual diff(xref, x) beyond the free-flyer block
MB_HD __forceinline__ double state_res(const Blk& b, const double* xref, const double* x, int i) {
  if (i < b.nj) return x[qof(b, i)] - xref[qof(b, i)];
  return x[b.nq + i - b.nj] - xref[b.nq + i - b.nj];
}

// LOCAL velocity of a frame payload d minus vref (pinocchio::getFrameVelocity,
// frame-velocity.hxx:57-59), from the world body velocities in V.
MB_HD inline void frame_velocity_res(const Blk& b, const WVals& V, const double* d, double* r) {
  const int j = frame_dof(b, d);
  double Rf[9], pf[3], m6[6];
  frame_placement(b, V, d, Rf, pf);
  for (int e = 0; e < 6; ++e) m6[e] = V.v(j)[e];
  motion_act_inv(Rf, pf, m6, r);
  for (int e = 0; e < 6; ++e) r[e] -= d[13 + e];
}

// Activation value of one cost record (kinematics in V; velocities in V only with
// vel: frame-velocity and centroidal-momentum costs are skipped without). Force costs and the
// impulse CoM cost return 0: they need the multipliers / v+ and are added after the contact solve.
MB_HD __forceinline__ double cost_activation(const Blk& b, const WVals& V, const CRec& C, const double* x,
                                             const double* u, int nu, bool vel = true) {
  const Act act = cost_act(b, C, nu);
  double a = 0.;
  if (C.type() == C_STATE) {
    const int ndx = 2 * b.nj;
    int i0 = 0;
    if (b.ff) {
      double Rr[9], pr[3], r[6];
      ff_rel(C.d(), x, Rr, pr);
      log6_t<double>(Rr, pr, r);
      for (int e = 0; e < 6; ++e) a += act.value2(e, r[e]);
      i0 = 6;
    }
    for (int i = i0; i < ndx; ++i) a += act.value2(i, state_res(b, C.d(), x, i));
  } else if (C.type() == C_CONTROL) {
    for (int i = 0; i < nu; ++i) a += act.value2(i, u[i] - C.d()[i]);
  } else if (force_cost(C.type()) || C.type() == C_IMPULSE_COM) {  // (the impulse CoM cost: after v+)
    return 0.;
  } else if (C.type() == C_COM_POSITION) {
    double c[3];
    com_value(b, V, c);
    for (int i = 0; i < 3; ++i) a += act.value2(i, c[i] - C.d()[i]);
  } else if (C.type() == C_FRAME_VELOCITY) {
    if (!vel) return 0.;
    double r[6];
    frame_velocity_res(b, V, C.d(), r);
    for (int i = 0; i < 6; ++i) a += act.value2(i, r[i]);
#if MB_CALC_MOMENTUM
  } else if (C.type() == C_CENTROIDAL_MOMENTUM) {
    if (!vel) return 0.;
    a = momentum_calc_value2(b, V, C);
#endif
  } else {
    double r[6] = {0., 0., 0., 0., 0., 0.};
    const int nr = frame_residual_value(b, V, C, r);
#pragma unroll
    for (int i = 0; i < 6; ++i)  // fixed trip count: r stays in registers
      if (i < nr) a += act.value2(i, r[i]);
  }
  return 0.5 * a;
}

// The long vector residuals (state, control) are summed lane-parallel in the calc:
// wide_cost says which records (the first kMaxWide such records) take that path.
constexpr int kMaxWide = 2;
MB_HD __forceinline__ bool wide_cost(const CRec& C, int nwide) {
  return (C.type() == C_STATE || C.type() == C_CONTROL) && nwide < kMaxWide;
}
// Lane l's share of twice the activation of a wide record: the rows i = l (mod L)
// (lane 0 also the free-flyer block of a state residual, log6 of the base).
MB_HD __forceinline__ double cost_activation_part(const Blk& b, const CRec& C, const double* x, const double* u,
                                                  int nu, int l, int L) {
  const Act act = cost_act(b, C, nu);
  double a = 0.;
  if (C.type() == C_STATE) {
    const int ndx = 2 * b.nj, i0 = b.ff ? 6 : 0;
    if (b.ff && l == 0) {
      double Rr[9], pr[3], r[6];
      ff_rel(C.d(), x, Rr, pr);
      log6_t<double>(Rr, pr, r);
      for (int e = 0; e < 6; ++e) a += act.value2(e, r[e]);
    }
    for (int i = i0 + l; i < ndx; i += L) a += act.value2(i, state_res(b, C.d(), x, i));
  } else {
    for (int i = l; i < nu; i += L) a += act.value2(i, u[i] - C.d()[i]);
  }
  return a;
}

// Cost value of the DAM (one thread; kinematics and velocities in V): sum of
// weight * activation in record (name) order (cost-sum.hxx:89-117).
MB_HD inline double cost_value(const Blk& b, const WVals& V, const double* x, const double* u, int nu) {
  double total = 0.;
  const double* cr = b.C;
  for (int k = 0; k < b.ncost; ++k) {
    const CRec C{cr};
    total += C.weight() * cost_activation(b, V, C, x, u, nu);
    cr += C.size();
  }
  return total;
}

// ---- contacts (ContactModel3D / 6D in the LOCAL frame) ----------------------
// Row offset of contact record k and its record pointer.
MB_HD inline const double* contact_rec(const Blk& b, int k, int* row0) {
  const double* r = b.K;
  int row = 0;
  for (int i = 0; i < k; ++i) {
    row += (int)r[0] == C_CONTACT_3D ? 3 : 6;
    r += (int)r[3];
  }
  *row0 = row;
  return r;
}

// a0 of a contact (contact-3d.hxx:35-43, contact-6d.hxx:31-44) in two parts,
// so that neither holds log6 and the frame motions live at once: the
// Baumgarte position term kp * (p - p_ref) | kp * log6(Mref^-1 oMf) (needs only
// the placements), then the frame drift acceleration (classical for 3D, gravity
// removed) + kd * v from the world velocity / acceleration of the body.
MB_HD __attribute__((always_inline)) inline void contact_a0_position(const Blk& b, const WVals& W, const CRec& C, double* a0) {
  const double kp = C.r[1];
  double r[6] = {0., 0., 0., 0., 0., 0.};
  if (kp != 0.) frame_residual_value(b, W, C, r);
  const int n = C.type() == C_CONTACT_3D ? 3 : 6;
#pragma unroll
  for (int e = 0; e < 6; ++e)  // fixed trip count: r stays in registers
    if (e < n) a0[e] = kp * r[e];
}
MB_HD __attribute__((always_inline)) inline void contact_a0_drift(const Blk& b, const WVals& W, const CRec& C, double* a0) {
  const double* d = C.d();
  const int j = frame_dof(b, d);
  double Rf[9], pf[3], m6[6], vf[6], af[6];
  frame_placement(b, W, d, Rf, pf);
  for (int e = 0; e < 6; ++e) m6[e] = W.v(j)[e];
  motion_act_inv(Rf, pf, m6, vf);
  for (int e = 0; e < 6; ++e) m6[e] = W.a(j)[e] - W.root_a()[e];  // data.a has no gravity
  motion_act_inv(Rf, pf, m6, af);
  const double kd = C.r[2];
  if (C.type() == C_CONTACT_3D) {
    double wxv[3];
    cross3(vf + 3, vf, wxv);
    for (int e = 0; e < 3; ++e) a0[e] += af[e] + wxv[e] + kd * vf[e];
  } else {
    for (int e = 0; e < 6; ++e) a0[e] += af[e] + kd * vf[e];
  }
}

// World force (at the origin) of contact record C for the multipliers lam
// (updateForce: jMf.act(Force(lambda[, 0])), contact-3d.hxx:59-67).
MB_HD inline void contact_world_force(const Blk& b, const WVals& W, const CRec& C, const double* lam, double* o) {
  double Rf[9], pf[3], f[6];
  frame_placement(b, W, C.d(), Rf, pf);
  const bool c3 = C.type() == C_CONTACT_3D;
  for (int e = 0; e < 6; ++e) f[e] = (c3 && e >= 3) ? 0. : lam[e];
  force_act(Rf, pf, f, o);
}

// lane j < nj: sum of the contact forces acting on dof j's body (world) into fx[6j..]
MB_HD inline void contact_joint_forces(const Blk& b, const WVals& W, const double* lam, double* fx, int j) {
  double F[6] = {0., 0., 0., 0., 0., 0.};
  const double* r = b.K;
  int row = 0;
  for (int k = 0; k < b.ncon; ++k) {
    const CRec C{r};
    if (frame_dof(b, C.d()) == j) {
      double o[6];
      contact_world_force(b, W, C, lam + row, o);
      for (int e = 0; e < 6; ++e) F[e] += o[e];
    }
    row += C.type() == C_CONTACT_3D ? 3 : 6;
    r += C.size();
  }
  for (int e = 0; e < 6; ++e) fx[6 * j + e] = F[e];
}

// lane c < nj: column c of the stacked contact Jacobian Jc (nc x nj,
// Jc[row * nj + c]) — the LOCAL frame Jacobian (pinocchio getFrameJacobian LOCAL,
// contact-3d.hxx:29 / contact-6d.hxx:29): the world motion S_c moved to the frame
// (SE3::actInv of oMf), zero unless c moves the frame's body; with At != null also
// into the columns [nj + row] of A (ld lda).
MB_HD __attribute__((always_inline)) inline void contact_jac_lane(const Blk& b, const WVals& W, int c, double* Jc, double* At,
                                                      int lda = 0) {
  double Sc[6];
  for (int e = 0; e < 6; ++e) Sc[e] = W.S(c)[e];
  const double* r = b.K;
  int row = 0;
  for (int k = 0; k < b.ncon; ++k) {
    const CRec C{r};
    const int j = frame_dof(b, C.d());
    double o[6] = {0., 0., 0., 0., 0., 0.};
    if ((*W.anc(j) >> c) & 1ull) {
      double Rf[9], pf[3];
      frame_placement(b, W, C.d(), Rf, pf);
      motion_act_inv(Rf, pf, Sc, o);
    }
    const int n = C.type() == C_CONTACT_3D ? 3 : 6;
    for (int e = 0; e < n; ++e) {
      Jc[(int64_t)(row + e) * b.nj + c] = o[e];
      if (At) At[(int64_t)(b.nj + row + e) * lda + c] = o[e];
    }
    row += n;
    r += C.size();
  }
}

}  // namespace mb
}  // namespace fddp
