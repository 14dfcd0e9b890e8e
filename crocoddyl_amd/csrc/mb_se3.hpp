// Multibody knots, SE(3) for the free-flyer state and the frame costs: exp6 / log6 on plain
// and dual numbers, ff_integrate / ff_difference, the Jexp6 / Jlog6 columns.
#pragma once

#include "mb_spatial.hpp"

namespace fddp {
namespace mb {

// ---- dual numbers for the exp6 / log6 Jacobians ----------------------------
struct Dual {
  double v, d;
  Dual() = default;
  MB_HD constexpr Dual(double v_, double d_ = 0.) : v(v_), d(d_) {}
};
MB_HD __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
MB_HD __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
MB_HD __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
MB_HD __forceinline__ Dual operator*(double s, Dual a) { return {s * a.v, s * a.d}; }
MB_HD __forceinline__ Dual operator/(Dual a, Dual b) { return {a.v / b.v, (a.d * b.v - a.v * b.d) / (b.v * b.v)}; }
MB_HD __forceinline__ Dual msqrt(Dual a) {
  const double s = sqrt(a.v);
  return {s, a.d / (2. * s)};
}
MB_HD __forceinline__ Dual masin(Dual a) { return {asin(a.v), a.d / sqrt(1. - a.v * a.v)}; }
MB_HD __forceinline__ Dual macos(Dual a) { return {acos(a.v), -a.d / sqrt(1. - a.v * a.v)}; }
MB_HD __forceinline__ Dual msin(Dual a) { return {sin(a.v), a.d * cos(a.v)}; }
MB_HD __forceinline__ Dual mcos(Dual a) { return {cos(a.v), -a.d * sin(a.v)}; }
MB_HD __forceinline__ double mval(Dual a) { return a.v; }
MB_HD __forceinline__ double msqrt(double a) { return sqrt(a); }
MB_HD __forceinline__ double masin(double a) { return asin(a); }
MB_HD __forceinline__ double macos(double a) { return acos(a); }
MB_HD __forceinline__ double msin(double a) { return sin(a); }
MB_HD __forceinline__ double mcos(double a) { return cos(a); }
MB_HD __forceinline__ double mval(double a) { return a; }

// log6(R, p) -> (lin, ang) (pinocchio::log6), R column-major. T = double, or
// Dual so that the tangent along (dR, dp) is Jlog6 * xi. Same branches as
// oracle/multibody_np.py:log3/log6.
template <class T>
MB_HD inline void log6_t(const T* R, const T* p, T* out) {
  auto at = [&](int r, int c) { return R[c * 3 + r]; };
  const T one(1.);
  const T tr = at(0, 0) + at(1, 1) + at(2, 2);
  const T c = 0.5 * (tr - one);
  const T w[3] = {at(2, 1) - at(1, 2), at(0, 2) - at(2, 0), at(1, 0) - at(0, 1)};
  const T s2 = 0.25 * (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  T om[3];
  T sth = T(0.), thg = T(0.);  // sin(theta), theta of the generic branch (beta reuses them)
  bool generic = false;
  if (mval(s2) < 1e-8 && mval(c) > 0.) {
    const T k = 0.5 * (one + (1. / 6.) * s2 + (3. / 40.) * (s2 * s2) + (5. / 112.) * (s2 * s2 * s2));
    for (int e = 0; e < 3; ++e) om[e] = k * w[e];
  } else if (mval(s2) < 1e-8) {  // theta near pi: axis from the symmetric part (value only)
    // (explicit selects: no runtime-indexed arrays, which would live in scratch)
    const double cv = mval(c) < -1. ? -1. : mval(c);
    const double th = acos(cv);
    auto axc = [&](double d) {
      const double t = (d - cv) / (1. - cv);
      return t > 0. ? sqrt(t) : 0.;
    };
    const double a0 = axc(mval(at(0, 0))), a1 = axc(mval(at(1, 1))), a2 = axc(mval(at(2, 2)));
    const int i0 = (a1 > a0) ? ((a2 > a1) ? 2 : 1) : ((a2 > a0) ? 2 : 0);
    const double s01 = mval(at(0, 1)) + mval(at(1, 0)), s02 = mval(at(0, 2)) + mval(at(2, 0)),
                 s12 = mval(at(1, 2)) + mval(at(2, 1));
    auto sgn = [](double v) { return v >= 0. ? 1. : -1.; };
    const double g0 = i0 == 0 ? 1. : (i0 == 1 ? sgn(s01) : sgn(s02));
    const double g1 = i0 == 1 ? 1. : (i0 == 0 ? sgn(s01) : sgn(s12));
    const double g2 = i0 == 2 ? 1. : (i0 == 0 ? sgn(s02) : sgn(s12));
    const double wi = i0 == 0 ? mval(w[0]) : (i0 == 1 ? mval(w[1]) : mval(w[2]));
    const double flip = wi < 0. ? -th : th;
    om[0] = T(flip * g0 * a0);
    om[1] = T(flip * g1 * a1);
    om[2] = T(flip * g2 * a2);
  } else {
    const T s = msqrt(s2);
    T th;
    if (mval(c) > 0.5)
      th = masin(s);
    else if (mval(c) < -0.5)
      th = T(M_PI) - masin(s);
    else
      th = macos(c);
    const T k = th / (2. * s);
    for (int e = 0; e < 3; ++e) om[e] = k * w[e];
    sth = s;
    thg = th;
    generic = true;
  }
  const T t2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
  T beta;
  if (mval(t2) < 1e-2) {
    beta = T(1. / 12.) + (1. / 720.) * t2 + (1. / 30240.) * (t2 * t2) + (1. / 1209600.) * (t2 * t2 * t2);
  } else if (generic) {  // 1/t^2 - sin t / (2 t (1 - cos t)) with sin, cos of theta read off R
    beta = one / (thg * thg) - sth / (2. * thg * (one - c));
  } else {
    const T t = msqrt(t2);
    beta = one / t2 - msin(t) / (2. * t * (one - mcos(t)));
  }
  // v = (I - 0.5 [w]x + beta [w]x^2) p ; [w]x^2 p = w (w.p) - |w|^2 p
  const T wp = om[0] * p[0] + om[1] * p[1] + om[2] * p[2];
  const T wxp[3] = {om[1] * p[2] - om[2] * p[1], om[2] * p[0] - om[0] * p[2], om[0] * p[1] - om[1] * p[0]};
  for (int e = 0; e < 3; ++e) {
    const T w2p = om[e] * wp - t2 * p[e];
    out[e] = p[e] - 0.5 * wxp[e] + beta * w2p;
    out[3 + e] = om[e];
  }
}

// exp6(nu) -> (R, p) (pinocchio::exp6): R = cos t I + (1 - cos t)/t^2 w w^T +
// sin t / t [w]x, p = sin t / t v + (1 - sin t / t)/t^2 (w.v) w + (1 - cos t)/t^2 w x v,
// Taylor branch for t^2 < 1e-8 (as oracle/multibody_np.py:exp6). T = double or Dual.
template <class T>
MB_HD inline void exp6_t(const T* nu, T* R, T* p) {
  const T* v = nu;
  const T* w = nu + 3;
  const T t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  T ct, st_t, a_wxv, a_w;
  if (mval(t2) < 1e-8) {
    ct = T(1.) - 0.5 * t2 + (1. / 24.) * (t2 * t2);
    st_t = T(1.) - (1. / 6.) * t2 + (1. / 120.) * (t2 * t2);
    a_wxv = T(0.5) - (1. / 24.) * t2 + (1. / 720.) * (t2 * t2);
    a_w = T(1. / 6.) - (1. / 120.) * t2 + (1. / 5040.) * (t2 * t2);
  } else {
    const T t = msqrt(t2);
    ct = mcos(t);
    st_t = msin(t) / t;
    a_wxv = (T(1.) - ct) / t2;
    a_w = (T(1.) - st_t) / t2;
  }
  // column-major R[c*3 + r] = ct d_rc + a_wxv w_r w_c + st_t [w]x(r, c)
  R[0] = ct + a_wxv * (w[0] * w[0]);
  R[1] = a_wxv * (w[1] * w[0]) + st_t * w[2];
  R[2] = a_wxv * (w[2] * w[0]) - st_t * w[1];
  R[3] = a_wxv * (w[0] * w[1]) - st_t * w[2];
  R[4] = ct + a_wxv * (w[1] * w[1]);
  R[5] = a_wxv * (w[2] * w[1]) + st_t * w[0];
  R[6] = a_wxv * (w[0] * w[2]) + st_t * w[1];
  R[7] = a_wxv * (w[1] * w[2]) - st_t * w[0];
  R[8] = ct + a_wxv * (w[2] * w[2]);
  const T wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2];
  const T wxv[3] = {w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]};
  for (int e = 0; e < 3; ++e) p[e] = st_t * v[e] + a_w * wv * w[e] + a_wxv * wxv[e];
}

// pinocchio SpecialEuclideanOperationTpl<3>::integrate: M1 = M0 exp6(dq); the
// quaternion re-extracted from M1's rotation, flipped into q0's hemisphere and
// first-order normalised. q7 = (p, quat xyzw); out may not alias q7.
MB_HD inline void ff_integrate(const double* q7, const double* dq, double* out) {
  double R0[9], Re[9], pe[3], R1[9], t[3];
  quat_to_R(q7 + 3, R0);
  exp6_t<double>(dq, Re, pe);
  matmul3(R0, Re, R1);
  matvec3(R0, pe, t);
  out[0] = q7[0] + t[0];
  out[1] = q7[1] + t[1];
  out[2] = q7[2] + t[2];
  double qn[4];
  R_to_quat(R1, qn);
  const double dd = qn[0] * q7[3] + qn[1] * q7[4] + qn[2] * q7[5] + qn[3] * q7[6];
  const double sg = dd < 0. ? -1. : 1.;
  const double n2 = qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3];
  const double al = sg * (3. - n2) * 0.5;
  for (int e = 0; e < 4; ++e) out[3 + e] = qn[e] * al;
}
// pinocchio SpecialEuclideanOperationTpl<3>::difference: log6(M0^-1 M1).
MB_HD inline void ff_difference(const double* q0, const double* q1, double* out) {
  double R0[9], R1[9], Rr[9], dp[3], pr[3];
  quat_to_R(q0 + 3, R0);
  quat_to_R(q1 + 3, R1);
  matTmul3(R0, R1, Rr);
  dp[0] = q1[0] - q0[0];
  dp[1] = q1[1] - q0[1];
  dp[2] = q1[2] - q0[2];
  matTvec3(R0, dp, pr);
  log6_t<double>(Rr, pr, out);
}
// column k of Jexp6(nu) (pinocchio Jexp6, the right Jacobian: exp6(nu + e eps)
// = exp6(nu) exp6(J e eps)): the twist of exp6(nu)^-1 d exp6(nu + eps e_k).
MB_HD inline void jexp6_col(const double* nu, int k, double* col) {
  Dual n[6], R[9], p[3];
  for (int e = 0; e < 6; ++e) n[e] = Dual{nu[e], e == k ? 1. : 0.};
  exp6_t<Dual>(n, R, p);
  double Rv[9], dR[9], dp[3], Om[9];
  for (int e = 0; e < 9; ++e) {
    Rv[e] = R[e].v;
    dR[e] = R[e].d;
  }
  for (int e = 0; e < 3; ++e) dp[e] = p[e].d;
  matTvec3(Rv, dp, col);
  matTmul3(Rv, dR, Om);  // [xi_ang]x
  col[3] = Om[5];        // (2,1)
  col[4] = Om[6];        // (0,2)
  col[5] = Om[1];        // (1,0)
}
// column k of Jlog6(M) (pinocchio Jlog6: log6(M exp6(e eps)) = log6(M) + J e eps)
MB_HD inline void jlog6_col(const double* R, const double* p, int k, double* col) {
  double xi[6] = {0., 0., 0., 0., 0., 0.};
  xi[k] = 1.;
  double dR[9], dp[3];
  for (int c = 0; c < 3; ++c) {  // dR = R [xi_ang]x
    double t[3];
    const double e[3] = {c == 0 ? 1. : 0., c == 1 ? 1. : 0., c == 2 ? 1. : 0.};
    cross3(xi + 3, e, t);
    matvec3(R, t, dR + 3 * c);
  }
  matvec3(R, xi, dp);
  Dual RD[9], PD[3], o[6];
  for (int e = 0; e < 9; ++e) RD[e] = Dual{R[e], dR[e]};
  for (int e = 0; e < 3; ++e) PD[e] = Dual{p[e], dp[e]};
  log6_t<Dual>(RD, PD, o);
  for (int e = 0; e < 6; ++e) col[e] = o[e].d;
}

}  // namespace mb
}  // namespace fddp
