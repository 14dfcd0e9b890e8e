// Multibody knots, spatial algebra: 3-vectors and rotations, spatial cross and inertia
// products, the joint records (JRec) with the dof / body helpers, quaternions.
#pragma once

#include "mb_base.hpp"

namespace fddp {
namespace mb {

// ---- 3-vectors / rotations (column-major 3x3: R[c*3 + r]) ------------------
MB_HD __forceinline__ void cross3(const double* a, const double* b, double* o) {
  const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x;
  o[1] = y;
  o[2] = z;
}
MB_HD __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
MB_HD __forceinline__ void matvec3(const double* R, const double* v, double* o) {  // o = R v
  const double x = R[0] * v[0] + R[3] * v[1] + R[6] * v[2];
  const double y = R[1] * v[0] + R[4] * v[1] + R[7] * v[2];
  const double z = R[2] * v[0] + R[5] * v[1] + R[8] * v[2];
  o[0] = x;
  o[1] = y;
  o[2] = z;
}
MB_HD __forceinline__ void matTvec3(const double* R, const double* v, double* o) {  // o = R^T v
  const double x = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  const double y = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  const double z = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
  o[0] = x;
  o[1] = y;
  o[2] = z;
}
MB_HD __forceinline__ void matmul3(const double* A, const double* B, double* O) {  // O = A B
  for (int c = 0; c < 3; ++c) matvec3(A, B + 3 * c, O + 3 * c);
}
MB_HD __forceinline__ void matTmul3(const double* A, const double* B, double* O) {  // O = A^T B
  for (int c = 0; c < 3; ++c) matTvec3(A, B + 3 * c, O + 3 * c);
}

// Spatial algebra in (linear, angular) order, as Pinocchio's Motion / Force.
// actInv on a motion by M = (R, p): lin' = R^T (v - p x w), ang' = R^T w.
MB_HD __forceinline__ void motion_act_inv(const double* R, const double* p, const double* m, double* o) {
  double t[3];
  cross3(p, m + 3, t);
  t[0] = m[0] - t[0];
  t[1] = m[1] - t[1];
  t[2] = m[2] - t[2];
  matTvec3(R, t, o);
  matTvec3(R, m + 3, o + 3);
}
// act on a force (child -> parent): f' = R f, n' = R n + p x f'.
MB_HD __forceinline__ void force_act(const double* R, const double* p, const double* f, double* o) {
  double ff[3], nn[3], t[3];
  matvec3(R, f, ff);
  matvec3(R, f + 3, nn);
  cross3(p, ff, t);
  o[0] = ff[0];
  o[1] = ff[1];
  o[2] = ff[2];
  o[3] = nn[0] + t[0];
  o[4] = nn[1] + t[1];
  o[5] = nn[2] + t[2];
}
// m1 x_motion m2 = (w1 x v2 + v1 x w2, w1 x w2)
MB_HD __forceinline__ void cross_m(const double* m1, const double* m2, double* o) {
  double a[3], b[3], c[3];
  cross3(m1 + 3, m2, a);
  cross3(m1, m2 + 3, b);
  cross3(m1 + 3, m2 + 3, c);
  o[0] = a[0] + b[0];
  o[1] = a[1] + b[1];
  o[2] = a[2] + b[2];
  o[3] = c[0];
  o[4] = c[1];
  o[5] = c[2];
}
// m x_force f = (w x f, w x n + v x f)
MB_HD __forceinline__ void cross_f(const double* m, const double* f, double* o) {
  double a[3], b[3], c[3];
  cross3(m + 3, f, a);
  cross3(m + 3, f + 3, b);
  cross3(m, f, c);
  o[0] = a[0];
  o[1] = a[1];
  o[2] = a[2];
  o[3] = b[0] + c[0];
  o[4] = b[1] + c[1];
  o[5] = b[2] + c[2];
}
// Inertia (mass m, CoM c, rotational inertia Ic about the CoM: xx yy zz xy xz yz)
// times a motion: f = m (v - c x w), n = Ic w + c x f.
MB_HD __forceinline__ void inertia_mul(double m, const double* c, const double* I6, const double* mo, double* o) {
  double t[3];
  cross3(c, mo + 3, t);
  const double f0 = m * (mo[0] - t[0]), f1 = m * (mo[1] - t[1]), f2 = m * (mo[2] - t[2]);
  const double w0 = mo[3], w1 = mo[4], w2 = mo[5];
  const double n0 = I6[0] * w0 + I6[3] * w1 + I6[4] * w2;
  const double n1 = I6[3] * w0 + I6[1] * w1 + I6[5] * w2;
  const double n2 = I6[4] * w0 + I6[5] * w1 + I6[2] * w2;
  const double f[3] = {f0, f1, f2};
  cross3(c, f, t);
  o[0] = f0;
  o[1] = f1;
  o[2] = f2;
  o[3] = n0 + t[0];
  o[4] = n1 + t[1];
  o[5] = n2 + t[2];
}
MB_HD __forceinline__ double dot6(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}

// Joint record accessors: [type, parent record (-1 universe), axis(3), placement
// R(9) p(3), mass, CoM(3), I(6)]
struct JRec {
  const double* r;
  MB_HD JRec(const Blk& b, int i) : r(mb_lds(b.J + (int64_t)kJRec * i)) {}
  MB_HD int type() const { return (int)r[0]; }
  MB_HD int parent() const { return (int)r[1]; }
  MB_HD const double* axis() const { return r + 2; }
  MB_HD const double* Rpl() const { return r + 5; }
  MB_HD const double* ppl() const { return r + 14; }
  MB_HD double mass() const { return r[17]; }
  MB_HD const double* com() const { return r + 18; }
  MB_HD const double* I6() const { return r + 21; }
};

// ---- dofs and bodies --------------------------------------------------------
// Dof d is one lane. A free-flyer record expands into dofs 0..5 (base twist:
// linear 0..2 along, angular 3..5 about the base axes) that share one body, whose
// inertia sits on dof 5; placements compose along 0 -> 1 -> .. -> 5 with the base
// pose on dof 0 and identities after it. Every other record is one dof, revolute (about its
// axis) or prismatic (along it).
MB_HD __forceinline__ int rec_of(const Blk& b, int d) { return b.ff ? (d < 6 ? 0 : d - 5) : d; }
// the dof that carries record r's body (and its frames)
MB_HD __forceinline__ int dof_of_rec(const Blk& b, int r) { return b.ff ? (r == 0 ? 5 : r + 5) : r; }
// configuration index of a one-dof joint (an angle or a length)
MB_HD __forceinline__ int qof(const Blk& b, int d) { return b.ff ? d + 1 : d; }
// the dof carrying the parent body (-1: universe)
MB_HD __forceinline__ int body_parent(const Blk& b, int d) {
  if (b.ff && d < 6) return -1;
  const int pr = JRec(b, rec_of(b, d)).parent();
  return pr < 0 ? -1 : dof_of_rec(b, pr);
}
// placement composition parent (free-flyer dofs chain 0 -> 5)
MB_HD __forceinline__ int chain_parent(const Blk& b, int d) { return (b.ff && d < 6) ? d - 1 : body_parent(b, d); }
MB_HD __forceinline__ Mask own_mask(const Blk& b, int d) { return (b.ff && d < 6) ? Mask(0x3F) : (Mask(1) << d); }
// dofs whose body is an ancestor-or-self of d's body
MB_HD inline Mask anc_mask(const Blk& b, int d) {
  Mask m = own_mask(b, d);
  for (int k = body_parent(b, d); k >= 0; k = body_parent(b, k)) m |= own_mask(b, k);
  return m;
}
MB_HD __forceinline__ bool carries_body(const Blk& b, int d) { return !(b.ff && d < 5); }
// joint-frame axis of dof d; prismatic: translation along it (free-flyer 0..2)
#if MB_PRISMATIC
MB_HD __forceinline__ bool dof_prismatic(const Blk& b, int d) { return (b.pris >> d) & 1ull; }
#else
MB_HD __forceinline__ bool dof_prismatic(const Blk& b, int d) { return b.ff && d < 3; }
#endif
MB_HD __forceinline__ void dof_axis(const Blk& b, int d, double* ax) {
  if (b.ff && d < 6) {
    ax[0] = d % 3 == 0 ? 1. : 0.;
    ax[1] = d % 3 == 1 ? 1. : 0.;
    ax[2] = d % 3 == 2 ? 1. : 0.;
  } else {
    const double* a = JRec(b, rec_of(b, d)).axis();
    ax[0] = a[0];
    ax[1] = a[1];
    ax[2] = a[2];
  }
}

// R = Rpl * exp(q [axis]x)  (Rodrigues: c I + s [a]x + (1 - c) a a^T)
MB_HD inline void joint_rotation(const double* Rpl, const double* ax, double q, double* R) {
  double s, c;
  sincos(q, &s, &c);
  const double oc = 1. - c;
  double Rj[9];
  Rj[0] = c + oc * ax[0] * ax[0];
  Rj[1] = oc * ax[1] * ax[0] + s * ax[2];
  Rj[2] = oc * ax[2] * ax[0] - s * ax[1];
  Rj[3] = oc * ax[0] * ax[1] - s * ax[2];
  Rj[4] = c + oc * ax[1] * ax[1];
  Rj[5] = oc * ax[2] * ax[1] + s * ax[0];
  Rj[6] = oc * ax[0] * ax[2] + s * ax[1];
  Rj[7] = oc * ax[1] * ax[2] - s * ax[0];
  Rj[8] = c + oc * ax[2] * ax[2];
  matmul3(Rpl, Rj, R);
}

// Eigen QuaternionBase::toRotationMatrix, quaternion (x, y, z, w); column-major R
MB_HD inline void quat_to_R(const double* qv, double* R) {
  const double x = qv[0], y = qv[1], z = qv[2], w = qv[3];
  const double tx = 2. * x, ty = 2. * y, tz = 2. * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1. - (tyy + tzz);
  R[1] = txy + twz;
  R[2] = txz - twy;
  R[3] = txy - twz;
  R[4] = 1. - (txx + tzz);
  R[5] = tyz + twx;
  R[6] = txz + twy;
  R[7] = tyz - twx;
  R[8] = 1. - (txx + tyy);
}

// Eigen's quaternion from a rotation matrix (quaternionbase_assign_impl), with the
// index selection written as explicit selects (no runtime-indexed arrays).
MB_HD inline void R_to_quat(const double* R, double* q) {
  auto at = [&](int r, int c) { return R[c * 3 + r]; };
  const double t = at(0, 0) + at(1, 1) + at(2, 2);
  if (t > 0.) {
    double s = sqrt(t + 1.);
    q[3] = 0.5 * s;
    s = 0.5 / s;
    q[0] = (at(2, 1) - at(1, 2)) * s;
    q[1] = (at(0, 2) - at(2, 0)) * s;
    q[2] = (at(1, 0) - at(0, 1)) * s;
    return;
  }
  int i = 0;
  if (at(1, 1) > at(0, 0)) i = 1;
  if (at(2, 2) > (i == 0 ? at(0, 0) : at(1, 1))) i = 2;
  if (i == 0) {
    double s = sqrt(at(0, 0) - at(1, 1) - at(2, 2) + 1.);
    q[0] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (at(2, 1) - at(1, 2)) * s;
    q[1] = (at(1, 0) + at(0, 1)) * s;
    q[2] = (at(2, 0) + at(0, 2)) * s;
  } else if (i == 1) {
    double s = sqrt(at(1, 1) - at(2, 2) - at(0, 0) + 1.);
    q[1] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (at(0, 2) - at(2, 0)) * s;
    q[2] = (at(2, 1) + at(1, 2)) * s;
    q[0] = (at(0, 1) + at(1, 0)) * s;
  } else {
    double s = sqrt(at(2, 2) - at(0, 0) - at(1, 1) + 1.);
    q[2] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (at(1, 0) - at(0, 1)) * s;
    q[0] = (at(0, 2) + at(2, 0)) * s;
    q[1] = (at(1, 2) + at(2, 1)) * s;
  }
}

}  // namespace mb
}  // namespace fddp
