// Multibody knots, the common ground: the hooks the diagnostic tools define, the stores and
// LDS accessors all the multibody code uses, the constants and record types, and the
// parameter-block header (Blk, parse, parse_uniform).
#pragma once

#include <type_traits>

#include "fddp_device.hpp"

// Everything except the workgroup drivers (knot_calc, knot_calc_diff,
// gauss_jordan) is __host__ __device__, so the same arithmetic is unit-tested
// on the CPU against the oracle (tests/test_multibody_host.py).
#define MB_HD __host__ __device__

// Diagnostic hooks, empty in the library. A tool or the host harness defines one before it
// includes multibody.hpp (tools/mb_probe.hip: all three; tools/gj_bench.hip: MB_GJ_MARK;
// tests/cpp/mb_host.cpp: MB_DUMP):
//   MB_DUMP copies an LDS matrix, rows x cols at leading dimension ld, out of the calcDiff
//     for the parity diagnosis; every thread calls it between phases.
//   MB_GJ_MARK(id) stamps a phase boundary of gj_mfma, tree_ltdl_wave and the calcDiff.
//   MB_TILE_* count the cycles of thread 0 inside the tile loops of the calcDiff's
//     matrix-core products, summed over its tiles in registers: MB_TILE_LAP(k) adds the time
//     since the last lap to sum k, after the operands named in MB_TILE_PIN4 have arrived;
//     MB_TILE_FLUSH(base) stores the sums and the tile count.
#ifndef MB_DUMP
#define MB_DUMP(slot, ptr, rows, cols, ld)
#endif
#ifndef MB_GJ_MARK
#define MB_GJ_MARK(id)
#endif
#ifndef MB_TILE_DECL
#define MB_TILE_DECL
#define MB_TILE_START(n)
#define MB_TILE_PIN4(a)
#define MB_TILE_LAP(k)
#define MB_TILE_FLUSH(base)
#endif

// On the device every multibody record (parameter block) and the work area live in
// LDS; the record / work-area accessors re-assert it where the pointer is formed, so
// the accesses compile to ds_* even where the address-space inference loses the
// entry's assumption (flat accesses to LDS pay a full round trip each). The host
// emulation (tests/cpp/mb_host.cpp) reads ordinary memory.
// A store to the caller's output blocks, which are in HBM: through a global pointer,
// so the compiler emits global_store instead of a flat store that every later LDS
// access of the wave must wait behind (flat may alias LDS).
MB_HD __forceinline__ void mb_gstore(double* p, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(__attribute__((address_space(1))) double*)p = v;
#else
  *p = v;
#endif
}
// two consecutive doubles (16-B aligned) in one store
MB_HD __forceinline__ void mb_gstore2(double* p, double v0, double v1) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(__attribute__((address_space(1))) double2*)p = make_double2(v0, v1);
#else
  p[0] = v0;
  p[1] = v1;
#endif
}
// A fresh register copy of v (device: an empty asm the optimiser cannot see through), so
// a value live across the whole kernel is reloaded from its spill slot once, here.
template <class T>
MB_HD __forceinline__ T mb_launder(T v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (sizeof(T) == 8) {
    long long x;
    __builtin_memcpy(&x, &v, 8);
    asm volatile("" : "+v"(x));
    __builtin_memcpy(&v, &x, 8);
  } else {
    int x;
    __builtin_memcpy(&x, &v, 4);
    asm volatile("" : "+v"(x));
    __builtin_memcpy(&v, &x, 4);
  }
#endif
  return v;
}
template <class T>
MB_HD __forceinline__ T* mb_lds(T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ::fddp::lds_ptr(p);
#else
  return p;
#endif
}

// MB_LANE_OPAQUE (per kernel object): every phase of the device executor gets its lane index
// as a fresh register copy, so what a phase derives from it (addresses, lane masks) is formed
// in the phase and not hoisted out of the caller's knot loop, to be held across every other
// phase at the register cap.
#ifndef MB_LANE_OPAQUE
#define MB_LANE_OPAQUE 0
#endif
// MB_CALC_IMPULSE_COM (per kernel object): the rollout's calc evaluates CostModelImpulseCoM
// records (two phases after v+). The three-waves-per-EU rollout object is built without them,
// at its register cap they cost it spills on every horizon; the launch plan never gives it a
// horizon with such a record (LdsPlan::has_icom, plan_variants).
#ifndef MB_CALC_IMPULSE_COM
#define MB_CALC_IMPULSE_COM 1
#endif
// MB_CALC_MOMENTUM (per kernel object): the rollout's calc evaluates CostModelCentroidalMomentum
// records (with the other records, beside the CRBA composites). As MB_CALC_IMPULSE_COM: the
// three-waves-per-EU rollout object is built without it, and the launch plan never gives it a
// horizon with such a record (LdsPlan::has_hmom, plan_variants).
#ifndef MB_CALC_MOMENTUM
#define MB_CALC_MOMENTUM 1
#endif
// MB_ACTUATION (per kernel object): the knot evaluates the actuation record (tau = S u, section
// flag bit 4). As the two switches above: the three-waves-per-EU rollout object and the
// spilled-plan calcDiff object (the headline's two kernels) are built without it, and the launch
// plan never gives them a horizon with such a record (LdsPlan::has_act, plan_lds, plan_variants).
#ifndef MB_ACTUATION
#define MB_ACTUATION 1
#endif
// MB_PRISMATIC (per kernel object): joint records of type J_PRISMATIC are read (Blk::pris, one
// bit per prismatic dof; dof_prismatic tests it). As MB_ACTUATION: the headline's two kernel
// objects are built without it, where the predicate is the free-flyer's `ff && d < 3` and parse
// reads no record type beyond record 0; the launch plan never gives them a horizon with such a
// record (LdsPlan::has_pris, plan_lds, plan_variants).
#ifndef MB_PRISMATIC
#define MB_PRISMATIC 1
#endif

namespace fddp {
namespace mb {

typedef unsigned long long Mask;  // one bit per dof
constexpr int kMaxJ = 64;         // dofs (nv)
constexpr int kJRec = 27;         // doubles per joint record
constexpr int kCHdr = 4;          // doubles of a cost record's header
constexpr int kMaxJacCosts = 8;   // costs with a dense residual Jacobian (frame, CoM, impulse CoM, momentum, free-flyer state)
constexpr int kMaxNc = 24;        // stacked contact rows (FDDP_KNOT_EULER_CONTACTFWD)
constexpr int kMbDiffNT = 256;    // threads of the knot-parallel calcDiff workgroup
enum { J_REVOLUTE = 0, J_FREEFLYER = 1, J_PRISMATIC = 2 };
// Cost record types; contact records (after the costs) use 5 / 6 and the same
// frame payload as the frame costs, so frame_residual serves both.
enum {
  C_STATE = 1,
  C_CONTROL = 2,
  C_FRAME_PLACEMENT = 3,
  C_FRAME_TRANSLATION = 4,
  C_CONTACT_3D = 5,
  C_CONTACT_6D = 6,
  // (the force costs 7, 9, 11 on an impulse knot read the impulse's multipliers Lambda instead:
  // CostModelContactImpulse, CostModelImpulseFrictionCone, CostModelImpulseCoPPosition)
  C_CONTACT_FORCE = 7,  // cost on a contact's force: payload [row0, nr, fref(6)] (contact-force.hxx)
  C_COM_POSITION = 8,   // r = com(q) - cref: payload [cref(3)] (com-position.hxx:49-75)
  C_FRICTION_CONE = 9,  // r = A lambda_lin: payload [row0, nc, nr, A (nr x 3 row-major)]
                        // (contact-friction-cone.hxx:51-91)
  C_FRAME_VELOCITY = 10,  // r = LOCAL frame velocity - vref: frame payload + vref(6) (frame-velocity.hxx:53-84)
  C_COP_POSITION = 11,    // r = A lambda of a 6D contact: payload [row0, nc, nr, A (nr x 6 row-major)]
                          // (contact-cop-position.hpp)
  C_FRAME_ROTATION = 12,  // r = log3(Rref^T oRf): frame payload + Rref^T (9) (frame-rotation.hxx)
  C_IMPULSE_COM = 13,     // r = Jcom(q) (v+ - v) on an impulse knot: empty payload (CostModelImpulseCoM)
  C_CENTROIDAL_MOMENTUM = 14  // r = hg(q, v) - href, hg = [linear; angular about the CoM], world axes: payload
                              // [href(6)] (centroidal-momentum.hxx); Euler knots only
};
constexpr int C_ACTUATION = 20;  // the actuation record after the contact records: S (nv x nu, column-major)
enum { SQ_NONE = 0, SQ_SMOOTH_SAT = 1 };  // its header slot 1: the squashing kind (smooth-sat.hpp)
// Activation of a cost record: header slot 2 (core/activations/*.hpp)
enum { A_QUAD = 0, A_WEIGHTED_QUAD = 1, A_QUAD_BARRIER = 2, A_WEIGHTED_QUAD_BARRIER = 3 };
constexpr int kInactiveForceRow = -2;  // force cost on an inactive contact / impulse: lambda = 0, no Jacobians

struct Blk {
  double dt;
  int nj;   // nv: dofs
  int nq;   // nv + 1 with a free-flyer root
  int nb;   // joint records (pinocchio joints)
  bool ff;  // record 0 is a free-flyer (dofs 0..5: base twist, body on dof 5)
#if MB_PRISMATIC
  Mask pris;  // the prismatic dofs (S = [axis; 0]): a free-flyer's dofs 0..2 and every J_PRISMATIC record's
#endif
  int ncost;
  const double* g;    // gravity (3)
  const double* arm;  // armature (nv)
  const double* J;    // joint records
  const double* C;    // cost records
  // contact section (DifferentialActionModelContactFwdDynamics); ncon == 0 without
  int nun;            // leading unactuated dofs: tau = [0_nun; u], nu = nj - nun
                      // (with an actuation record: nj - nu, so that nu = nj - nun holds everywhere)
  const double* S;    // the actuation record's matrix dtau/du (nj x nu, column-major): tau = S u; null without
#if MB_ACTUATION
  const double* sq;   // squashing kind 1 (smooth-sat) of that record: lb(nu), ub(nu), a(nu), tau = S s(u); null without
#endif
  int ncon, nc;       // active contact records, stacked rows
  double damping;     // JMinvJt_damping
  const double* K;    // contact records
  // impulse section instead (ActionModelImpulseFwdDynamics, nu = 0)
  bool impulse;
  double r_coeff;     // restitution coefficient
  bool enable_force;  // section flag bit 2 (contact: 2, impulse: 3): the multiplier Jacobians of the force costs
};
// Row i of S u (S nj x nu column-major and u in LDS on the device). Out of line there: a knot
// without the record pays a uniform branch around a call, and the kernels' register allocation
// around it stays what it was (inlined it sent the rollout's split gains loop's arrays to scratch,
// as the momentum record did: MB_MOMENTUM_OUTLINE).
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline)) double act_row_dot(const double* S_, const double* u_, int nj, int nu, int i) {
  const double* S = ::fddp::lds_ptr(S_);
  const double* u = ::fddp::lds_ptr(u_);
#else
inline double act_row_dot(const double* S, const double* u, int nj, int nu, int i) {
#endif
  double s = 0.;
  for (int c = 0; c < nu; ++c) s += S[(int64_t)c * nj + i] * u[c];
  return s;
}
// Smooth-sat squashing of control c (record slots lb, ub, a at sq, nu apart; LDS on the device):
//   s = 0.5 (sqrt((u - lb)^2 + a) - sqrt((u - ub)^2 + a) + lb + ub),
//   D = ds/du = 0.5 ((u - lb) / sqrt((u - lb)^2 + a) - (u - ub) / sqrt((u - ub)^2 + a)),
// two square roots per control (a > 0: the launch plan refuses a = 0, where D is 0/0 on a bound).
// Out of line on the device, as act_row_dot. s into o[c]; with `diff` (the calcDiff) D into o[nu + c].
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline)) void squash_eval(const double* sq_, int nu, int c, double u, double* o_, bool diff) {
  const double* sq = ::fddp::lds_ptr(sq_);
  double* o = ::fddp::lds_ptr(o_);
#else
inline void squash_eval(const double* sq, int nu, int c, double u, double* o, bool diff) {
#endif
  const double lb = sq[c], ub = sq[nu + c], a = sq[2 * nu + c];
  const double dl = u - lb, du = u - ub;
  const double rl = sqrt(dl * dl + a), ru = sqrt(du * du + a);
  o[c] = 0.5 * (rl - ru + lb + ub);
  if (diff) o[nu + c] = 0.5 * (dl / rl - du / ru);
}
// tau_i of the knot's actuation at u (nu entries): S u with an actuation record, else [0_nun; u]
// (a squashed record: the caller passes s(u), formed once per knot by squash_eval)
MB_HD __forceinline__ double act_tau(const Blk& b, const double* u, int i) {
#if MB_ACTUATION
  if (b.S) return act_row_dot(b.S, u, b.nj, b.nj - b.nun, i);
#endif
  return i < b.nun ? 0. : u[i - b.nun];
}

#if MB_PRISMATIC
// One bit per prismatic dof of the nb joint records at J (LDS on the device): a free-flyer's dofs
// 0..2 and every J_PRISMATIC record's dof. Out of line on the device, as act_row_dot: a knot pays
// a call per parse, and the kernels' register allocation around it stays what it was (inlined,
// the loop cost the 128-thread calcDiff kernel, at its 168-VGPR cap, 15 more VGPR spills; out of
// line 7).
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline)) Mask pris_mask(const double* J_, int nb, bool ff) {
  const double* J = ::fddp::lds_ptr(J_);
#else
inline Mask pris_mask(const double* J, int nb, bool ff) {
#endif
  Mask m = ff ? Mask(7) : Mask(0);
  for (int r = ff ? 1 : 0; r < nb; ++r)
    if ((int)J[kJRec * r] == J_PRISMATIC) m |= Mask(1) << (ff ? r + 5 : r);
  return m;
}
#endif

MB_HD inline Blk parse(const double* P) {
  Blk b;
  b.dt = P[0];
  b.nj = (int)P[1];
  b.ncost = (int)P[2];
  b.g = P + FDDP_PARAM_HEADER;
  b.arm = b.g + 3;
  b.J = b.arm + b.nj;
  b.ff = (int)b.J[0] == J_FREEFLYER;
  b.nb = b.ff ? b.nj - 5 : b.nj;
  b.nq = b.ff ? b.nj + 1 : b.nj;
#if MB_PRISMATIC
  b.pris = pris_mask(b.J, b.nb, b.ff);
#endif
  b.C = b.J + (int64_t)kJRec * b.nb;
  const double* e = b.C;
  for (int k = 0; k < b.ncost; ++k) e += (int)e[3];
  b.nun = 0;
  b.ncon = b.nc = 0;
  b.damping = 0.;
  b.K = e;
  b.impulse = false;
  b.enable_force = false;
  b.r_coeff = 0.;
  b.S = nullptr;
#if MB_ACTUATION
  b.sq = nullptr;
#endif
  if (e - P < (int64_t)P[3]) {  // [nun | r_coeff, damping, ncontact, 0 | 1 | 2 | 3] + records
    b.impulse = ((int)e[3] & 1) != 0;
    b.enable_force = ((int)e[3] & 2) != 0;
    b.nun = b.impulse ? b.nj : (int)e[0];
    b.r_coeff = b.impulse ? e[0] : 0.;
    b.damping = e[1];
    b.ncon = (int)e[2];
    b.K = e + 4;
    const double* r = b.K;
    for (int k = 0; k < b.ncon; ++k) {
      b.nc += (int)r[0] == C_CONTACT_3D ? 3 : 6;
      r += (int)r[3];
    }
#if MB_ACTUATION
    if (((int)e[3] & 4) != 0) {  // [20, 0, 0, 4 + nv nu] + S: tau = S u
      const bool sat = (int)r[1] == SQ_SMOOTH_SAT;  // [20, 1, 0, 4 + nv nu + 3 nu] + S + lb + ub + a: tau = S s(u)
      const int nu = ((int)r[3] - 4) / (sat ? b.nj + 3 : b.nj);
      b.nun = b.nj - nu;
      b.S = r + 4;
      if (sat) b.sq = b.S + (int64_t)b.nj * nu;
    }
#endif
  }
  return b;
}

// MB_BLK_UNIFORM (per kernel object, as MB_MFMA_SCALAR_SHAPE): the header parsed from the
// LDS-staged block is the same in every lane, but arrives in vector registers and stays live
// through the whole calc. parse_uniform moves every field into scalar registers (the first
// lane's value; doubles in two halves, the LDS pointers by their 32-bit LDS address, so they
// keep their address space). The host path is parse itself.
#ifndef MB_BLK_UNIFORM
#define MB_BLK_UNIFORM 0
#endif
#if MB_BLK_UNIFORM && defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ int mb_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bool mb_uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }
__device__ __forceinline__ double mb_uniform(double v) {
  int h[2];
  __builtin_memcpy(h, &v, 8);
  h[0] = __builtin_amdgcn_readfirstlane(h[0]);
  h[1] = __builtin_amdgcn_readfirstlane(h[1]);
  __builtin_memcpy(&v, h, 8);
  return v;
}
__device__ __forceinline__ Mask mb_uniform(Mask v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((Mask)hi << 32) | lo;
}
__device__ __forceinline__ const double* mb_uniform(const double* p) {
  typedef const __attribute__((address_space(3))) double* LdsP;
  const unsigned a = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(LdsP)p);
  return (const double*)(LdsP)(size_t)a;
}
#endif
// P: the block in LDS (device)
MB_HD __forceinline__ Blk parse_uniform(const double* P) {
  Blk b = parse(P);
#if MB_BLK_UNIFORM && defined(__HIP_DEVICE_COMPILE__)
  b.dt = mb_uniform(b.dt);
  b.nj = mb_uniform(b.nj);
  b.nq = mb_uniform(b.nq);
  b.nb = mb_uniform(b.nb);
  b.ff = mb_uniform(b.ff);
#if MB_PRISMATIC
  b.pris = mb_uniform(b.pris);
#endif
  b.ncost = mb_uniform(b.ncost);
  b.g = mb_uniform(b.g);
  b.arm = mb_uniform(b.arm);
  b.J = mb_uniform(b.J);
  b.C = mb_uniform(b.C);
  b.nun = mb_uniform(b.nun);
  b.S = b.S ? mb_uniform(b.S) : nullptr;
#if MB_ACTUATION
  b.sq = b.sq ? mb_uniform(b.sq) : nullptr;
#endif
  b.ncon = mb_uniform(b.ncon);
  b.nc = mb_uniform(b.nc);
  b.damping = mb_uniform(b.damping);
  b.K = mb_uniform(b.K);
  b.impulse = mb_uniform(b.impulse);
  b.r_coeff = mb_uniform(b.r_coeff);
  b.enable_force = mb_uniform(b.enable_force);
#endif
  return b;
}

}  // namespace mb
}  // namespace fddp
