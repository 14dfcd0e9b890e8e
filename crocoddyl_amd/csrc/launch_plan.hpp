// The launch plan of a handle: which kernel variant runs, with how much dynamic LDS, and
// how many line-search trials run together. Every dispatch threshold of libfddp_hip lives
// here, as plain data and free functions of (dims, knots, parameter pool, overrides, device
// facts): no HIP runtime call, no getenv, no global state, so the host tests
// (tests/cpp/mb_host.cpp mb_host_launch_plan) evaluate the rules the library runs.
// fddp_hip.hip apply_knots reads the overrides, calls plan_lds, uploads, sets the LDS
// attributes, gathers the device facts and calls plan_variants; the launchers and
// fddp_get_kernel_info read the plan.
#ifndef CROCODDYL_AMD_LAUNCH_PLAN_HPP_
#define CROCODDYL_AMD_LAUNCH_PLAN_HPP_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "fddp_kernels.hpp"
#include "fast_path.hpp"
#include "ktab.hpp"
#include "multibody.hpp"
#include "mb_quasistatic.hpp"

namespace fddp {
namespace plan {

// A workgroup's LDS bytes up to which one CU (160 KB) holds two / four workgroups
constexpr int64_t kLdsTwoPerCu = 80 * 1024, kLdsFourPerCu = 40 * 1024;

// The override variables (A/B runs, the variant tests), as fddp_hip.hip read_overrides
// parses them; the defaults are the "unset" values, under which the rules decide.
struct Overrides {
  int mb_w1 = -1;       // FDDP_MB_W1: 0 / 1 forces the 2- / 1-wave/EU calcDiff build
  int mb_nt = 0;        // FDDP_MB_NT: 128 / 256 / 512 forces the calcDiff workgroup size
  int mb_spill = -1;    // FDDP_MB_SPILL: 0 forces the all-LDS calcDiff plan (1: the rule; refused where it
                        // would spill a horizon that the spilled plan's kernel cannot run, has_pris)
  int fwd_mb_off = 0;   // FDDP_FWD_MB=0: the generic rollout on multibody horizons
  int fwd_mbw = 0;      // FDDP_FWD_MBW: 2 / 3 forces the rollout's waves/EU build
  int bwd_waves = 0;    // FDDP_BWD_WAVES: 1 / 4 / 8 waves per element of the MFMA sweep
  int bwd_generic = 0;  // FDDP_BACKWARD=generic: the VALU sweep
  int fast_off = 0;     // FDDP_FAST=0: no dense-knot fast path
  int ls_par = 0;       // CROCODDYL_AMD_LS_PAR in [1, 16] (read at create; 0: chosen per problem)
};

// What the rules need to know about the device and the compiled kernels, gathered by
// fddp_hip.hip after the LDS attributes are set. Rollout entries are indexed by ktab::FWD_*,
// sweep entries by bwd_slot(waves).
struct DeviceFacts {
  int cus = 0;                        // compute units
  int fwd_api[4] = {0, 0, 0, 0};      // occupancy API: workgroups per CU at LdsPlan::fwd_smem
  int fwd_static[4] = {0, 0, 0, 0};   // the kernel's static LDS bytes
  int bwd_code[3] = {0, 0, 0};        // ktab::backward_mfma_setup for 1 / 4 / 8 waves: variant code (< 0: none)
  int bwd_occ[3] = {0, 0, 0};         // ... and its workgroups per CU
};
inline int bwd_slot(int waves) { return waves == 1 ? 0 : (waves == 4 ? 1 : 2); }

// Everything apply_knots decides before its first HIP call.
struct LdsPlan {
  const char* error = nullptr;  // a refusal (FDDP_ERR_INVALID_ARG): the plan is not usable
  bool has_mb = false;          // multibody knots present (mb_knot_kernel)
  bool all_mb = false;          // every knot is a multibody knot
  bool has_icom = false;        // a knot carries a CostModelImpulseCoM record (no FWD_MB rollout)
  bool has_hmom = false;        // a knot carries a CostModelCentroidalMomentum record (no FWD_MB rollout)
  bool has_act = false;         // a knot carries an actuation record, tau = S u or S s(u) (no FWD_MB rollout, no spilled plan)
  bool has_pris = false;        // a knot's tree has a prismatic joint record (no FWD_MB rollout, no spilled plan)
  int mb_nj = 0;                // largest multibody tree (dofs)
  int64_t mbw = 0, mbw_fwd = 0, mbd = 0;  // Dev::mbw, mbw_fwd, mbd
  int mbspill = 0, dxv_mbw = 0;           // Dev::mbspill, dxv_mbw
  int64_t mb_all_lds = 0;       // bytes of the calcDiff's all-LDS plan (what the spill rule weighs)
  size_t mb_diff_smem = 0;      // dynamic LDS of mb_knot_kernel under the plan's flags
  int64_t qsw = 0;              // LDS doubles of the quasi-static knot's work area (0: no running multibody knot with controls)
  size_t qs_smem = 0;           // dynamic LDS of quasi_static_kernel: the work area, the state, the parameter block
  const char* qs_error = nullptr;  // why fddp_quasi_static is refused on these knots (the handle itself stands)
  int64_t pcap = 0;             // doubles of LDS reserved for a resident parameter block
  size_t fwd_smem = 0, calc_smem = 0, cdiff_smem = 0, fused_smem = 0, fwd_fast_smem = 0;
  bool fast = false;            // dense-knot fast path (fast_path.hpp) for calc / calcDiff / forward
  int npar = 1;                 // initial trial-group size of the line search
  bool npar_adapt = false;      // ... re-chosen after every solve (fddp_hip.hip choose_npar)
  bool uniform_nu = false;      // the MFMA sweep applies
  int ntl = 0, mtl = 0;         // its 16-tiles of ndx and nu_max
};

struct VariantPlan {
  int mb = -1;           // ktab::MB_* of the knot-parallel calc / calcDiff (-1: no multibody knots)
  int fwd = 0;           // ktab::FWD_* of the rollout
  int bwd = 0;           // 0 generic, else (NTL*10+MTL)*10+waves of the MFMA sweep
  double ls_slots = 0.;  // rollout workgroups resident on the device at once
};

struct LaunchPlan {
  Overrides ov;
  LdsPlan lds;
  VariantPlan var;
};

inline int64_t block_doubles(int kind, int nx, int nu) {
  switch (kind) {
    case FDDP_KNOT_LQR:
      return FDDP_PARAM_HEADER + 2LL * nx * nx + 2LL * nx * nu + (int64_t)nu * nu + 2LL * nx + nu;
    case FDDP_KNOT_UNICYCLE:
      return FDDP_PARAM_HEADER;
    case FDDP_KNOT_EULER_DIFFLQR: {
      const int64_t nq = nx / 2;
      return FDDP_PARAM_HEADER + 2 * nq * nq + nq * nu + nq + (int64_t)nx * nx + (int64_t)nx * nu +
             (int64_t)nu * nu + nx + nu;
    }
  }
  return -1;
}

// Why a parameter block is refused: a literal, and the number of an unknown record type.
struct Refusal {
  const char* text = nullptr;
  int type = -1;
  Refusal& operator=(const char* s) { return text = s, *this; }
  std::string str() const { return type < 0 ? std::string(text) : text + (" " + std::to_string(type)); }
};

// Checks one FDDP_KNOT_EULER_FREEFWD / _CONTACTFWD / FDDP_KNOT_IMPULSEFWD block
// (layouts in include/fddp_hip.h) against nx / nu and the space left in the
// pool. Returns its size in doubles, or -1 with `why` set. nj / njac / nc:
// dofs, jac costs and contact rows (LDS sizing).
inline int64_t mb_block_check(const double* P, int64_t avail, int kind, int nx, int nu, Refusal& why, int* nj_out,
                              int* njac_out, int* nc_out, bool* vcols_out = nullptr, int* nu_out = nullptr,
                              int* nrows_out = nullptr, bool* act_out = nullptr, bool* pris_out = nullptr,
                              bool* sat_out = nullptr) {
  using namespace fddp::mb;
  if (avail < FDDP_PARAM_HEADER) return why = "block out of range", -1;
  const double dt = P[0];
  const int nj = (int)P[1], ncost = (int)P[2];
  const int64_t size = (int64_t)P[3];
  if (!(dt >= 0.) || !std::isfinite(dt)) return why = "dt has positive value", -1;
  if ((double)nj != P[1] || nj < 1 || nj > kMaxJ) return why = "number of dofs out of [1, 64]", -1;
  if (size > avail || (double)size != P[3]) return why = "block out of range", -1;
  int64_t o = FDDP_PARAM_HEADER + 3 + nj;
  if (o + kJRec > size) return why = "block too small for its joints", -1;
  const bool ff = (int)P[o] == J_FREEFLYER;
  if (ff && nj < 6) return why = "a free-flyer root needs nv >= 6", -1;
  const int nb = ff ? nj - 5 : nj, nq = ff ? nj + 1 : nj;
  if (nx != nq + nj) return why = "multibody knots need nx = nq + nv", -1;
  const bool contact = kind == FDDP_KNOT_EULER_CONTACTFWD, impulse = kind == FDDP_KNOT_IMPULSEFWD;
  if (!contact && !impulse && (nu != nj || ff)) return why = "ActuationModelFull needs nu = nv and no free-flyer", -1;
  if (impulse && nu != 0) return why = "impulse knots have nu = 0", -1;
  if (impulse && dt != 0.) return why = "impulse blocks carry dt = 0 (no integrator)", -1;
  if ((double)ncost != P[2] || ncost < 0 || ncost > kMaxCosts) return why = "number of costs out of [0, 64]", -1;
  int force_rows = 0;  // rows the contact-force costs read
  bool pris = false;   // a prismatic joint record
  if (o + (int64_t)kJRec * nb > size) return why = "block too small for its joints", -1;
  for (int i = 0; i < nb; ++i) {
    const double* J = P + o + (int64_t)kJRec * i;
    const int type = (int)J[0], par = (int)J[1];
    if ((double)type != J[0] || (type != J_REVOLUTE && type != J_FREEFLYER && type != J_PRISMATIC))
      return why = "unknown joint type", -1;
    if (type == J_FREEFLYER && (i != 0 || par != -1)) return why = "a free-flyer may only be the root joint", -1;
    if ((double)par != J[1] || par < -1 || par >= i) return why = "joint parents must precede their children", -1;
    if (type == J_PRISMATIC) pris = true;
    if (type == J_REVOLUTE || type == J_PRISMATIC) {
      const double an = std::sqrt(J[2] * J[2] + J[3] * J[3] + J[4] * J[4]);
      if (!(std::fabs(an - 1.) < 1e-9)) return why = "joint axes must be unit vectors", -1;
    }
    if (!(J[17] >= 0.)) return why = "negative body mass", -1;
  }
  o += (int64_t)kJRec * nb;
  int njac = 0;
  bool vcols = false;
  for (int k = 0; k < ncost; ++k) {
    if (o + kCHdr > size) return why = "cost records out of range", -1;
    const double* C = P + o;
    const int type = (int)C[0];
    const int64_t rs = (int64_t)C[3];
    const int act = (int)C[2];
    if ((double)act != C[2] || act < A_QUAD || act > A_WEIGHTED_QUAD_BARRIER)
      return why = "unknown activation kind", -1;
    const int ap = act <= A_WEIGHTED_QUAD ? 1 : (act == A_QUAD_BARRIER ? 2 : 3);  // parameter rows per residual
    int64_t want = -1;
    if (type == C_STATE) want = kCHdr + nx + ap * 2 * nj;
    if (type == C_CONTROL) want = kCHdr + nu + ap * (int64_t)nu;
    if (type == C_FRAME_PLACEMENT) want = kCHdr + 25 + ap * 6;
    if (type == C_FRAME_TRANSLATION) want = kCHdr + 16 + ap * 3;
    if (type == C_FRAME_ROTATION) want = kCHdr + 22 + ap * 3;
    if (type == C_FRAME_VELOCITY) {
      if (impulse) return why = "frame-velocity costs are covered on Euler knots only", -1;
      want = kCHdr + 19 + ap * 6;
    }
    if (type == C_COM_POSITION) want = kCHdr + 3 + ap * 3;
    if (type == C_IMPULSE_COM) {  // empty payload: the activation parameters follow the header
      if (!impulse) return why = "the impulse CoM cost needs an impulse knot", -1;
      want = kCHdr + ap * 3;
    }
    if (type == C_CENTROIDAL_MOMENTUM) {  // [href(6)]; an impulse knot runs no kinematics at v
      if (impulse) return why = "centroidal-momentum costs are covered on Euler knots only", -1;
      want = kCHdr + 6 + ap * 6;
    }
    if (type == C_CONTACT_FORCE || type == C_FRICTION_CONE || type == C_COP_POSITION) {
      // [row0, nr, fref(6)] | [row0, nc, nr, A(3 nr)] | [row0, nc, nr, A(6 nr)]; rows checked against the
      // contacts below (on an impulse knot: against its impulses, whose multipliers the rows index)
      if (!contact && !impulse) return why = "force costs need contact knots", -1;
      if (o + kCHdr + 3 > size) return why = "cost records out of range", -1;
      const int row0 = (int)C[kCHdr];
      if ((double)row0 != C[kCHdr] || (row0 < 0 && row0 != kInactiveForceRow))
        return why = "contact-force cost row out of range", -1;
      if (type == C_CONTACT_FORCE) {
        const int nrf = (int)C[kCHdr + 1];
        if (nrf != 3 && nrf != 6) return why = "contact-force costs need a 3- or 6-row force", -1;
        want = kCHdr + 8 + ap * nrf;
        if (row0 >= 0) force_rows = std::max(force_rows, row0 + nrf);
      } else if (type == C_COP_POSITION) {
        const int ncc = (int)C[kCHdr + 1], nrc = (int)C[kCHdr + 2];
        if ((double)nrc != C[kCHdr + 2] || nrc < 1 || nrc > 6) return why = "CoP support rows out of [1, 6]", -1;
        if (row0 >= 0 && ncc != 6)
          return why = impulse ? "CoP position cost on an impulse of 6 rows" : "CoP position cost on a contact of 6 rows", -1;
        want = kCHdr + 3 + 6 * nrc + ap * nrc;
        if (row0 >= 0) force_rows = std::max(force_rows, row0 + ncc);
      } else {
        const int ncc = (int)C[kCHdr + 1], nrc = (int)C[kCHdr + 2];
        if ((double)nrc != C[kCHdr + 2] || nrc < 1 || nrc > 6) return why = "friction cone rows out of [1, 6]", -1;
        if (row0 >= 0 && ncc != 3 && ncc != 6) return why = "friction cone on a contact of 3 or 6 rows", -1;
        want = kCHdr + 3 + 3 * nrc + ap * nrc;
        if (row0 >= 0) force_rows = std::max(force_rows, row0 + ncc);
      }
    }
    if (want < 0) return why = "unknown cost type", why.type = type, -1;
    if (rs != want || o + rs > size) return why = "cost record of the wrong size", -1;
    if (type == C_FRAME_PLACEMENT || type == C_FRAME_TRANSLATION || type == C_FRAME_VELOCITY ||
        type == C_FRAME_ROTATION) {
      const int fj = (int)C[kCHdr];
      if ((double)fj != C[kCHdr] || fj < 0 || fj >= nb) return why = "frame attached to an unknown joint", -1;
    }
    if (type == C_STATE && ff)  // the reference state's free-flyer pose must be finite
      for (int e = 0; e < 7; ++e)
        if (!std::isfinite(C[kCHdr + e])) return why = "non-finite reference state", -1;
    if (type == C_FRAME_PLACEMENT || type == C_FRAME_TRANSLATION || type == C_COM_POSITION ||
        type == C_FRAME_VELOCITY || type == C_FRAME_ROTATION || type == C_IMPULSE_COM ||
        type == C_CENTROIDAL_MOMENTUM || (type == C_STATE && ff))
      ++njac;
    if (type == C_FRAME_VELOCITY || type == C_CENTROIDAL_MOMENTUM) vcols = true;
    o += rs;
  }
  int nc = 0;
  bool act = false;  // flag bit 4: an actuation record after the contacts
  bool sat = false;  // ... whose header slot 1 is SQ_SMOOTH_SAT: tau = S s(u)
  std::vector<std::pair<int, int>> crow;  // (row0, rows) of every contact record
  if (contact || impulse) {  // [nun | r_coeff, damping, ncontact, 0 | 2 | 4 | 6 (contact), 1 | 3 (impulse)] + records
    if (o + 4 > size) return why = "contact section out of range", -1;
    const int nun = (int)P[o], ncon = (int)P[o + 2];
    const double damping = P[o + 1];
    if (impulse && (P[o + 3] == 5. || P[o + 3] == 7.)) return why = "impulse knots take no actuation record (nu = 0)", -1;
    if (impulse ? (P[o + 3] != 1. && P[o + 3] != 3.)
                : (P[o + 3] != 0. && P[o + 3] != 2. && P[o + 3] != 4. && P[o + 3] != 6.))
      return why = "contact / impulse section flag does not match the kind", -1;
    act = contact && ((int)P[o + 3] & 4) != 0;
    if (impulse) {
      if (!(P[o] >= 0.) || !std::isfinite(P[o])) return why = "The restitution coefficient has to be positive", -1;
    } else if (act) {
      if (P[o] != 0.) return why = "an actuation record needs nun = 0 in the section header", -1;
      if (nu < 1 || nu > nj) return why = "actuation record: nu out of [1, nv]", -1;
    } else {
      if ((double)nun != P[o] || nun < 0 || nun >= nj) return why = "unactuated dofs out of [0, nv)", -1;
      if (ff && nun != 6) return why = "ActuationModelFloatingBase on a free-flyer leaves 6 dofs unactuated", -1;
      if (nu != nj - nun) return why = "ActuationModelFloatingBase needs nu = nv - nun", -1;
    }
    if (!(damping >= 0.) || !std::isfinite(damping)) return why = "The damping factor has to be positive", -1;
    if ((double)ncon != P[o + 2] || ncon < 0) return why = "negative number of contacts", -1;
    o += 4;
    for (int k = 0; k < ncon; ++k) {
      if (o + kCHdr + 1 > size) return why = "contact records out of range", -1;
      const double* C = P + o;
      const int type = (int)C[0];
      const int64_t rs = (int64_t)C[3];
      int64_t want = -1;
      if (type == C_CONTACT_3D) want = kCHdr + (impulse ? 13 : 16);
      if (type == C_CONTACT_6D) want = kCHdr + (impulse ? 13 : 25);
      if (want < 0) return why = "unknown contact type", why.type = type, -1;
      if (rs != want || o + rs > size) return why = "contact record of the wrong size", -1;
      const int fj = (int)C[kCHdr];
      if ((double)fj != C[kCHdr] || fj < 0 || fj >= nb) return why = "contact frame attached to an unknown joint", -1;
      if (!std::isfinite(C[1]) || !std::isfinite(C[2])) return why = "non-finite contact gains", -1;
      const int rows = type == C_CONTACT_3D ? 3 : 6;
      crow.emplace_back(nc, rows);
      nc += rows;
      o += rs;
    }
    if (nc > kMaxNc) return why = "more than 24 contact rows in one knot", -1;
    if (act) {  // [20, 0, 0, 4 + nv nu] + S (nv x nu, column-major): tau = S u
                // [20, 1, 0, 4 + nv nu + 3 nu] + S + lb(nu) + ub(nu) + a(nu): tau = S s(u), smooth-sat
      if (o + kCHdr > size) return why = "block ends before its actuation record", -1;
      const double* A = P + o;
      if (A[0] != (double)C_ACTUATION) return why = "actuation record of the wrong type", -1;
      if (A[1] != (double)SQ_NONE && A[1] != (double)SQ_SMOOTH_SAT)
        return why = "actuation record with an unknown squashing kind", -1;
      sat = A[1] == (double)SQ_SMOOTH_SAT;
      const int64_t want = kCHdr + (int64_t)nj * nu + (sat ? 3 * (int64_t)nu : 0);
      if (A[3] != (double)want) return why = "actuation record of the wrong size", -1;
      if (o + want > size) return why = "block ends before its actuation record", -1;
      for (int64_t e = 0; e < (int64_t)nj * nu; ++e)
        if (!std::isfinite(A[kCHdr + e])) return why = "non-finite entry in the actuation matrix", -1;
      if (sat) {
        const double* lb = A + kCHdr + (int64_t)nj * nu;
        const double *ub = lb + nu, *a = ub + nu;
        for (int c = 0; c < 3 * nu; ++c)
          if (!std::isfinite(lb[c])) return why = "non-finite squashing bound or smoothing term", -1;
        for (int c = 0; c < nu; ++c)
          if (lb[c] >= ub[c]) return why = "squashing bounds need lb < ub", -1;
        // (a = (smooth (ub - lb))^2; at a = 0, ds/du is 0/0 on a bound)
        for (int c = 0; c < nu; ++c)
          if (!(a[c] > 0.)) return why = "squashing needs a positive smoothing term (smooth > 0)", -1;
      }
      o += want;
    }
  }
  if (force_rows > nc)
    return why = impulse ? "impulse cost reads rows beyond the impulses" : "contact-force cost reads rows beyond the contacts", -1;
  if (force_rows > 0) {  // each contact-force cost reads exactly one contact of its size
    int64_t oc = FDDP_PARAM_HEADER + 3 + nj + (int64_t)kJRec * nb;
    for (int k = 0; k < ncost; ++k) {
      const double* C = P + oc;
      if (((int)C[0] == C_CONTACT_FORCE || (int)C[0] == C_FRICTION_CONE || (int)C[0] == C_COP_POSITION) &&
          (int)C[kCHdr] >= 0) {
        bool hit = false;
        for (const auto& r : crow) hit = hit || (r.first == (int)C[kCHdr] && r.second == (int)C[kCHdr + 1]);
        if (!hit) return why = "a force cost must read one whole contact of its size", -1;
      }
      oc += (int64_t)C[3];
    }
  }
  if (o != size) return why = "block size does not match its records", -1;
  if (njac > kMaxJacCosts) return why = "more than 8 frame / CoM / frame-velocity / free-flyer state costs in one knot", -1;
  const int nrows = count_cost_rows(parse(P), nu);
  if (nrows > kMaxCostRows) return why = "more than 64 cost residual rows with dense Jacobians in one knot", -1;
  if ((pad2(diff_layout(nj, njac, nc, vcols, nu, nrows, 0, act, sat).total) + pad2(size)) * 8 > 160 * 1024)
    return why = "too many dofs for the calcDiff LDS plan", -1;
  if (nj_out) *nj_out = std::max(*nj_out, nj);
  if (njac_out) *njac_out = std::max(*njac_out, njac);
  if (nc_out) *nc_out = std::max(*nc_out, nc);
  if (vcols_out) *vcols_out = *vcols_out || vcols;
  if (nu_out) *nu_out = std::max(*nu_out, nu);
  if (nrows_out) *nrows_out = std::max(*nrows_out, nrows);
  if (act_out) *act_out = *act_out || act;
  if (pris_out) *pris_out = *pris_out || pris;
  if (sat_out) *sat_out = *sat_out || sat;
  return size;
}

// The LDS plans, the fast-path choice and the initial trial-group size of a knot sequence
// (validated by fddp_hip.hip check_knots, which refuses a bad block before the library
// plans; a host caller that plans unchecked knots gets the first block refusal's text as
// the plan's error, unless the plan itself is refused first).
inline LdsPlan plan_lds(const fddp_dims& d, const fddp_knot_desc* knots, const double* params, int64_t n_params,
                        const Overrides& ov) {
  using ktab::kNT;
  LdsPlan p;
  const int64_t sX = pad2(d.nx), sN = pad2(d.ndx), sM = pad2(d.nu_max > 0 ? d.nu_max : 1);
  int64_t pmax = 0;
  int64_t mb_pmax = 0;  // largest multibody parameter block (staged in LDS by mb_knot_kernel)
  int mb_nj = 0, mb_njac = 0, mb_nc = 0;
  bool mb_vcols = false, mb_act = false;
  int mb_nu = 0, mb_nrows = 0;
  // each multibody block's own shape: the device lays out a knot's calcDiff LDS from its
  // own block, so the plan to allocate is the largest knot's, not the plan of the largest
  // value of every parameter (on the Solo12 trot those come from different knots: 82.2 KB,
  // one workgroup per CU, against the largest knot's 79.6 KB)
  struct MbShape {
    int nj, njac, nc, nu, nrows;
    bool vcols, act, sat;
  };
  std::vector<MbShape> shapes;
  const char* refused = nullptr;  // the first block refusal
  p.all_mb = true;
  for (int t = 0; t <= d.T; ++t) {
    int64_t sz;
    if (is_mb_kind(knots[t].kind)) {
      p.has_mb = true;
      sz = 0;
      const int nb = knots[t].param_stride > 0 ? d.B : 1;
      for (int b = 0; b < nb; ++b) {
        const int64_t off = knots[t].param_offset + (int64_t)b * knots[t].param_stride;
        Refusal why;
        MbShape k{0, 0, 0, 0, 0, false, false, false};
        bool pris = false;
        const int64_t s1 = mb_block_check(params + off, n_params - off, knots[t].kind, d.nx, knots[t].nu, why, &k.nj,
                                          &k.njac, &k.nc, &k.vcols, &k.nu, &k.nrows, &k.act, &pris, &k.sat);
        if (s1 < 0 && !refused) refused = why.text;
        if (s1 >= 0 && fddp::mb::has_impulse_com(fddp::mb::parse(params + off))) p.has_icom = true;
        if (s1 >= 0 && fddp::mb::has_momentum(fddp::mb::parse(params + off))) p.has_hmom = true;
        if (s1 >= 0 && k.act) p.has_act = true;
        if (s1 >= 0 && pris) p.has_pris = true;
        // (a refused block is planned with its size field, as mb_pmax is: the budget below
        // then refuses only what is over it)
        const int64_t own = (int64_t)params[off + 3];
        sz = std::max(sz, s1 < 0 ? own : s1);
        mb_pmax = std::max<int64_t>(mb_pmax, own);
        mb_nj = std::max(mb_nj, k.nj);
        mb_njac = std::max(mb_njac, k.njac);
        mb_nc = std::max(mb_nc, k.nc);
        mb_vcols = mb_vcols || k.vcols;
        mb_act = mb_act || k.act;
        mb_nu = std::max(mb_nu, k.nu);
        mb_nrows = std::max(mb_nrows, k.nrows);
        if (s1 >= 0 && t < d.T && knots[t].kind != FDDP_KNOT_IMPULSEFWD && k.nu > 0)
          p.qsw = std::max<int64_t>(p.qsw, pad2(fddp::mb::quasi_static_work_doubles(k.nj, k.nc, k.nu)));
        bool seen = false;
        for (const MbShape& q : shapes)
          seen = seen || (q.nj == k.nj && q.njac == k.njac && q.nc == k.nc && q.nu == k.nu && q.nrows == k.nrows &&
                          q.vcols == k.vcols && q.act == k.act && q.sat == k.sat);
        if (!seen) shapes.push_back(k);
      }
    } else {
      p.all_mb = false;
      sz = block_doubles(knots[t].kind, d.nx, knots[t].nu);
    }
    pmax = std::max<int64_t>(pmax, sz);
  }
  p.mbw = p.has_mb ? pad2(fddp::mb::calc_work_doubles(mb_nj, mb_nc)) : 0;
  p.mbw_fwd = p.has_mb ? pad2(fddp::mb::calc_dense_doubles(mb_nj, mb_nc)) : 0;
  p.mb_nj = mb_nj;
  // parallel line-search trials: they pay on the large trees (C5 Talos, nv = 38:
  // forward -12 %), where one rollout keeps a CU busy longest; on small ones (C4
  // Solo12, nv = 18) the extra trials cost more than the shorter chains save
  p.npar = ov.ls_par ? ov.ls_par : (p.has_mb && mb_nj >= 24 ? 4 : 1);
  p.npar_adapt = !ov.ls_par && p.has_mb;
  // the calcDiff's LDS plan: spilled to the output blocks where the all-LDS plan would
  // leave room for one workgroup per CU only (multibody.hpp diff_spill; FDDP_MB_SPILL=0
  // forces the all-LDS plan, for A/B runs)
  auto plan_doubles = [&](int spill) {  // the largest knot's plan under spill flags `spill`
    int64_t mx = 0;
    for (const MbShape& q : shapes)
      mx = std::max<int64_t>(
          mx, pad2(fddp::mb::diff_layout(q.nj, q.njac, q.nc, q.vcols, q.nu, q.nrows, spill, q.act, q.sat).total));
    return mx;
  };
  p.mb_all_lds = p.has_mb ? (plan_doubles(0) + pad2(mb_pmax)) * 8 : 0;
  // (the spill flags themselves from the largest value of every parameter: the spilled
  // arrays must fit their output blocks on every knot)
  // (a horizon with an actuation record never spills: the spilled plan's kernel is built without
  // the record's phases, MB_ACTUATION in k_mb.hip; every accepted block fits the all-LDS plan;
  // nor does a horizon with a prismatic joint record, MB_PRISMATIC there)
  p.mbspill = p.has_mb && !mb_act && !p.has_pris && ov.mb_spill != 0 && p.mb_all_lds > kLdsTwoPerCu
                  ? fddp::mb::diff_spill(mb_nj, mb_njac, mb_nc, mb_vcols, mb_nu, mb_nrows, mb_pmax, d.nu_max, mb_act)
                  : 0;
  p.mbd = p.has_mb ? plan_doubles(p.mbspill) : 0;
  p.mb_diff_smem = p.has_mb ? sizeof(double) * (p.mbd + pad2(mb_pmax)) : 0;
  p.qs_smem = p.qsw ? sizeof(double) * (p.qsw + pad2(d.nx) + pad2(mb_pmax)) : 0;
  if (p.qs_smem > 160 * 1024) p.qs_error = "the quasi-static knot's work area and parameter block exceed the CU's LDS";
  const int64_t budget = (150 * 1024) / 8 - (2 * sX + sM + 2 * sN + 5 * (kNT / kWave) + 16) - p.mbw;
  // LDS-staged parameter blocks up to pcap doubles; larger (dense) blocks are read from
  // global memory. The multibody calc reads its block from LDS only (knots.hpp), so
  // pcap covers at least the largest multibody block.
  p.pcap = pmax <= budget ? pad2(pmax) : (pad2(mb_pmax) <= budget ? pad2(mb_pmax) : 0);
  if (p.has_mb && p.pcap < pad2(mb_pmax)) {
    p.error = "multibody parameter blocks exceed the LDS budget of the calc / rollout kernels";
    return p;
  }
  // (dx in the tail of the calc's scratch when the gains' K staging leaves room: on the C5 walk
  // that takes the rollout's LDS to 52.6 KB, three workgroups per CU; the LDS is allocated in
  // 2 KB granules (measured: tools/occ_probe.hip), which the occupancy API does not model)
  p.dxv_mbw = p.mbw_fwd >= (int64_t)d.nu_max * d.ndx + 2 * sN ? 1 : 0;
  p.fwd_smem = sizeof(double) * (p.pcap + fwd_lds_doubles<kNT, false>(sX, sN, sM) - (p.dxv_mbw ? 2 * sN : 0) + p.mbw_fwd);
  p.calc_smem = sizeof(double) * (p.pcap + 2 * sX + sM + 5 * (kNT / kWave) + 16 + p.mbw);
  p.cdiff_smem = sizeof(double) * (p.pcap + sX + sM);
  {  // dense-knot fast path: every knot LQR / Euler∘DiffLQR, block LDS-resident
    bool dense = p.pcap > 0 && d.nx == d.ndx && d.nx <= kNT && d.nu_max <= kNT;
    for (int t = 0; t <= d.T; ++t)
      dense = dense && (knots[t].kind == FDDP_KNOT_LQR || knots[t].kind == FDDP_KNOT_EULER_DIFFLQR);
    p.fused_smem = sizeof(double) * (p.pcap + calc_tiled_lds(sX, sM));
    p.fwd_fast_smem = sizeof(double) * (p.pcap + fwd_lds_doubles<kNT, true>(sX, sN, sM));
    p.fast = dense && !ov.fast_off && p.fused_smem <= 160 * 1024 && p.fwd_fast_smem <= 160 * 1024;
  }
  // backward sweep: MFMA tiles when every running knot has nu == nu_max, or on multibody
  // horizons (their calcDiff zero-fills the Fu columns beyond a knot's nu, so the sweep
  // runs a knot on its own nu: the impulse knots of the gaits)
  p.uniform_nu = d.nu_max > 0;
  for (int t = 0; t < d.T; ++t) p.uniform_nu = p.uniform_nu && knots[t].nu == d.nu_max;
  p.uniform_nu = p.uniform_nu || (p.all_mb && d.nu_max > 0);
  p.ntl = (d.ndx + 15) / 16;
  p.mtl = (d.nu_max + 15) / 16;
  if (refused) p.error = refused;
  if (!p.error && p.has_icom && ov.fwd_mbw == 3)
    p.error = "FDDP_FWD_MBW=3 on a horizon with an impulse CoM cost: that rollout build does not evaluate it";
  if (!p.error && p.has_hmom && ov.fwd_mbw == 3)
    p.error = "FDDP_FWD_MBW=3 on a horizon with a centroidal-momentum cost: that rollout build does not evaluate it";
  if (!p.error && p.has_act && ov.fwd_mbw == 3)
    p.error = "FDDP_FWD_MBW=3 on a horizon with an actuation record: that rollout build does not evaluate it";
  if (!p.error && p.has_pris && ov.fwd_mbw == 3)
    p.error = "FDDP_FWD_MBW=3 on a horizon with a prismatic joint: that rollout build does not read the joint type";
  // (asked for by name where the rule would spill: the small plans, which never spill, pass)
  if (!p.error && p.has_pris && ov.mb_spill > 0 && p.mb_all_lds > kLdsTwoPerCu)
    p.error = "FDDP_MB_SPILL=1 on a horizon with a prismatic joint: the spilled-plan calcDiff build does not read the joint type";
  return p;
}

// Workgroups of a kernel one CU holds at once: the occupancy API's answer, capped by the
// LDS (dynamic + static bytes) allocated in 2 KB granules (measured on gfx950,
// tools/occ_probe.hip: 53,248 B per workgroup fit three per CU, 53,776 B two, where the API
// still says three).
inline int resident_per_cu(int api, size_t dyn_bytes, size_t static_bytes) {
  const size_t g = 2048, lds = ((dyn_bytes + static_bytes + g - 1) / g) * g;
  const int by_lds = lds > 0 ? (int)((160 * 1024) / lds) : api;
  return std::max(1, std::min(api, by_lds));
}

// The kernel variants of a plan on a device.
inline VariantPlan plan_variants(const LdsPlan& l, const fddp_dims& d, const Overrides& ov, const DeviceFacts& f) {
  VariantPlan v;
  if (l.has_mb) {
    // The knot-parallel kernel's LDS plan leaves room for one workgroup per CU: take the
    // 1-wave/EU build (no spills; FDDP_MB_W1=0 forces the 2-wave one, for A/B runs).
    const bool one_per_cu = ov.mb_w1 >= 0 ? ov.mb_w1 == 1 : (int64_t)l.mb_diff_smem > kLdsTwoPerCu;
    // 512-thread (8-wave) workgroups for the one-per-CU plans: two waves per SIMD where the
    // 256-thread plan has one (C5 calcDiff 66 -> 59 ms); FDDP_MB_NT=256 / 512 forces
    const bool x8 = ov.mb_nt ? ov.mb_nt == 512 : one_per_cu;
    // 128-thread (2-wave) workgroups for the small trees whose LDS plan fits four per CU
    const bool x2 = ov.mb_nt ? ov.mb_nt == 128 : (l.mb_nj <= 16 && (int64_t)l.mb_diff_smem <= kLdsFourPerCu);
    v.mb = l.mbspill ? ktab::MB_S2 : x2 ? ktab::MB_X2 : (x8 ? ktab::MB_X8 : (one_per_cu ? ktab::MB_W1 : ktab::MB_W2));
  }
  const int cus = std::max(1, f.cus);
  // The rollout variant: the generic one for mixed horizons (FDDP_FWD_MB=0 selects it on
  // multibody-only ones, for A/B runs); for multibody-only horizons the variant with only the
  // multibody calc compiled in: the three-workgroups-per-CU build (168 VGPRs, spills) when its
  // LDS allows three per CU and the batch needs more than two per CU, else the 256-VGPR build
  // (FDDP_FWD_MBW=2|3 forces one).
  if (l.fast) {
    v.fwd = ktab::FWD_FAST;
  } else if (!(l.all_mb && !ov.fwd_mb_off)) {
    v.fwd = ktab::FWD_GENERIC;
  } else {
    const bool three = resident_per_cu(f.fwd_api[ktab::FWD_MB], l.fwd_smem, f.fwd_static[ktab::FWD_MB]) >= 3;
    // (a horizon with an impulse CoM or a centroidal-momentum cost, an actuation record or a
    // prismatic joint never: that build's calc has no code for them, MB_CALC_IMPULSE_COM /
    // MB_CALC_MOMENTUM / MB_ACTUATION / MB_PRISMATIC; plan_lds refuses the override that would force it)
    const bool take3 = !l.has_icom && !l.has_hmom && !l.has_act && !l.has_pris && (ov.fwd_mbw ? ov.fwd_mbw == 3 : (three && d.B > 2 * cus));
    v.fwd = take3 ? ktab::FWD_MB : ktab::FWD_MB2;
  }
  if (!l.fast) v.ls_slots = (double)cus * resident_per_cu(f.fwd_api[v.fwd], l.fwd_smem, f.fwd_static[v.fwd]);
  int bwd = -1;
  if (l.uniform_nu && !ov.bwd_generic) {
    // eight waves per element, the fastest knot (measured round 4: one wave (C3) or four
    // (C2) per element are slower, 12.1 / 1.06 ms against 3.6 / 0.89 ms), unless the
    // four-wave plan keeps more elements resident: the sweep is a serial chain per
    // element, so its time goes with the rounds of resident workgroups, ceil(B / slots),
    // and a four-wave knot takes ~1.15x an eight-wave one (C3, B = 512 on 256 CUs: two
    // four-wave workgroups per CU, one round, 3.20 -> 2.16 ms; C4 and C2 keep eight).
    // FDDP_BWD_WAVES=1|4|8 overrides.
    int nw = ov.bwd_waves ? ov.bwd_waves : 8;
    // one-wave plans exist for the small shapes (NTL + MTL <= 4, MTL = 1); four-wave
    // plans where C^T has its own LDS area (else C^T over Zu needs the 8-wave plan's
    // late LDS-DMA); everything else runs eight waves (ktab::backward_mfma_setup)
    const int ntl = l.ntl, mtl = l.mtl;
    const bool known = (ntl == 5 && mtl == 2) || (mtl == 1 && ntl >= 1 && ntl <= 3);
    if (known) {
      if (nw == 1 && !(ntl + mtl <= 4 && mtl == 1)) nw = 8;
      if (f.bwd_code[bwd_slot(nw)] < 0 && nw == 4) nw = 8;
      bwd = f.bwd_code[bwd_slot(nw)];
      const int occ = f.bwd_occ[bwd_slot(nw)], v4 = f.bwd_code[bwd_slot(4)], occ4 = f.bwd_occ[bwd_slot(4)];
      if (!ov.bwd_waves && bwd > 0 && mtl == 1 && v4 > 0 && f.cus > 0 && occ > 0 && occ4 > 0) {
        const int64_t r8 = (d.B + (int64_t)f.cus * occ - 1) / ((int64_t)f.cus * occ);
        const int64_t r4 = (d.B + (int64_t)f.cus * occ4 - 1) / ((int64_t)f.cus * occ4);
        if (1.2 * (double)r4 < (double)r8) bwd = v4;
      }
    }
  }
  v.bwd = bwd > 0 ? bwd : 0;
  return v;
}

// The rollout variant a launch takes under the handle's solver kind (fddp_set_solver_kind
// switches kinds on a live handle, so this is asked at every launch, not planned): the
// three-workgroups-per-CU multibody build has no DDP mode compiled in (fddp_kernels.hpp
// FDDP_FWD_DDP_MB3), so a DDP / BoxDDP handle planned onto it rolls out with the
// two-workgroup build, which takes the same dynamic LDS. Every other variant has the mode.
inline int rollout_for_kind(int fwd, int solver_kind) {
  const bool ddp = solver_kind == FDDP_SOLVER_DDP || solver_kind == FDDP_SOLVER_BOXDDP;
  return ddp && fwd == ktab::FWD_MB && !FDDP_FWD_DDP_MB3 ? ktab::FWD_MB2 : fwd;
}

}  // namespace plan
}  // namespace fddp

#endif  // CROCODDYL_AMD_LAUNCH_PLAN_HPP_
