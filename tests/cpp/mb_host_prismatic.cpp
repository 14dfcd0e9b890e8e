// Test harness (CPU), beside mb_host.cpp: the entry points the prismatic-joint tests need
// (tests/test_prismatic_host.py). The knot calc both ways (tree-sparse and the rollout's dense
// one), the calcDiff, the joint-space inertia and the bias forces of a block's tree as the device
// code forms them (for the closed-form pins), the parsed prismatic mask, one block's check, and
// the plan's prismatic flag with the variants and figures it selects.
// With -DMB_HOST_PRISMATIC_MAIN the file is a stand-alone program (a cart-pole block through
// every entry point), for a host sanitizer build.
#include <cstdio>
#include <vector>

#include "../../crocoddyl_amd/csrc/multibody.hpp"
#include "../../crocoddyl_amd/csrc/launch_plan.hpp"

using namespace fddp::mb;

namespace {
struct Shape {
  int njac, nu, nrows;
  bool vc, act;
};
Shape shape_of(const Blk& b) {
  Shape s;
  s.vc = false;
  s.njac = count_jac_costs(b, &s.vc);
  s.nu = b.nj - b.nun;
  s.nrows = count_cost_rows(b, s.nu);
  s.act = b.S != nullptr;
  return s;
}
}  // namespace

extern "C" {

double pris_host_calc(const double* P, int nx, const double* x, const double* u, int use_u, double* xnext) {
  const Blk b = parse(P);
  std::vector<double> w(calc_work_doubles(b.nj, b.nc), 0.);
  return knot_calc_x(HostExec{256}, P, nx, x, u, use_u != 0, xnext, w.data());
}

double pris_host_calc_dense(const double* P, int nx, const double* x, const double* u, int use_u, double* xnext) {
  const Blk b = parse(P);
  std::vector<double> w(calc_dense_doubles(b.nj, b.nc), 0.);
  return knot_calc_dense_x(HostExec{256}, P, nx, x, u, use_u != 0, xnext, w.data());
}

// calcDiff under plan flags `spill` (< 0: the block's own, diff_spill at nu_max m) with nt lanes
void pris_host_calc_diff(const double* P, int nx, int m, int spill, int nt, const double* x, const double* u, int use_u,
                         double* Fx, double* Fu, double* Lxx, double* Lxu, double* Luu, double* Lx, double* Lu,
                         double* xnext, double* cost) {
  const Blk b = parse(P);
  const Shape s = shape_of(b);
  if (spill < 0) spill = diff_spill(b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, (int64_t)P[3], m, s.act);
  std::vector<double> w(diff_layout(b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, spill, s.act).htotal, 0.);
  knot_calc_diff_x(HostExec{nt}, P, nx, m, x, u, use_u != 0, w.data(), Fx, Fu, Lxx, Lxu, Luu, Lx, Lu, xnext, cost,
                   nullptr, spill);
}

// M + diag(armature) (nv x nv, column-major) and nle = RNEA(q, v, 0) of the block's tree, by the
// device's world-frame recursions (world_kinematics with its CRBA columns, world_rnea)
void pris_host_m_nle(const double* P, const double* q, const double* v, double* M, double* nle) {
  const Blk b = parse(P);
  const int nj = b.nj;
  std::vector<double> w(WVals::doubles(nj) + part_doubles(nj), 0.);
  const WVals W{w.data(), nj, w.data() + WVals::doubles(nj)};
  for (int e = 0; e < nj * nj; ++e) M[e] = 0.;
  const HostExec ex{256};
  world_kinematics(ex, b, W, q, M, nj, [](int, int) {}, [](int, int) {});
  world_rnea(ex, b, W, v, nullptr, nle);
}

// the prismatic dofs as the device's parser sees them (Blk::pris)
uint64_t pris_host_mask(const double* P) { return parse(P).pris; }

// launch_plan.hpp mb_block_check of one block: its size, or -1 with the reason in msg; out: nj,
// njac, nc, nu, the prismatic flag as the plan counts them
int64_t pris_host_block_check(const double* P, int64_t avail, int kind, int nx, int nu, int64_t* out, char* msg, int cap) {
  fddp::plan::Refusal why;
  int nj = 0, njac = 0, nc = 0, nuo = 0, nrows = 0;
  bool vc = false, act = false, pris = false;
  const int64_t s =
      fddp::plan::mb_block_check(P, avail, kind, nx, nu, why, &nj, &njac, &nc, &vc, &nuo, &nrows, &act, &pris);
  if (s < 0) return std::snprintf(msg, cap, "%s", why.str().c_str()), -1;
  const int64_t f[] = {nj, njac, nc, nuo, pris ? 1 : 0};
  for (int i = 0; i < 5; ++i) out[i] = f[i];
  return s;
}

// plan_lds / plan_variants of a knot sequence: out[0] LdsPlan::has_pris, out[1] the rollout
// variant (ktab::FWD_*), out[2] the calcDiff variant (ktab::MB_*), out[3] LdsPlan::mbspill, out[4]
// the calcDiff kernel's dynamic LDS bytes, out[5] the all-LDS plan's bytes, out[6..8] the calc /
// rollout-calc / calcDiff work areas in doubles, out[9] the rollout's dynamic LDS bytes, out[10]
// the resident block's doubles. Returns 0, or 1 with the plan's refusal in msg.
int pris_host_plan(const fddp_dims* d, const fddp_knot_desc* knots, const double* params, int64_t n_params,
                   const fddp::plan::Overrides* ov, const fddp::plan::DeviceFacts* facts, int64_t* out, char* msg,
                   int cap) {
  const fddp::plan::LdsPlan l = fddp::plan::plan_lds(*d, knots, params, n_params, *ov);
  if (l.error) return std::snprintf(msg, cap, "%s", l.error), 1;
  const fddp::plan::VariantPlan v = fddp::plan::plan_variants(l, *d, *ov, *facts);
  const int64_t f[] = {l.has_pris ? 1 : 0, v.fwd, v.mb, l.mbspill, (int64_t)l.mb_diff_smem, l.mb_all_lds, l.mbw, l.mbw_fwd,
                       l.mbd, (int64_t)l.fwd_smem, l.pcap};
  for (int i = 0; i < 11; ++i) out[i] = f[i];
  return 0;
}
}

#ifdef MB_HOST_PRISMATIC_MAIN
// A cart-pole block (a prismatic cart along x, a revolute pole about y with a point mass at -l z,
// a state and a control cost, full actuation) through every entry point above.
int main() {
  const int nv = 2, nx = 4;
  std::vector<double> P = {1e-2, 2, 2, 0, /* gravity, armature */ 0, 0, -9.81, 0, 0};
  const double cart[27] = {2, -1, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0, 0, 0, 0, 0.02, 0.02, 0.02, 0, 0, 0};
  const double pole[27] = {0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0.3, 0, 0, -0.8, 0, 0, 0, 0, 0, 0};
  P.insert(P.end(), cart, cart + 27);
  P.insert(P.end(), pole, pole + 27);
  const double state_cost[] = {1, 1e-2, 0, 4 + nx + 2 * nv, 0, 0, 0, 0, 1, 1, 1, 1};
  const double control_cost[] = {2, 1e-2, 0, 4 + nv + nv, 0, 0, 1, 1};
  P.insert(P.end(), state_cost, state_cost + 12);
  P.insert(P.end(), control_cost, control_cost + 8);
  P[3] = (double)P.size();
  int64_t out[11];
  char msg[256] = "";
  if (pris_host_block_check(P.data(), (int64_t)P.size(), FDDP_KNOT_EULER_FREEFWD, nx, nv, out, msg, sizeof msg) < 0 ||
      out[4] != 1 || pris_host_mask(P.data()) != 1) {
    std::printf("block refused: %s\n", msg);
    return 1;
  }
  const double x[4] = {0.3, 0.7, -0.2, 0.5}, u[2] = {0.4, -0.1};
  double xa[4], xb[4], xc[4], cost, M[4], nle[2];
  const double ca = pris_host_calc(P.data(), nx, x, u, 1, xa), cb = pris_host_calc_dense(P.data(), nx, x, u, 1, xb);
  std::vector<double> Fx(16), Fu(8), Lxx(16), Lxu(8), Luu(4), Lx(4), Lu(2);
  for (int nt : {128, 256, 512})
    pris_host_calc_diff(P.data(), nx, nv, -1, nt, x, u, 1, Fx.data(), Fu.data(), Lxx.data(), Lxu.data(), Luu.data(),
                        Lx.data(), Lu.data(), xc, &cost);
  pris_host_m_nle(P.data(), x, x + 2, M, nle);
  const double mc = 1.0, mp = 0.3, l = 0.8, th = x[1], g = 9.81;
  const double want[6] = {mc + mp, -mp * l * std::cos(th), -mp * l * std::cos(th), mp * l * l,
                          mp * l * std::sin(th) * x[3] * x[3], mp * g * l * std::sin(th)};
  const double got[6] = {M[0], M[1], M[2], M[3], nle[0], nle[1]};
  double worst = std::fabs(ca - cb) + std::fabs(ca - cost);
  for (int e = 0; e < 4; ++e) worst = std::fmax(worst, std::fabs(xa[e] - xb[e]) + std::fabs(xa[e] - xc[e]));
  for (int e = 0; e < 6; ++e) worst = std::fmax(worst, std::fabs(got[e] - want[e]));
  std::printf("cart-pole: worst deviation %.3e\n", worst);
  return worst < 1e-12 ? 0 : 1;
}
#endif
