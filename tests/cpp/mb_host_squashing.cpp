// Test harness (CPU), beside mb_host_actuation.cpp: the entry points the squashed-actuation tests
// need (tests/test_squashing_host.py). The knot calc both ways (tree-sparse and the rollout's dense
// one), the calcDiff with its work area sized for the record's product (Kinv_atau S) and for s(u),
// ds/du, one block's check with what the launch plan takes from it, the device's own counts from
// the same block, the static check of the plans with the new area, and the plan's actuation flag
// with the variants it selects.
#include <cstdio>
#include <vector>

#include "../../crocoddyl_amd/csrc/multibody.hpp"
#include "../../crocoddyl_amd/csrc/launch_plan.hpp"

using namespace fddp::mb;

namespace {
struct Shape {
  int njac, nu, nrows;
  bool vc, act, sat;
};
// the counts the device derives from a block to lay out the calcDiff's LDS (knot_calc_diff_x)
Shape shape_of(const Blk& b) {
  Shape s;
  s.vc = false;
  s.njac = count_jac_costs(b, &s.vc);
  s.nu = b.nj - b.nun;
  s.nrows = count_cost_rows(b, s.nu);
  s.act = b.S != nullptr;
  s.sat = b.sq != nullptr;
  return s;
}
}  // namespace

extern "C" {

double sq_host_calc(const double* P, int nx, const double* x, const double* u, int use_u, double* xnext) {
  const Blk b = parse(P);
  std::vector<double> w(calc_work_doubles(b.nj, b.nc), 0.);
  return knot_calc_x(HostExec{256}, P, nx, x, u, use_u != 0, xnext, w.data());
}

double sq_host_calc_dense(const double* P, int nx, const double* x, const double* u, int use_u, double* xnext) {
  const Blk b = parse(P);
  std::vector<double> w(calc_dense_doubles(b.nj, b.nc), 0.);
  return knot_calc_dense_x(HostExec{256}, P, nx, x, u, use_u != 0, xnext, w.data());
}

// calcDiff under plan flags `spill` (< 0: the block's own, diff_spill at nu_max m) with nt lanes
void sq_host_calc_diff(const double* P, int nx, int m, int spill, int nt, const double* x, const double* u, int use_u,
                        double* Fx, double* Fu, double* Lxx, double* Lxu, double* Luu, double* Lx, double* Lu,
                        double* xnext, double* cost) {
  const Blk b = parse(P);
  const Shape s = shape_of(b);
  if (spill < 0) spill = diff_spill(b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, (int64_t)P[3], m, s.act, s.sat);
  std::vector<double> w(diff_layout(b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, spill, s.act, s.sat).htotal, 0.);
  knot_calc_diff_x(HostExec{nt}, P, nx, m, x, u, use_u != 0, w.data(), Fx, Fu, Lxx, Lxu, Luu, Lx, Lu, xnext, cost,
                   nullptr, spill);
}

// launch_plan.hpp mb_block_check of one block: its size, or -1 with the reason in msg; out: nj,
// njac, nc, vcols, nu, nrows, the actuation flag (2: squashed) as the plan counts them, then the
// doubles of the all-LDS calcDiff plan it budgets for the block
int64_t sq_host_block_check(const double* P, int64_t avail, int kind, int nx, int nu, int64_t* out, char* msg, int cap) {
  fddp::plan::Refusal why;
  int nj = 0, njac = 0, nc = 0, nuo = 0, nrows = 0;
  bool vc = false, act = false, pris = false, sat = false;
  const int64_t s = fddp::plan::mb_block_check(P, avail, kind, nx, nu, why, &nj, &njac, &nc, &vc, &nuo, &nrows, &act, &pris, &sat);
  if (s < 0) return std::snprintf(msg, cap, "%s", why.str().c_str()), -1;
  const int64_t f[] = {nj, njac, nc, vc ? 1 : 0, nuo, nrows, act ? (sat ? 2 : 1) : 0,
                       diff_layout(nj, njac, nc, vc, nuo, nrows, 0, act, sat).total};
  for (int i = 0; i < 8; ++i) out[i] = f[i];
  return s;
}

// the device's side of the same: out: nj, njac, nc, vcols, nu, nrows, the actuation flag, the
// doubles of its all-LDS plan, the offset and size of the Kinv_atau S area (-1, 0: none), then
// those of the s(u), ds/du area
void sq_host_device_counts(const double* P, int64_t* out) {
  const Blk b = parse(P);
  const Shape s = shape_of(b);
  const DiffLayout l = diff_layout(b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, 0, s.act, s.sat);
  const int64_t f[] = {b.nj, s.njac, b.nc, s.vc ? 1 : 0, s.nu, s.nrows, s.act ? (s.sat ? 2 : 1) : 0, l.total, l.KS, l.ksz, l.sq, l.sqsz};
  for (int i = 0; i < 12; ++i) out[i] = f[i];
}

// the static check of the block's calcDiff plan under flags `spill` (diff_layout_check): 0, or 1
// with the conflicting pair's names in msg
int sq_host_layout_check(const double* P, int spill, char* msg, int cap) {
  const Blk b = parse(P);
  const Shape s = shape_of(b);
  const DiffLayout l = diff_layout(b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, spill, s.act, s.sat);
  int i = 0, j = 0;
  if (!diff_layout_check(l, b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, &i, &j)) return 0;
  DiffRegion r[40];
  diff_layout_regions(l, b.nj, s.njac, b.nc, s.vc, s.nu, s.nrows, r);
  std::snprintf(msg, cap, "%s / %s", r[i].name, r[j].name);
  return 1;
}

// plan_lds / plan_variants of a knot sequence: out[0] LdsPlan::has_act, out[1] the rollout variant
// (ktab::FWD_*), out[2] the calcDiff variant (ktab::MB_*), out[3] LdsPlan::mbspill, out[4] the
// calcDiff kernel's dynamic LDS bytes. Returns 0, or 1 with the plan's refusal in msg.
int sq_host_plan(const fddp_dims* d, const fddp_knot_desc* knots, const double* params, int64_t n_params,
                  const fddp::plan::Overrides* ov, const fddp::plan::DeviceFacts* facts, int64_t* out, char* msg,
                  int cap) {
  const fddp::plan::LdsPlan l = fddp::plan::plan_lds(*d, knots, params, n_params, *ov);
  if (l.error) return std::snprintf(msg, cap, "%s", l.error), 1;
  const fddp::plan::VariantPlan v = fddp::plan::plan_variants(l, *d, *ov, *facts);
  out[0] = l.has_act ? 1 : 0;
  out[1] = v.fwd;
  out[2] = v.mb;
  out[3] = l.mbspill;
  out[4] = (int64_t)l.mb_diff_smem;
  return 0;
}
}
