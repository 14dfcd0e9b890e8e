// Test harness (CPU), beside mb_host.cpp and mb_host_impulse.cpp: the entry points the
// centroidal-momentum tests need (tests/test_momentum_cost_host.py). The rollout's knot calc
// (knot_calc_dense_x, which evaluates the record beside the CRBA composites), one block's check
// with the counts the launch plan takes from it, the device's own counts from the same block,
// and the plan's momentum flag with the rollout variant it selects.
#include <cstdio>
#include <vector>

#include "../../crocoddyl_amd/csrc/multibody.hpp"
#include "../../crocoddyl_amd/csrc/launch_plan.hpp"

using namespace fddp::mb;

extern "C" {

// model->calc as the rollout runs it (the dense solve; mb_host_calc runs the tree-sparse one)
double mom_host_calc_dense(const double* P, int nx, const double* x, const double* u, int use_u, double* xnext) {
  const Blk b = parse(P);
  std::vector<double> w(calc_dense_doubles(b.nj, b.nc), 0.);
  return knot_calc_dense_x(HostExec{256}, P, nx, x, u, use_u != 0, xnext, w.data());
}

// launch_plan.hpp mb_block_check of one block: its size, or -1 with the reason in msg;
// out: nj, njac, nc, vcols, nu, nrows as the plan counts them
int64_t mom_host_block_check(const double* P, int64_t avail, int kind, int nx, int nu, int64_t* out, char* msg, int cap) {
  fddp::plan::Refusal why;
  int nj = 0, njac = 0, nc = 0, nuo = 0, nrows = 0;
  bool vc = false;
  const int64_t s = fddp::plan::mb_block_check(P, avail, kind, nx, nu, why, &nj, &njac, &nc, &vc, &nuo, &nrows);
  if (s < 0) return std::snprintf(msg, cap, "%s", why.str().c_str()), -1;
  const int64_t f[] = {nj, njac, nc, vc ? 1 : 0, nuo, nrows};
  for (int i = 0; i < 6; ++i) out[i] = f[i];
  return s;
}

// what the device derives from the block to lay out the calcDiff's LDS: out: njac, the
// velocity-column flag, the stacked residual rows, the residual size of record k (-1: none)
void mom_host_device_counts(const double* P, int nu, int k, int64_t* out) {
  const Blk b = parse(P);
  bool vc = false;
  out[0] = count_jac_costs(b, &vc);
  out[1] = vc ? 1 : 0;
  out[2] = count_cost_rows(b, nu);
  out[3] = -1;
  const double* cr = b.C;
  for (int i = 0; i < b.ncost; ++i) {
    const CRec C{cr};
    if (i == k) out[3] = jac_cost(b, C.type()) ? jac_rows(C.type()) : -1;
    cr += C.size();
  }
}

// plan_lds / plan_variants of a knot sequence: out[0] LdsPlan::has_hmom, out[1] the rollout
// variant (ktab::FWD_*), out[2] the calcDiff variant (ktab::MB_*), out[3] LdsPlan::mbspill.
// Returns 0, or 1 with the plan's refusal in msg.
int mom_host_plan(const fddp_dims* d, const fddp_knot_desc* knots, const double* params, int64_t n_params,
                  const fddp::plan::Overrides* ov, const fddp::plan::DeviceFacts* facts, int* out, char* msg, int cap) {
  const fddp::plan::LdsPlan l = fddp::plan::plan_lds(*d, knots, params, n_params, *ov);
  if (l.error) return std::snprintf(msg, cap, "%s", l.error), 1;
  const fddp::plan::VariantPlan v = fddp::plan::plan_variants(l, *d, *ov, *facts);
  out[0] = l.has_hmom ? 1 : 0;
  out[1] = v.fwd;
  out[2] = v.mb;
  out[3] = l.mbspill;
  return 0;
}
}
