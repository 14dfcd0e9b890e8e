// Test harness (CPU), beside mb_host.cpp: the entry points the impulse-cost tests need
// (tests/test_impulse_costs_host.py). The rollout's knot calc (knot_calc_dense_x, which
// evaluates CostModelImpulseCoM after v+), one block's check with the counts the launch plan
// takes from it, and the plan's impulse-CoM flag with the rollout variant it selects.
#include <cstdio>
#include <vector>

#include "../../crocoddyl_amd/csrc/multibody.hpp"
#include "../../crocoddyl_amd/csrc/launch_plan.hpp"

using namespace fddp::mb;

extern "C" {

// model->calc as the rollout runs it (the dense solve; mb_host_calc runs the tree-sparse one)
double mb_host_calc_dense(const double* P, int nx, const double* x, const double* u, int use_u, double* xnext) {
  const Blk b = parse(P);
  std::vector<double> w(calc_dense_doubles(b.nj, b.nc), 0.);
  return knot_calc_dense_x(HostExec{256}, P, nx, x, u, use_u != 0, xnext, w.data());
}

// launch_plan.hpp mb_block_check of one block: its size, or -1 with the reason in msg;
// out: nj, njac, nc, vcols, nu, nrows as the plan counts them
int64_t mb_host_block_check(const double* P, int64_t avail, int kind, int nx, int nu, int64_t* out, char* msg, int cap) {
  fddp::plan::Refusal why;
  int nj = 0, njac = 0, nc = 0, nuo = 0, nrows = 0;
  bool vc = false;
  const int64_t s = fddp::plan::mb_block_check(P, avail, kind, nx, nu, why, &nj, &njac, &nc, &vc, &nuo, &nrows);
  if (s < 0) return std::snprintf(msg, cap, "%s", why.str().c_str()), -1;
  const int64_t f[] = {nj, njac, nc, vc ? 1 : 0, nuo, nrows};
  for (int i = 0; i < 6; ++i) out[i] = f[i];
  return s;
}

// plan_lds / plan_variants of a knot sequence: out[0] LdsPlan::has_icom, out[1] the rollout
// variant (ktab::FWD_*). Returns 0, or 1 with the plan's refusal in msg.
int mb_host_plan_icom(const fddp_dims* d, const fddp_knot_desc* knots, const double* params, int64_t n_params,
                      const fddp::plan::Overrides* ov, const fddp::plan::DeviceFacts* facts, int* out, char* msg,
                      int cap) {
  const fddp::plan::LdsPlan l = fddp::plan::plan_lds(*d, knots, params, n_params, *ov);
  if (l.error) return std::snprintf(msg, cap, "%s", l.error), 1;
  out[0] = l.has_icom ? 1 : 0;
  out[1] = fddp::plan::plan_variants(l, *d, *ov, *facts).fwd;
  return 0;
}
}
