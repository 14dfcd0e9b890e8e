// SolverDDP's getters through the C++ facade without set_debug (tests/test_getters_facade_gpu.py):
// get_Vxx, get_Vx, get_Qxx, get_Qxu, get_Quu, get_Qx, get_Qu right after computeDirection(), as
// the reference's binding test reads them, against the C ABI's values of the same handle and
// against a second solver that ran in debug mode; SolverBoxFDDP::get_Quu_inv after a solve.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "crocoddyl_amd/solver_fddp_hip.hpp"

namespace croc = crocoddyl_amd;

static int compare(const char* name, const std::vector<croc::VectorXd>& got, fddp_handle* h, int which, int nk,
                   size_t per, bool want_nonzero) {
  std::vector<double> abi((size_t)nk * per, 0.);
  if (fddp_get_quantity(h, which, abi.data()) != FDDP_OK) {
    std::printf("%s: fddp_get_quantity: %s\n", name, fddp_last_error());
    return 1;
  }
  if ((int)got.size() != nk) {
    std::printf("%s: %zu knots for %d\n", name, got.size(), nk);
    return 1;
  }
  bool any = false;
  for (int t = 0; t < nk; ++t) {
    if (got[t].size() != per || std::memcmp(got[t].data(), abi.data() + (size_t)t * per, sizeof(double) * per)) {
      std::printf("%s: knot %d differs from the C ABI's\n", name, t);
      return 1;
    }
    for (double v : got[t]) any = any || v != 0.;
  }
  if (want_nonzero && !any) {
    std::printf("%s: all zero\n", name);
    return 1;
  }
  std::printf("%s ok\n", name);
  return 0;
}

static int same(const char* name, const std::vector<croc::VectorXd>& a, const std::vector<croc::VectorXd>& b) {
  if (a.size() != b.size()) return 1;
  for (size_t t = 0; t < a.size(); ++t)
    if (a[t].size() != b[t].size() || std::memcmp(a[t].data(), b[t].data(), sizeof(double) * a[t].size())) {
      std::printf("%s: knot %zu differs from the debug solver's\n", name, t);
      return 1;
    }
  return 0;
}

int main() {
  try {
    const int T = 10, n = 24, m = 12;
    auto model = std::make_shared<croc::ActionModelLQR>(n, m, false);
    std::vector<std::shared_ptr<croc::ActionModelBase> > running(T, model);
    croc::VectorXd x0(n, 0.);
    for (int i = 0; i < n; ++i) x0[i] = -1. + 2. * i / (n - 1);
    auto problem = std::make_shared<croc::ShootingProblem>(x0, running, model);
    croc::SolverFDDP solver(problem), dbg(problem);
    dbg.set_debug(true);
    const std::vector<croc::VectorXd> none;
    for (croc::SolverFDDP* s : {&solver, &dbg}) {
      s->setCandidate(none, none, false);
      s->computeDirection();
    }
    fddp_handle* h = solver.handle();
    int bad = 0;
    bad += compare("Vxx", solver.get_Vxx(), h, FDDP_Q_VXX, T + 1, (size_t)n * n, true);
    bad += compare("Vx", solver.get_Vx(), h, FDDP_Q_VX, T + 1, n, true);
    bad += compare("Qxx", solver.get_Qxx(), h, FDDP_Q_QXX, T, (size_t)n * n, true);
    bad += compare("Qxu", solver.get_Qxu(), h, FDDP_Q_QXU, T, (size_t)n * m, true);
    bad += compare("Quu", solver.get_Quu(), h, FDDP_Q_QUU, T, (size_t)m * m, true);
    bad += compare("Qx", solver.get_Qx(), h, FDDP_Q_QX, T, n, true);
    bad += compare("Qu", solver.get_Qu(), h, FDDP_Q_QU, T, m, true);
    bad += same("Vxx", solver.get_Vxx(), dbg.get_Vxx()) + same("Vx", solver.get_Vx(), dbg.get_Vx()) +
           same("Qxx", solver.get_Qxx(), dbg.get_Qxx()) + same("Qxu", solver.get_Qxu(), dbg.get_Qxu()) +
           same("Quu", solver.get_Quu(), dbg.get_Quu()) + same("Qx", solver.get_Qx(), dbg.get_Qx()) +
           same("Qu", solver.get_Qu(), dbg.get_Qu()) + same("K", solver.get_K(), dbg.get_K());
    // SolverBoxFDDP: Quu_inv of the last pass of a solve that ends on its limits
    auto bmodel = std::make_shared<croc::ActionModelLQR>(n, m, false);
    croc::VectorXd lim(m, 0.);  // graded: with 0.05 on every control the solution clamps them all (Quu_inv = 0)
    for (int i = 0; i < m; ++i) lim[i] = 0.05 + 2.95 * i / (m - 1);
    croc::VectorXd nlim(lim);
    for (double& v : nlim) v = -v;
    bmodel->set_u_lb(nlim);
    bmodel->set_u_ub(lim);
    std::vector<std::shared_ptr<croc::ActionModelBase> > brun(T, bmodel);
    auto bprob = std::make_shared<croc::ShootingProblem>(x0, brun, bmodel);
    croc::SolverBoxFDDP bsolver(bprob);
    bsolver.solve(none, none, 4);
    bad += compare("Quu_inv", bsolver.get_Quu_inv(), bsolver.handle(), FDDP_Q_QUU_INV, T, (size_t)m * m, true);
    std::printf(bad ? "getters FAILED\n" : "getters ok\n");
    return bad ? 1 : 0;
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
}
