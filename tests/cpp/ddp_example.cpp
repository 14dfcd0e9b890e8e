// crocoddyl_amd::SolverDDP and SolverBoxDDP through the C++ facade, on the problems
// tests/test_ddp_cpp.py solves with the Python facade: the unicycle of the reference's
// examples/notebooks/unicycle_towards_origin.ipynb (cost weights (3, 1), x0 = (-4, -4, 0),
// T = 20), which constructs crocoddyl.SolverDDP(problem), and a control-limited LQR.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "crocoddyl_amd/solver_fddp_hip.hpp"

namespace croc = crocoddyl_amd;

int main() {
  try {
    auto uni = std::make_shared<croc::ActionModelUnicycle>();
    uni->wx = 3.;
    uni->wu = 1.;
    std::vector<std::shared_ptr<croc::ActionModelBase> > urun(20, uni);
    croc::VectorXd ux0 = {-4., -4., 0.};
    auto uprob = std::make_shared<croc::ShootingProblem>(ux0, urun, uni);
    croc::SolverDDP ddp(uprob);
    const bool ok = ddp.solve();
    const auto xs = ddp.get_xs();
    std::printf("ddp converged=%d iter=%zu feasible=%d cost=%.17e stop=%.17e xT=%.17e,%.17e,%.17e d=%.17e,%.17e\n", ok,
                ddp.get_iter(), ddp.get_is_feasible() ? 1 : 0, ddp.get_cost(), ddp.get_stop(), xs.back()[0],
                xs.back()[1], xs.back()[2], ddp.get_d()[0], ddp.get_d()[1]);
    // the phases of a DDP solver: no gap is closed at any step length
    croc::SolverDDP step(uprob);
    std::vector<croc::VectorXd> xw(21, croc::VectorXd{-3., -3.5, 0.2});
    step.setCandidate(xw, std::vector<croc::VectorXd>(), false);
    step.set_solver_state(0, 1e-9, 1e-9, false);
    step.computeDirection(true);
    const double dV = step.tryStep(0.5);
    const auto d = step.expectedImprovement();
    const auto xt = step.get_xs_try();
    std::printf("step dV=%.17e d=%.17e,%.17e x0try=%.17e,%.17e,%.17e\n", dV, d[0], d[1], xt[0][0], xt[0][1], xt[0][2]);
    // control-limited LQR with SolverBoxDDP (box-ddp.cpp)
    const int T = 20;
    auto bmodel = std::make_shared<croc::ActionModelLQR>(24, 12, false);
    bmodel->set_u_lb(croc::VectorXd(12, -0.05));
    bmodel->set_u_ub(croc::VectorXd(12, 0.05));
    std::vector<std::shared_ptr<croc::ActionModelBase> > brun(T, bmodel);
    croc::VectorXd x0(24, 0.);
    auto bprob = std::make_shared<croc::ShootingProblem>(x0, brun, bmodel);
    croc::SolverBoxDDP box(bprob);
    const bool bok = box.solve(std::vector<croc::VectorXd>(), std::vector<croc::VectorXd>(), 20);
    double umax = 0.;
    for (const auto& u : box.get_us())
      for (double v : u) umax = std::max(umax, std::fabs(v));
    std::printf("box converged=%d iter=%zu feasible=%d cost=%.17e umax=%.17e th_stop=%.1e\n", bok, box.get_iter(),
                box.get_is_feasible() ? 1 : 0, box.get_cost(), umax, box.get_th_stop());
    return (ok && umax <= 0.05) ? 0 : 2;
  } catch (const croc::Exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}
