// The squashed actuation on the C++ facade: a quadrotor with a two-joint arm (free-flyer base body,
// two short revolute links, a tip frame) under ActuationSquashingModel(ActuationModelMultiCopterBase,
// SquashingModelSmoothSat) in free flight (the contact-kind block with no contacts and section
// flag 4) and with its arm's tip held by a 6D contact (flag 4 | 2 after the contact), a knot whose
// squashed inner actuation is the floating base (S written as the selection matrix), and one with
// another smooth value. Packs the problem; tests/test_squashing_cpp.py builds the same with the
// Python facade and compares the blocks double for double.
//
// usage: squashing_example pack FILE          write the knot descriptors + parameter pool
//        squashing_example solve FILE ITERS   SolverFDDP on the GPU: the result and the trajectory
//        squashing_example refuse WHAT        print the refusal of: nu (a squashing of another nu than
//                                             the actuation's), ns (of another ns), bounds (lb >= ub),
//                                             smooth (a negative smooth), twice (a squashed actuation
//                                             squashed again)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "crocoddyl_amd/multibody.hpp"
#include "crocoddyl_amd/solver_fddp_hip.hpp"

namespace croc = crocoddyl_amd;
using croc::Vec3;
using croc::VectorXd;

static std::shared_ptr<croc::Model> quadrotor_arm() {
  auto m = std::make_shared<croc::Model>(croc::JointModelFreeFlyer());
  m->appendBodyToJoint(1, croc::Inertia(1.477, Vec3(0., 0., -0.01), croc::Mat3::Diag(0.0115, 0.0115, 0.0218)));
  m->addFrame("base_link", 1, croc::SE3::Identity());
  int j = m->addJoint(1, croc::JointModelRevoluteUnaligned(Vec3(0, 1, 0)), croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., -0.05)),
                      "arm_1_joint");
  m->appendBodyToJoint(j, croc::Inertia(0.12, Vec3(0., 0., -0.06), croc::Mat3::Diag(4e-4, 4e-4, 5e-5)));
  j = m->addJoint(j, croc::JointModelRevoluteUnaligned(Vec3(1, 0, 0)), croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., -0.12)),
                  "arm_2_joint");
  m->appendBodyToJoint(j, croc::Inertia(0.12, Vec3(0., 0., -0.06), croc::Mat3::Diag(4e-4, 4e-4, 5e-5)));
  m->addFrame("arm_tip", j, croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., -0.12)));
  return m;
}

// the quadrotor example's map, row-major 6 x 4
static VectorXd tau_f(double d = 0.1525, double cf = 6.6e-5, double cm = 1e-6) {
  const double r = cm / cf;
  return VectorXd{0., 0., 0., 0., 0., 0., 0., 0., 1., 1., 1., 1., 0., d, 0., -d, -d, 0., d, 0., -r, r, -r, r};
}

typedef std::shared_ptr<croc::ActionModelBase> Action;
typedef std::shared_ptr<croc::ActuationModelAbstract> Actuation;

static std::shared_ptr<croc::CostModelSum> costs_of(std::shared_ptr<croc::Model> m, std::shared_ptr<croc::StateMultibody> state,
                                                    int nu) {
  auto costs = std::make_shared<croc::CostModelSum>(state, nu);
  VectorXd xref(state->get_nx(), 0.);
  xref[6] = 1.;
  costs->addCost("xReg", std::make_shared<croc::CostModelState>(state, xref, nu), 1e-2);
  costs->addCost("uReg", std::make_shared<croc::CostModelControl>(state, nu), 1e-2);
  costs->addCost("goalPose",
                 std::make_shared<croc::CostModelFramePlacement>(
                     state, croc::FramePlacement(m->getFrameId("arm_tip"), croc::SE3(croc::Mat3::Identity(), Vec3(0.3, -0.2, 0.4))), nu),
                 1.0);
  return costs;
}

static Action flight(std::shared_ptr<croc::Model> m, std::shared_ptr<croc::StateMultibody> state, Actuation act, double dt) {
  auto dmodel = std::make_shared<croc::DifferentialActionModelFreeFwdDynamics>(state, act, costs_of(m, state, act->nu));
  return std::make_shared<croc::IntegratedActionModelEuler>(dmodel, dt);
}

static Action perched(std::shared_ptr<croc::Model> m, std::shared_ptr<croc::StateMultibody> state, Actuation act, double dt) {
  const int nu = act->nu;
  auto contacts = std::make_shared<croc::ContactModelMultiple>(state, nu);
  const double gains[2] = {0., 20.};
  contacts->addContact("tip_contact", std::make_shared<croc::ContactModel6D>(
                                          state, croc::FramePlacement(m->getFrameId("arm_tip"), croc::SE3::Identity()), nu, gains));
  auto dmodel = std::make_shared<croc::DifferentialActionModelContactFwdDynamics>(state, act, contacts, costs_of(m, state, nu),
                                                                                  1e-6, true);
  return std::make_shared<croc::IntegratedActionModelEuler>(dmodel, dt);
}

typedef std::shared_ptr<croc::SquashingModelSmoothSat> Squashing;

// thrusts in (0.1, 5), arm torques in (-2, 2)
static Squashing rotor_limits(double smooth = 0.1) {
  auto sq = std::make_shared<croc::SquashingModelSmoothSat>(VectorXd{0.1, 0.1, 0.1, 0.1, -2., -2.},
                                                            VectorXd{5., 5., 5., 5., 2., 2.}, 6);
  if (smooth != 0.1) sq->set_smooth(smooth);
  return sq;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s pack FILE | solve FILE ITERS | refuse nu|ns|bounds|smooth|twice\n", argv[0]);
    return 2;
  }
  try {
    auto m = quadrotor_arm();
    auto state = std::make_shared<croc::StateMultibody>(m);
    Actuation rotors = std::make_shared<croc::ActuationModelMultiCopterBase>(state, 4, tau_f());
    if (!std::strcmp(argv[1], "refuse")) {
      const std::string what = argv[2];
      if (what == "nu") {
        croc::ActuationSquashingModel(state, rotors, rotor_limits(), 5);
      } else if (what == "ns") {
        croc::ActuationSquashingModel(state, rotors,
                                      std::make_shared<croc::SquashingModelSmoothSat>(VectorXd(4, 0.), VectorXd(4, 1.), 4), 6);
      } else if (what == "bounds") {
        croc::SquashingModelSmoothSat(VectorXd{0., 1.}, VectorXd{1., 1.}, 2);
      } else if (what == "smooth") {
        rotor_limits()->set_smooth(-0.1);
      } else {
        Actuation once = std::make_shared<croc::ActuationSquashingModel>(state, rotors, rotor_limits(), 6);
        croc::ActuationSquashingModel(state, once, rotor_limits(), 6);
      }
      std::printf("built what should have been refused: %s\n", what.c_str());
      return 4;
    }
    Actuation squashed = std::make_shared<croc::ActuationSquashingModel>(state, rotors, rotor_limits(), 6);
    if (squashed->nu != 6 || squashed->matrix() != rotors->matrix() || squashed->squashing()->size() != 18) return 5;
    Actuation softer = std::make_shared<croc::ActuationSquashingModel>(state, rotors, rotor_limits(0.25), 6);
    // the floating base squashed: tau = [0_6; s(u)], nu = 2
    Actuation base = std::make_shared<croc::ActuationModelFloatingBase>(state);
    Actuation arm_only = std::make_shared<croc::ActuationSquashingModel>(
        state, base, std::make_shared<croc::SquashingModelSmoothSat>(VectorXd{-1., -0.5}, VectorXd{1., 1.5}, 2), 2);
    // s and ds/du on the host: the midpoint maps to itself
    {
      VectorXd sv, dv;
      rotor_limits()->calc(VectorXd{2.55, 2.55, 2.55, 2.55, 0., 0.}, sv);
      rotor_limits()->calcDiff(VectorXd{2.55, 2.55, 2.55, 2.55, 0., 0.}, dv);
      if (std::fabs(sv[0] - 2.55) > 1e-15 || std::fabs(sv[5]) > 1e-15 || !(dv[0] > 0.98 && dv[0] < 0.99)) return 6;
    }
    VectorXd x0(state->get_nx(), 0.);
    x0[2] = 0.5;
    x0[6] = 1.;
    std::vector<Action> models = {flight(m, state, squashed, 1e-2), perched(m, state, squashed, 1e-2),
                                  flight(m, state, arm_only, 1e-2), flight(m, state, softer, 1e-2)};
    auto problem = std::make_shared<croc::ShootingProblem>(x0, models, flight(m, state, squashed, 0.));
    if (!std::strcmp(argv[1], "solve")) {
      const int maxiter = argc > 3 ? std::atoi(argv[3]) : 3;
      const int T = problem->get_T();
      croc::SolverFDDP solver(problem);
      std::vector<VectorXd> xs(T + 1, x0), us;
      const bool ok = solver.solve(xs, us, maxiter, false, 1e-9);
      VectorXd flat;
      for (const auto& x : solver.get_xs()) flat.insert(flat.end(), x.begin(), x.end());
      for (const auto& u : solver.get_us()) {
        VectorXd up(problem->get_nu_max(), 0.);
        for (size_t c = 0; c < u.size() && c < up.size(); ++c) up[c] = u[c];
        flat.insert(flat.end(), up.begin(), up.end());
      }
      const fddp_result r = solver.get_results()[0];
      FILE* f = std::fopen(argv[2], "wb");
      if (!f) return 3;
      std::fwrite(&r, 1, sizeof(r), f);
      std::fwrite(flat.data(), 1, 8 * flat.size(), f);
      std::fclose(f);
      std::printf("squashing solved=%d iter=%zu cost=%.12e\n", ok, solver.get_iter(), solver.get_cost());
      return 0;
    }
    std::vector<fddp_knot_desc> knots;
    VectorXd pool;
    problem->pack(knots, pool);
    const int64_t nk = (int64_t)knots.size(), np = (int64_t)pool.size();
    const int32_t dims[4] = {problem->get_nx(), problem->get_ndx(), problem->get_nu_max(), problem->get_T()};
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(dims, 1, sizeof(dims), f);
    std::fwrite(&nk, 1, 8, f);
    std::fwrite(knots.data(), 1, sizeof(fddp_knot_desc) * nk, f);
    std::fwrite(&np, 1, 8, f);
    std::fwrite(pool.data(), 1, 8 * np, f);
    std::fclose(f);
    std::printf("packed T=%d nx=%d knots=%lld pool=%lld\n", problem->get_T(), problem->get_nx(), (long long)nk, (long long)np);
    return 0;
  } catch (const croc::Exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}
