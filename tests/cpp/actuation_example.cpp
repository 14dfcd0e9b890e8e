// The linear actuations on the C++ facade: a quadrotor with a two-joint arm (free-flyer base body,
// two short revolute links, a tip frame) under ActuationModelMultiCopterBase in free flight
// (DifferentialActionModelFreeFwdDynamics: the contact-kind block with no contacts and section
// flag 4) and with its arm's tip held by a 6D contact (DifferentialActionModelContactFwdDynamics
// through the ActuationModelAbstract overload: flag 4 | 2 after the contact), and a knot under
// ActuationModelLinear with a dense S. Packs the problem; tests/test_actuation_cpp.py builds the
// same with the Python facade and compares the blocks double for double.
//
// usage: actuation_example pack FILE     write the knot descriptors + parameter pool
//        actuation_example refuse WHAT   print the refusal of: freeflyer (a multicopter on a fixed
//                                        base), nu (an octocopter without an arm: nu > nv),
//                                        full (ActuationModelFull on the contact model)
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "crocoddyl_amd/multibody.hpp"

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

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s pack FILE | refuse freeflyer|nu|full\n", argv[0]);
    return 2;
  }
  try {
    auto m = quadrotor_arm();
    auto state = std::make_shared<croc::StateMultibody>(m);
    if (!std::strcmp(argv[1], "refuse")) {
      const std::string what = argv[2];
      if (what == "freeflyer") {
        auto arm = std::make_shared<croc::Model>();
        int j = arm->addJoint(0, croc::JointModelRevoluteUnaligned(Vec3(0, 0, 1)), croc::SE3::Identity(), "j1");
        arm->appendBodyToJoint(j, croc::Inertia(1., Vec3(0., 0., 0.1), croc::Mat3::Diag(0.01, 0.01, 0.01)));
        croc::ActuationModelMultiCopterBase(std::make_shared<croc::StateMultibody>(arm), 4, tau_f());
      } else if (what == "nu") {
        auto base = std::make_shared<croc::Model>(croc::JointModelFreeFlyer());
        base->appendBodyToJoint(1, croc::Inertia(1., Vec3(0., 0., 0.), croc::Mat3::Diag(0.01, 0.01, 0.01)));
        croc::ActuationModelMultiCopterBase(std::make_shared<croc::StateMultibody>(base), 8, VectorXd(48, 1.));
      } else {
        auto fixed = std::make_shared<croc::Model>();
        int j = fixed->addJoint(0, croc::JointModelRevoluteUnaligned(Vec3(0, 0, 1)), croc::SE3::Identity(), "j1");
        fixed->appendBodyToJoint(j, croc::Inertia(1., Vec3(0., 0., 0.1), croc::Mat3::Diag(0.01, 0.01, 0.01)));
        fixed->addFrame("arm_tip", j, croc::SE3::Identity());
        auto st = std::make_shared<croc::StateMultibody>(fixed);
        Actuation full = std::make_shared<croc::ActuationModelFull>(st);
        perched(fixed, st, full, 1e-2);
      }
      std::printf("built what should have been refused: %s\n", what.c_str());
      return 4;
    }
    Actuation rotors = std::make_shared<croc::ActuationModelMultiCopterBase>(state, 4, tau_f());
    if (rotors->nu != 6 || !rotors->matrix() || rotors->matrix()->size() != 48) return 5;
    // a dense S (8 x 3, column-major): S(i, c) = 0.1 (i + 1) - 0.3 c, the diagonal raised by one
    VectorXd S(24);
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 8; ++i) S[8 * c + i] = 0.1 * (i + 1) - 0.3 * c + (i == c ? 1. : 0.);
    Actuation dense = std::make_shared<croc::ActuationModelLinear>(state, S, 3);
    VectorXd x0(state->get_nx(), 0.);
    x0[2] = 0.5;
    x0[6] = 1.;
    std::vector<Action> models = {flight(m, state, rotors, 1e-2), perched(m, state, rotors, 1e-2), flight(m, state, dense, 1e-2),
                                  flight(m, state, rotors, 1e-2)};
    auto problem = std::make_shared<croc::ShootingProblem>(x0, models, flight(m, state, rotors, 0.));
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
