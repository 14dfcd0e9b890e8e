// The impulse costs on the C++ facade: a one-legged hopper (free-flyer, hip, knee, ankle; a
// sole frame under the ankle, a toe frame beside it) lands through an
// ActionModelImpulseFwdDynamics with a 6D sole impulse behind a 3D toe impulse in name order,
// and asks of the landing impulse what the reference fork's jumps ask: CostModelContactImpulse
// (default and weighted), CostModelImpulseFrictionCone (the cone's own barrier by default),
// CostModelImpulseCoPPosition (default and weighted barrier) and CostModelImpulseCoM; a second
// landing knot has the toe impulse switched off (its costs read Lambda = 0) and no multiplier
// Jacobians. Packs the problem; tests/test_impulse_costs_cpp.py builds the same with the
// Python facade and compares the blocks double for double.
//
// usage: impulse_costs_example pack FILE     write the knot descriptors + parameter pool
//        impulse_costs_example refuse WHAT   print the refusal of: cop3d (a CoP cost on a 3D
//                                            impulse), contact (a contact-class cost on an
//                                            impulse knot), dam (an impulse cost in a
//                                            differential model), noimpulse (a frame without
//                                            any impulse)
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "crocoddyl_amd/multibody.hpp"

namespace croc = crocoddyl_amd;
using croc::Vec3;
using croc::VectorXd;

static std::shared_ptr<croc::Model> hopper() {
  auto m = std::make_shared<croc::Model>(croc::JointModelFreeFlyer());
  m->appendBodyToJoint(1, croc::Inertia(4.0, Vec3(0.01, 0., 0.05), croc::Mat3::Diag(0.05, 0.06, 0.03)));
  m->addFrame("torso", 1, croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., 0.2)));
  int j = m->addJoint(1, croc::JointModelRevoluteUnaligned(Vec3(0, 1, 0)), croc::SE3(croc::Mat3::Identity(), Vec3(0., 0.05, -0.1)),
                      "hip");
  m->appendBodyToJoint(j, croc::Inertia(1.2, Vec3(0., 0., -0.15), croc::Mat3::Diag(0.01, 0.01, 0.002)));
  j = m->addJoint(j, croc::JointModelRevoluteUnaligned(Vec3(0, 1, 0)), croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., -0.3)),
                  "knee");
  m->appendBodyToJoint(j, croc::Inertia(0.8, Vec3(0., 0., -0.14), croc::Mat3::Diag(0.008, 0.008, 0.001)));
  const int knee = j;
  j = m->addJoint(j, croc::JointModelRevoluteUnaligned(Vec3(1, 0, 0)), croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., -0.3)),
                  "ankle");
  m->appendBodyToJoint(j, croc::Inertia(0.3, Vec3(0.02, 0., -0.03), croc::Mat3::Diag(0.0005, 0.001, 0.001)));
  m->addFrame("sole", j, croc::SE3(croc::Mat3::Identity(), Vec3(0.01, 0., -0.06)));
  m->addFrame("shin", knee, croc::SE3(croc::Mat3::Identity(), Vec3(0.03, 0., -0.2)));
  return m;
}

typedef std::shared_ptr<croc::ActionModelBase> Action;
typedef std::shared_ptr<croc::CostModelAbstract> Cost;

static std::shared_ptr<croc::ActivationModelAbstract> weighted_barrier(int nr, double lb, double ub) {
  VectorXd w(nr);
  for (int i = 0; i < nr; ++i) w[i] = 0.5 + 0.25 * i;
  return std::make_shared<croc::ActivationModelWeightedQuadraticBarrier>(croc::ActivationBounds(VectorXd(nr, lb), VectorXd(nr, ub)), w);
}

// the landing knot: "a_shin" (3D) precedes "sole" (6D) in name order, so the sole's rows are 3..8
static Action landing(std::shared_ptr<croc::Model> m, std::shared_ptr<croc::StateMultibody> state, bool shin_active,
                      bool enable_force, const std::string& extra = "") {
  const int sole = m->getFrameId("sole"), shin = m->getFrameId("shin"), torso = m->getFrameId("torso");
  auto impulses = std::make_shared<croc::ImpulseModelMultiple>(state);
  if (extra == "cop3d")
    impulses->addImpulse("sole", std::make_shared<croc::ImpulseModel3D>(state, sole));
  else
    impulses->addImpulse("sole", std::make_shared<croc::ImpulseModel6D>(state, sole));
  impulses->addImpulse("a_shin", std::make_shared<croc::ImpulseModel3D>(state, shin), shin_active);
  auto costs = std::make_shared<croc::CostModelSum>(state, 0);
  const double fref[6] = {0.5, -0.25, 3., 0.01, 0.02, -0.03}, zero[6] = {0., 0., 0., 0., 0., 0.};
  croc::FrictionCone cone(Vec3(0., 0., 1.), 0.7, 4, false);
  if (extra != "cop3d") {
    costs->addCost("sole_impulse", std::make_shared<croc::CostModelContactImpulse>(state, croc::FrameForce(sole, fref)), 1e-2);
  }
  costs->addCost("shin_impulse",
                 std::make_shared<croc::CostModelContactImpulse>(
                     state, std::make_shared<croc::ActivationModelWeightedQuad>(VectorXd{1., 2., 0.5}), croc::FrameForce(shin, zero)),
                 2e-2);
  costs->addCost("sole_cone", std::make_shared<croc::CostModelImpulseFrictionCone>(state, croc::FrameFrictionCone(sole, cone)), 1e1);
  costs->addCost("shin_cone",
                 std::make_shared<croc::CostModelImpulseFrictionCone>(state, weighted_barrier(5, -1., 2.),
                                                                      croc::FrameFrictionCone(shin, cone)),
                 5.);
  costs->addCost("sole_CoP", std::make_shared<croc::CostModelImpulseCoPPosition>(state, croc::FrameCoPSupport(sole, 0.2, 0.1)), 1e1);
  if (extra != "cop3d")
    costs->addCost("sole_CoP_weighted",
                   std::make_shared<croc::CostModelImpulseCoPPosition>(state, weighted_barrier(4, 0., DBL_MAX),
                                                                       croc::FrameCoPSupport(sole, 0.16, 0.08)),
                   2.5);
  costs->addCost("com", std::make_shared<croc::CostModelImpulseCoM>(state), 1e2);
  costs->addCost("com_weighted",
                 std::make_shared<croc::CostModelImpulseCoM>(state, std::make_shared<croc::ActivationModelWeightedQuad>(VectorXd{1., 1., 4.})),
                 3.);
  VectorXd xref(state->get_nx(), 0.);
  xref[6] = 1.;
  costs->addCost("xReg", std::make_shared<croc::CostModelState>(state, xref, 0), 1e-1);
  if (extra == "contact")
    costs->addCost("contact_cone", std::make_shared<croc::CostModelContactFrictionCone>(state, croc::FrameFrictionCone(sole, cone), 0),
                   1.);
  if (extra == "noimpulse")
    costs->addCost("torso_impulse", std::make_shared<croc::CostModelContactImpulse>(state, croc::FrameForce(torso, zero), 3), 1.);
  return std::make_shared<croc::ActionModelImpulseFwdDynamics>(state, impulses, costs, 0.25, 1e-6, enable_force);
}

// a swing knot (free dynamics, floating-base actuation); with `impulse_cost` an impulse cost in it
static Action swing(std::shared_ptr<croc::StateMultibody> state, double dt, bool impulse_cost) {
  auto actuation = std::make_shared<croc::ActuationModelFloatingBase>(state);
  auto costs = std::make_shared<croc::CostModelSum>(state, impulse_cost ? 0 : actuation->nu);
  if (impulse_cost)
    costs->addCost("com", std::make_shared<croc::CostModelImpulseCoM>(state), 1.);
  else
    costs->addCost("ctrlReg", std::make_shared<croc::CostModelControl>(state, actuation->nu), 1e-1);
  if (impulse_cost) actuation->nu = 0;  // (so that the sum's dimension matches and the cost itself is refused)
  auto dmodel = std::make_shared<croc::DifferentialActionModelFreeFwdDynamics>(state, actuation, costs);
  return std::make_shared<croc::IntegratedActionModelEuler>(dmodel, dt);
}

static int write_pack(const char* file, std::shared_ptr<croc::ShootingProblem> problem) {
  std::vector<fddp_knot_desc> knots;
  VectorXd pool;
  problem->pack(knots, pool);
  const int64_t nk = (int64_t)knots.size(), np = (int64_t)pool.size();
  const int32_t dims[4] = {problem->get_nx(), problem->get_ndx(), problem->get_nu_max(), problem->get_T()};
  FILE* f = file ? std::fopen(file, "wb") : nullptr;
  if (!f) return 3;
  std::fwrite(dims, 1, sizeof(dims), f);
  std::fwrite(&nk, 1, 8, f);
  std::fwrite(knots.data(), 1, sizeof(fddp_knot_desc) * nk, f);
  std::fwrite(&np, 1, 8, f);
  std::fwrite(pool.data(), 1, 8 * np, f);
  std::fclose(f);
  std::printf("packed T=%d nx=%d knots=%lld pool=%lld\n", problem->get_T(), problem->get_nx(), (long long)nk, (long long)np);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s pack FILE | refuse cop3d|contact|dam|noimpulse\n", argv[0]);
    return 2;
  }
  try {
    auto m = hopper();
    auto state = std::make_shared<croc::StateMultibody>(m);
    VectorXd x0(state->get_nx(), 0.);
    x0[2] = 0.7;
    x0[6] = 1.;
    if (!std::strcmp(argv[1], "refuse")) {
      const std::string what = argv[2];
      std::vector<Action> models = {what == "dam" ? swing(state, 1e-2, true) : landing(m, state, true, true, what)};
      auto problem = std::make_shared<croc::ShootingProblem>(x0, models, swing(state, 0., false));
      std::vector<fddp_knot_desc> knots;
      VectorXd out;
      problem->pack(knots, out);
      std::printf("packed what should have been refused: %s\n", what.c_str());
      return 4;
    }
    std::vector<Action> models = {swing(state, 1e-2, false), landing(m, state, true, true), landing(m, state, false, false),
                                  swing(state, 1e-2, false)};
    return write_pack(argv[2], std::make_shared<croc::ShootingProblem>(x0, models, swing(state, 0., false)));
  } catch (const croc::Exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}
