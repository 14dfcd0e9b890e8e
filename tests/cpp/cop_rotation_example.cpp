// CostModelContactCoPPosition and CostModelFrameRotation on the C++ facade: a one-legged
// hopper (free-flyer, hip, knee, ankle; a sole frame under the ankle) with the costs of the
// reference fork's humanoid walks on its stance knot -- a 6D sole contact, its friction cone,
// the CoP cost with the default barrier and with a weighted one, a torso rotation cost -- an
// impulse knot with the rotation cost, and a stance knot whose sole contact is switched off.
// Packs the problem; tests/test_ext_costs_cpp.py builds the same with the Python facade and
// compares the blocks bit for bit.
//
// usage: cop_rotation_example pack FILE     write the knot descriptors + parameter pool
//        cop_rotation_example refuse        a CoP cost on a 3D contact: prints the refusal
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
  j = m->addJoint(j, croc::JointModelRevoluteUnaligned(Vec3(1, 0, 0)), croc::SE3(croc::Mat3::Identity(), Vec3(0., 0., -0.3)),
                  "ankle");
  m->appendBodyToJoint(j, croc::Inertia(0.3, Vec3(0.02, 0., -0.03), croc::Mat3::Diag(0.0005, 0.001, 0.001)));
  m->addFrame("sole", j, croc::SE3(croc::Mat3::Identity(), Vec3(0.01, 0., -0.06)));
  return m;
}

// Rx(-0.2) Rz(0.3), entries written out: both facades are given the same doubles
static croc::Mat3 torso_ref() {
  const double a[3][3] = {{0.955336489125606, -0.2955202066613396, 0.},
                          {0.2896294776255156, 0.9362933635841992, 0.19866933079506122},
                          {-0.058710801693827154, -0.1897961286473454, 0.9800665778412416}};
  croc::Mat3 R;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) R(i, k) = a[i][k];
  return R;
}

typedef std::shared_ptr<croc::ActionModelBase> Action;

static Action stance(std::shared_ptr<croc::Model> m, std::shared_ptr<croc::StateMultibody> state, bool contact6d,
                     bool active, double dt) {
  auto actuation = std::make_shared<croc::ActuationModelFloatingBase>(state);
  const int nu = actuation->nu, sole = m->getFrameId("sole"), torso = m->getFrameId("torso");
  auto contacts = std::make_shared<croc::ContactModelMultiple>(state, nu);
  const double gains[2] = {0., 30.};
  if (contact6d)
    contacts->addContact("sole_contact",
                         std::make_shared<croc::ContactModel6D>(state, croc::FramePlacement(sole, croc::SE3::Identity()), nu, gains),
                         active);
  else
    contacts->addContact("sole_contact",
                         std::make_shared<croc::ContactModel3D>(state, croc::FrameTranslation(sole, Vec3(0., 0., 0.)), nu, gains),
                         active);
  auto costs = std::make_shared<croc::CostModelSum>(state, nu);
  croc::FrictionCone cone(Vec3(0., 0., 1.), 0.7, 4, false);
  costs->addCost("sole_frictionCone",
                 std::make_shared<croc::CostModelContactFrictionCone>(
                     state, std::make_shared<croc::ActivationModelQuadraticBarrier>(croc::ActivationBounds(cone.lb, cone.ub)),
                     croc::FrameFrictionCone(sole, cone), nu),
                 1e1);
  costs->addCost("sole_CoP", std::make_shared<croc::CostModelContactCoPPosition>(state, croc::FrameCoPSupport(sole, 0.2, 0.1), nu),
                 1e1);
  costs->addCost("sole_CoP_weighted",
                 std::make_shared<croc::CostModelContactCoPPosition>(
                     state,
                     std::make_shared<croc::ActivationModelWeightedQuadraticBarrier>(
                         croc::ActivationBounds(VectorXd(4, 0.), VectorXd(4, DBL_MAX)), VectorXd{0.5, 1., 2., 1.5}),
                     croc::FrameCoPSupport(sole, 0.16, 0.08), nu),
                 2.5);
  costs->addCost("torsoRot", std::make_shared<croc::CostModelFrameRotation>(state, croc::FrameRotation(torso, torso_ref()), nu),
                 1e2);
  costs->addCost("torsoRot_weighted",
                 std::make_shared<croc::CostModelFrameRotation>(
                     state, std::make_shared<croc::ActivationModelWeightedQuad>(VectorXd{1., 2., 0.5}),
                     croc::FrameRotation(sole, croc::Mat3::Identity()), nu),
                 3.0);
  costs->addCost("ctrlReg", std::make_shared<croc::CostModelControl>(state, nu), 1e-1);
  auto dmodel = std::make_shared<croc::DifferentialActionModelContactFwdDynamics>(state, actuation, contacts, costs, 1e-6, true);
  return std::make_shared<croc::IntegratedActionModelEuler>(dmodel, dt);
}

static Action landing(std::shared_ptr<croc::Model> m, std::shared_ptr<croc::StateMultibody> state) {
  auto impulses = std::make_shared<croc::ImpulseModelMultiple>(state);
  impulses->addImpulse("sole_impulse", std::make_shared<croc::ImpulseModel6D>(state, m->getFrameId("sole")));
  auto costs = std::make_shared<croc::CostModelSum>(state, 0);
  costs->addCost("torsoRot",
                 std::make_shared<croc::CostModelFrameRotation>(state, croc::FrameRotation(m->getFrameId("torso"), torso_ref()), 0),
                 1e2);
  return std::make_shared<croc::ActionModelImpulseFwdDynamics>(state, impulses, costs);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s pack FILE | refuse\n", argv[0]);
    return 2;
  }
  try {
    auto m = hopper();
    auto state = std::make_shared<croc::StateMultibody>(m);
    if (!std::strcmp(argv[1], "refuse")) {
      VectorXd out;
      auto em = std::dynamic_pointer_cast<croc::IntegratedActionModelEuler>(stance(m, state, false, true, 1e-2));
      std::vector<Action> models = {em};
      VectorXd x0(state->get_nx(), 0.);
      x0[6] = 1.;
      auto problem = std::make_shared<croc::ShootingProblem>(x0, models, models.back());
      std::vector<fddp_knot_desc> knots;
      problem->pack(knots, out);
      std::printf("packed a CoP cost on a 3D contact\n");
      return 4;
    }
    if (argc < 3) return 2;
    std::vector<Action> models = {stance(m, state, true, true, 1e-2), landing(m, state), stance(m, state, true, false, 1e-2),
                                  stance(m, state, true, true, 0.)};
    VectorXd x0(state->get_nx(), 0.);
    x0[2] = 0.7;
    x0[6] = 1.;
    auto problem = std::make_shared<croc::ShootingProblem>(x0, models, models.back());
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
