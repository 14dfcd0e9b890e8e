// Prismatic joints on the C++ facade: the cart-pole (a prismatic cart along x, a revolute pole
// about y, ActuationModelLinear S = [1, 0]^T on free forward dynamics) and the two-legged hopper
// (a free-flyer body, per leg a revolute hip and a prismatic shank; floating-base actuation, a 3D
// contact on one foot and a 6D one on the other), with the numbers of
// crocoddyl_amd/robots.py sample_cartpole / sample_hopper. Packs a horizon of either;
// tests/test_prismatic_cpp.py builds the same with the Python facade and compares the blocks bit
// for bit, and the joint placements of the host kinematics.
//
// usage: prismatic_example pack cartpole|hopper FILE   write the knot descriptors + parameter pool
//        prismatic_example kin cartpole|hopper         print oMi of every joint at a fixed q
//        prismatic_example refuse                      print the refusal of a zero prismatic axis
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "crocoddyl_amd/multibody.hpp"

namespace croc = crocoddyl_amd;
using croc::Mat3;
using croc::SE3;
using croc::Vec3;
using croc::VectorXd;

typedef std::shared_ptr<croc::ActionModelBase> Action;
typedef std::shared_ptr<croc::ActuationModelAbstract> Actuation;
typedef std::shared_ptr<croc::Model> ModelPtr;
typedef std::shared_ptr<croc::StateMultibody> StatePtr;

static ModelPtr cartpole() {
  auto m = std::make_shared<croc::Model>();
  const int cart = m->addJoint(0, croc::JointModelPX(), SE3(), "cart_joint");
  m->appendBodyToJoint(cart, croc::Inertia(1.0, Vec3(0., 0., 0.), Mat3::Diag(0.02, 0.02, 0.02)));
  m->addFrame("cart_joint", cart);
  const int pole = m->addJoint(cart, croc::JointModelRY(), SE3(), "pole_joint");
  m->appendBodyToJoint(pole, croc::Inertia(0.3, Vec3(0., 0., -0.8), Mat3::Diag(0., 0., 0.)));
  m->addFrame("pole_joint", pole);
  m->addFrame("pole_tip", pole, SE3(Mat3::Identity(), Vec3(0., 0., -0.8)));
  return m;
}

static ModelPtr hopper() {
  auto m = std::make_shared<croc::Model>(croc::JointModelFreeFlyer());
  m->appendBodyToJoint(1, croc::Inertia(4.0, Vec3(0., 0., 0.02), Mat3::Diag(0.06, 0.05, 0.07)));
  m->addFrame("root_joint", 1);
  m->addFrame("base_link", 1);
  for (int k = 0; k < 2; ++k) {
    const std::string leg = "leg" + std::to_string(k);
    const double y = 0.12 * (2.0 * k / 1 - 1.0);
    const int hip = m->addJoint(1, croc::JointModelRY(), SE3(Mat3::Identity(), Vec3(0., y, -0.05)), leg + "_hip");
    m->appendBodyToJoint(hip, croc::Inertia(0.8, Vec3(0., 0., -0.12), Mat3::Diag(0.006, 0.006, 0.001)));
    m->addFrame(leg + "_hip", hip);
    const int shank = m->addJoint(hip, croc::JointModelPrismaticUnaligned(0., 0., -1.), SE3(Mat3::Identity(), Vec3(0., 0., -0.25)),
                                  leg + "_shank");
    m->appendBodyToJoint(shank, croc::Inertia(0.4, Vec3(0., 0., -0.15), Mat3::Diag(0.004, 0.004, 0.0005)));
    m->addFrame(leg + "_shank", shank);
    m->addFrame(leg + "_foot", shank, SE3(Mat3::Identity(), Vec3(0., 0., -0.3)));
    m->setJointLimits(hip, -1.2, 1.2, 10.0);
    m->setJointLimits(shank, -0.15, 0.15, 3.0);
  }
  return m;
}

static VectorXd standing() { return VectorXd{0., 0., 0.58, 0., 0., 0., 1., 0.1, -0.02, -0.1, -0.02}; }

static std::shared_ptr<croc::CostModelSum> costs_of(ModelPtr m, StatePtr state, int nu, const VectorXd& xref,
                                                    const std::string& frame, const Vec3& target) {
  auto costs = std::make_shared<croc::CostModelSum>(state, nu);
  costs->addCost("xReg", std::make_shared<croc::CostModelState>(state, xref, nu), 1e-2);
  costs->addCost("uReg", std::make_shared<croc::CostModelControl>(state, nu), 1e-2);
  costs->addCost("track", std::make_shared<croc::CostModelFrameTranslation>(
                              state, croc::FrameTranslation(m->getFrameId(frame), target), nu), 1.0);
  return costs;
}

static Action cartpole_knot(ModelPtr m, StatePtr state, double dt) {
  Actuation act = std::make_shared<croc::ActuationModelLinear>(state, VectorXd{1., 0.}, 1);
  auto dmodel = std::make_shared<croc::DifferentialActionModelFreeFwdDynamics>(
      state, act, costs_of(m, state, 1, VectorXd(4, 0.), "pole_tip", Vec3(0., 0., 0.8)));
  return std::make_shared<croc::IntegratedActionModelEuler>(dmodel, dt);
}

static Action hopper_knot(ModelPtr m, StatePtr state, double dt) {
  Actuation act = std::make_shared<croc::ActuationModelFloatingBase>(state);
  const int nu = act->nu;
  auto contacts = std::make_shared<croc::ContactModelMultiple>(state, nu);
  const double gains[2] = {0., 10.};
  contacts->addContact("c0_foot0", std::make_shared<croc::ContactModel3D>(
                                       state, croc::FrameTranslation(m->getFrameId("leg0_foot"), Vec3(0.1, -0.12, 0.)), nu, gains));
  contacts->addContact("c1_foot1", std::make_shared<croc::ContactModel6D>(
                                       state, croc::FramePlacement(m->getFrameId("leg1_foot"),
                                                                   SE3(Mat3::Identity(), Vec3(-0.1, 0.12, 0.01))), nu, gains));
  VectorXd xref(state->get_nx(), 0.);
  const VectorXd q0 = standing();
  for (size_t i = 0; i < q0.size(); ++i) xref[i] = q0[i];
  auto dmodel = std::make_shared<croc::DifferentialActionModelContactFwdDynamics>(
      state, act, contacts, costs_of(m, state, nu, xref, "base_link", Vec3(0., 0., 0.6)), 1e-3, true);
  return std::make_shared<croc::IntegratedActionModelEuler>(dmodel, dt);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s pack cartpole|hopper FILE | kin cartpole|hopper | refuse\n", argv[0]);
    return 2;
  }
  try {
    if (!std::strcmp(argv[1], "refuse")) {
      croc::JointModelPrismaticUnaligned(0., 0., 0.);
      std::printf("built what should have been refused\n");
      return 4;
    }
    if (argc < 3) return 2;
    const bool cp = !std::strcmp(argv[2], "cartpole");
    ModelPtr m = cp ? cartpole() : hopper();
    if (!std::strcmp(argv[1], "kin")) {
      VectorXd q = cp ? VectorXd{0.3, 0.7} : standing();
      if (!cp) q[8] = 0.07, q[10] = -0.11;
      const std::vector<SE3> oM = m->placements(q);
      std::printf("%d %d %d\n", m->njoints(), m->nq(), m->nv());
      for (int j = 1; j < m->njoints(); ++j) {
        std::printf("%d", m->kinds[j]);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) std::printf(" %.17g", oM[j].rotation(r, c));
        for (int r = 0; r < 3; ++r) std::printf(" %.17g", oM[j].translation[r]);
        std::printf("\n");
      }
      return 0;
    }
    if (argc < 4) return 2;
    auto state = std::make_shared<croc::StateMultibody>(m);
    VectorXd x0(state->get_nx(), 0.);
    if (cp) {
      x0[1] = 0.3;
    } else {
      const VectorXd q0 = standing();
      for (size_t i = 0; i < q0.size(); ++i) x0[i] = q0[i];
    }
    const Action running = cp ? cartpole_knot(m, state, 5e-2) : hopper_knot(m, state, 1e-2);
    const std::vector<Action> models(3, running);  // (one model for the three knots: one block)
    auto problem = std::make_shared<croc::ShootingProblem>(x0, models, cp ? cartpole_knot(m, state, 0.) : hopper_knot(m, state, 0.));
    std::vector<fddp_knot_desc> knots;
    VectorXd pool;
    problem->pack(knots, pool);
    const int64_t nk = (int64_t)knots.size(), np = (int64_t)pool.size();
    const int32_t dims[4] = {problem->get_nx(), problem->get_ndx(), problem->get_nu_max(), problem->get_T()};
    FILE* f = std::fopen(argv[3], "wb");
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
