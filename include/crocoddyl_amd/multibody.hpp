// crocoddyl_amd C++ facade, multibody part (header-only): the reference's C++ model
// classes for the legged-robot path, as parameter carriers that pack the
// FDDP_KNOT_EULER_FREEFWD / _CONTACTFWD / FDDP_KNOT_IMPULSEFWD blocks of
// include/fddp_hip.h. Nothing here computes dynamics: calc / calcDiff run in
// libfddp_hip on the GPU. The host kinematics below (placements, frame placement,
// centre of mass, generalized gravity) serve problem builders (gait references,
// quasi-static warm starts), as pinocchio's do for the reference's builders.
//
// Reference classes mirrored (same names, constructor arguments and defaults):
//   pinocchio::Model subset: Model (addJoint, appendBodyToJoint, addFrame, getFrameId,
//     getJointId, nq, nv, gravity, referenceConfigurations, limits), SE3, Inertia,
//     JointModelFreeFlyer, JointModelRevoluteUnaligned / RX / RY / RZ,
//     JointModelPrismaticUnaligned / PX / PY / PZ
//   StateMultibody                            multibody/states/multibody.hxx:14-240
//   ActuationModelFull / ActuationModelFloatingBase   multibody/actuations/{full,floating-base}.hpp
//   ActuationModelMultiCopterBase                     multibody/actuations/multicopter-base.hpp
//   ActuationModelLinear (tau = S u, S constant)      a project extension
//   ActuationSquashingModel, SquashingModelSmoothSat  core/actuation/actuation-squashing.hpp, squashing/smooth-sat.hpp
//   ActivationModelQuad / WeightedQuad / QuadraticBarrier / WeightedQuadraticBarrier,
//     ActivationBounds                        core/activations/*.hpp
//   FrictionCone                              multibody/friction-cone.hxx:24-96
//   FramePlacement / FrameTranslation / FrameRotation / FrameMotion / FrameForce /
//     FrameFrictionCone / FrameCoPSupport     multibody/frames.hpp
//   CostModelState / Control / FramePlacement / FrameTranslation / FrameRotation /
//     FrameVelocity / CoMPosition / ContactForce / ContactFrictionCone /
//     ContactCoPPosition, CostModelSum
//                                             multibody/costs/*.hxx, cost-sum.hxx:18-160
//   ContactModel3D / ContactModel6D, ContactModelMultiple   multibody/contacts/*.hxx
//   DifferentialActionModelFreeFwdDynamics    multibody/actions/free-fwddyn.hxx:24-160
//   DifferentialActionModelContactFwdDynamics multibody/actions/contact-fwddyn.hxx:24-207
//   ImpulseModel3D / ImpulseModel6D, ImpulseModelMultiple, ActionModelImpulseFwdDynamics
//                                             multibody/impulses/*.hxx, actions/impulse-fwddyn.hxx
// with IntegratedActionModelEuler, ShootingProblem and SolverFDDP of
// solver_fddp_hip.hpp. The packing is the Python facade's
// (crocoddyl_amd/multibody.py) double for double; tests/test_cpp_multibody.py checks it.
#ifndef CROCODDYL_AMD_MULTIBODY_HPP_
#define CROCODDYL_AMD_MULTIBODY_HPP_

#include <cfloat>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "solver_fddp_hip.hpp"

namespace crocoddyl_amd {

// record type codes of the multibody blocks (include/fddp_hip.h)
enum { kJointRec = 27, kCostHdr = 4, kMaxContactRows = 24, kMaxDofs = 64 };
enum { JOINT_REVOLUTE = 0, JOINT_FREEFLYER = 1, JOINT_PRISMATIC = 2 };
enum { COST_STATE = 1, COST_CONTROL = 2, COST_FRAME_PLACEMENT = 3, COST_FRAME_TRANSLATION = 4, CONTACT_3D = 5,
       CONTACT_6D = 6, COST_CONTACT_FORCE = 7, COST_COM_POSITION = 8, COST_FRICTION_CONE = 9,
       COST_FRAME_VELOCITY = 10, COST_COP_POSITION = 11, COST_FRAME_ROTATION = 12, COST_IMPULSE_COM = 13,
       COST_CENTROIDAL_MOMENTUM = 14 };
enum { ACT_QUAD = 0, ACT_WEIGHTED_QUAD = 1, ACT_QUAD_BARRIER = 2, ACT_WEIGHTED_QUAD_BARRIER = 3 };
static const double kInactiveForceRow = -2.;  // the contact / impulse exists but is inactive

struct Vec3 {
  double v[3] = {0., 0., 0.};
  Vec3() {}
  Vec3(double x, double y, double z) : v{x, y, z} {}
  double& operator[](int i) { return v[i]; }
  double operator[](int i) const { return v[i]; }
  Vec3 operator+(const Vec3& o) const { return Vec3(v[0] + o[0], v[1] + o[1], v[2] + o[2]); }
  Vec3 operator-(const Vec3& o) const { return Vec3(v[0] - o[0], v[1] - o[1], v[2] - o[2]); }
  Vec3 operator*(double s) const { return Vec3(v[0] * s, v[1] * s, v[2] * s); }
  Vec3 operator/(double s) const { return Vec3(v[0] / s, v[1] / s, v[2] / s); }
};

struct Mat3 {  // row-major
  double m[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
  static Mat3 Identity() {
    Mat3 r;
    r.m[0][0] = r.m[1][1] = r.m[2][2] = 1.;
    return r;
  }
  static Mat3 Diag(double a, double b, double c) {
    Mat3 r;
    r.m[0][0] = a;
    r.m[1][1] = b;
    r.m[2][2] = c;
    return r;
  }
  double& operator()(int i, int j) { return m[i][j]; }
  double operator()(int i, int j) const { return m[i][j]; }
  Mat3 operator*(const Mat3& o) const {
    Mat3 r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.m[i][j] = m[i][0] * o.m[0][j] + m[i][1] * o.m[1][j] + m[i][2] * o.m[2][j];
    return r;
  }
  Vec3 operator*(const Vec3& x) const {
    Vec3 r;
    for (int i = 0; i < 3; ++i) r[i] = m[i][0] * x[0] + m[i][1] * x[1] + m[i][2] * x[2];
    return r;
  }
  Mat3 transpose() const {
    Mat3 r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.m[i][j] = m[j][i];
    return r;
  }
  Mat3 operator+(const Mat3& o) const {
    Mat3 r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.m[i][j] = m[i][j] + o.m[i][j];
    return r;
  }
};

// pinocchio::SE3 subset
struct SE3 {
  Mat3 rotation = Mat3::Identity();
  Vec3 translation;
  SE3() {}
  SE3(const Mat3& R, const Vec3& p) : rotation(R), translation(p) {}
  static SE3 Identity() { return SE3(); }
  SE3 inverse() const {
    const Mat3 Rt = rotation.transpose();
    const Vec3 t = Rt * translation;
    return SE3(Rt, Vec3(-t[0], -t[1], -t[2]));
  }
  SE3 operator*(const SE3& o) const { return SE3(rotation * o.rotation, translation + rotation * o.translation); }
  // pack: R column-major (Eigen's order: the rows of R^T) then p
  void pack(VectorXd& out) const {
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) out.push_back(rotation(i, j));
    for (int i = 0; i < 3; ++i) out.push_back(translation[i]);
  }
};

// pinocchio::Inertia: mass, lever (CoM in the joint frame), rotational inertia about the CoM
struct Inertia {
  double mass = 0.;
  Vec3 lever;
  Mat3 inertia;
  Inertia() {}
  Inertia(double m, const Vec3& c, const Mat3& I) : mass(m), lever(c), inertia(I) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        if (std::fabs(I(i, j) - I(j, i)) > 1e-12 * (1. + std::fabs(I(i, j))))
          throw Exception("Invalid argument: the rotational inertia must be symmetric");
  }
  static Inertia Zero() { return Inertia(); }
  Inertia se3Action(const SE3& M) const {  // Inertia::se3Action
    Inertia r;
    r.mass = mass;
    r.lever = M.rotation * lever + M.translation;
    r.inertia = M.rotation * inertia * M.rotation.transpose();
    return r;
  }
  Inertia operator+(const Inertia& o) const {  // Inertia::operator+ (parallel-axis shift)
    const double m = mass + o.mass;
    if (m == 0.) return Inertia();
    const Vec3 c = (lever * mass + o.lever * o.mass) / m;
    auto shift = [&](const Mat3& I, double mi, const Vec3& ci) {
      const Vec3 d = ci - c;
      const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      Mat3 S;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S(i, j) = mi * ((i == j ? dd : 0.) - d[i] * d[j]);
      return I + S;
    };
    Inertia r;
    r.mass = m;
    r.lever = c;
    r.inertia = shift(inertia, mass, lever) + shift(o.inertia, o.mass, o.lever);
    return r;
  }
};

struct JointModelFreeFlyer {};
struct JointModelRevoluteUnaligned {
  Vec3 axis;
  explicit JointModelRevoluteUnaligned(const Vec3& a) {
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (n == 0.) throw Exception("Invalid argument: zero joint axis");
    axis = a / n;
  }
  JointModelRevoluteUnaligned(double x, double y, double z) : JointModelRevoluteUnaligned(Vec3(x, y, z)) {}
};
inline JointModelRevoluteUnaligned JointModelRX() { return JointModelRevoluteUnaligned(1., 0., 0.); }
inline JointModelRevoluteUnaligned JointModelRY() { return JointModelRevoluteUnaligned(0., 1., 0.); }
inline JointModelRevoluteUnaligned JointModelRZ() { return JointModelRevoluteUnaligned(0., 0., 1.); }
// pinocchio::JointModelPrismaticUnaligned(axis): q is a length along the axis
struct JointModelPrismaticUnaligned {
  Vec3 axis;
  explicit JointModelPrismaticUnaligned(const Vec3& a) {
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (n == 0.) throw Exception("Invalid argument: zero joint axis");
    axis = a / n;
  }
  JointModelPrismaticUnaligned(double x, double y, double z) : JointModelPrismaticUnaligned(Vec3(x, y, z)) {}
};
inline JointModelPrismaticUnaligned JointModelPX() { return JointModelPrismaticUnaligned(1., 0., 0.); }
inline JointModelPrismaticUnaligned JointModelPY() { return JointModelPrismaticUnaligned(0., 1., 0.); }
inline JointModelPrismaticUnaligned JointModelPZ() { return JointModelPrismaticUnaligned(0., 0., 1.); }

inline Mat3 skew(const Vec3& w) {
  Mat3 K;
  K(0, 1) = -w[2];
  K(0, 2) = w[1];
  K(1, 0) = w[2];
  K(1, 2) = -w[0];
  K(2, 0) = -w[1];
  K(2, 1) = w[0];
  return K;
}
inline Mat3 rot_axis(const Vec3& ax, double q) {  // Rodrigues
  const Mat3 K = skew(ax), KK = K * K;
  Mat3 R = Mat3::Identity();
  const double s = std::sin(q), c1 = 1. - std::cos(q);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R(i, j) = R(i, j) + s * K(i, j) + c1 * KK(i, j);
  return R;
}
inline Mat3 quat_to_R(double x, double y, double z, double w) {
  Mat3 R;
  R(0, 0) = 1 - 2 * (y * y + z * z);
  R(0, 1) = 2 * (x * y - z * w);
  R(0, 2) = 2 * (x * z + y * w);
  R(1, 0) = 2 * (x * y + z * w);
  R(1, 1) = 1 - 2 * (x * x + z * z);
  R(1, 2) = 2 * (y * z - x * w);
  R(2, 0) = 2 * (x * z - y * w);
  R(2, 1) = 2 * (y * z + x * w);
  R(2, 2) = 1 - 2 * (x * x + y * y);
  return R;
}

// pinocchio::Model stand-in over the subset the device covers: trees of revolute and
// prismatic joints, optionally below a free-flyer root. Joint / frame 0 = universe, as in Pinocchio.
// From a real pinocchio::Model: one joint record per joint from
// model.parents, model.jointPlacements, model.inertias and the joint's axis;
// frames from model.frames (name, parent joint, placement).
class Model {
 public:
  struct Frame {
    std::string name;
    int parent;
    SE3 placement;
  };
  std::vector<std::string> names{"universe"};
  std::vector<int> parents{0};
  std::vector<int> kinds{JOINT_REVOLUTE};
  std::vector<Vec3> axes{Vec3()};
  std::vector<SE3> jointPlacements{SE3()};
  std::vector<Inertia> inertias{Inertia()};
  std::vector<Frame> frames{Frame{"universe", 0, SE3()}};
  Vec3 gravity{0., 0., -9.81};  // Model::gravity981
  std::map<std::string, VectorXd> referenceConfigurations;
  VectorXd defaultState;  // set by the gait builders, as the reference's rmodel.defaultState

  Model() {}
  explicit Model(const JointModelFreeFlyer& root) { addJoint(0, root, SE3(), "root_joint"); }

  int njoints() const { return (int)names.size(); }
  int nq() const {
    int n = 0;
    for (int j = 1; j < njoints(); ++j) n += kinds[j] == JOINT_FREEFLYER ? 7 : 1;
    return n;
  }
  int nv() const {
    int n = 0;
    for (int j = 1; j < njoints(); ++j) n += kinds[j] == JOINT_FREEFLYER ? 6 : 1;
    return n;
  }
  bool has_freeflyer() const { return njoints() > 1 && kinds[1] == JOINT_FREEFLYER; }
  int idx_q(int j) const {
    int n = 0;
    for (int k = 1; k < j; ++k) n += kinds[k] == JOINT_FREEFLYER ? 7 : 1;
    return n;
  }
  int idx_v(int j) const {
    int n = 0;
    for (int k = 1; k < j; ++k) n += kinds[k] == JOINT_FREEFLYER ? 6 : 1;
    return n;
  }

  int addJoint(int parent, const JointModelFreeFlyer&, const SE3& placement, const std::string& name) {
    if (njoints() != 1 || parent != 0)
      throw Exception("Invalid argument: the device path takes a free-flyer as the root joint only");
    return add(parent, JOINT_FREEFLYER, Vec3(), placement, name, 6);
  }
  int addJoint(int parent, const JointModelRevoluteUnaligned& j, const SE3& placement, const std::string& name) {
    return add(parent, JOINT_REVOLUTE, j.axis, placement, name, 1);
  }
  int addJoint(int parent, const JointModelPrismaticUnaligned& j, const SE3& placement, const std::string& name) {
    return add(parent, JOINT_PRISMATIC, j.axis, placement, name, 1);
  }
  void appendBodyToJoint(int joint, const Inertia& I, const SE3& placement = SE3()) {
    inertias.at(joint) = inertias.at(joint) + I.se3Action(placement);
  }
  int addFrame(const std::string& name, int parent_joint, const SE3& placement = SE3()) {
    frames.push_back(Frame{name, parent_joint, placement});
    return (int)frames.size() - 1;
  }
  int getFrameId(const std::string& name) const {
    for (size_t i = 0; i < frames.size(); ++i)
      if (frames[i].name == name) return (int)i;
    throw Exception("Invalid argument: unknown frame " + name);
  }
  bool existFrame(const std::string& name) const {
    for (const Frame& f : frames)
      if (f.name == name) return true;
    return false;
  }
  int getJointId(const std::string& name) const {
    for (size_t i = 0; i < names.size(); ++i)
      if (names[i] == name) return (int)i;
    return njoints();
  }
  // URDF <limit> of a revolute (rad, rad/s) or prismatic (m, m/s) joint (lower/upperPositionLimit, velocityLimit)
  void setJointLimits(int joint, double lower, double upper, double velocity) {
    limits_[joint] = {lower, upper, velocity};
  }
  VectorXd lowerPositionLimit() const { return qlim(0, -INFINITY); }
  VectorXd upperPositionLimit() const { return qlim(1, INFINITY); }
  VectorXd velocityLimit() const {
    VectorXd out(nv(), INFINITY);
    for (int j = 1; j < njoints(); ++j) {
      auto it = limits_.find(j);
      if (kinds[j] != JOINT_FREEFLYER && it != limits_.end()) out[idx_v(j)] = it->second[2];
    }
    return out;
  }
  VectorXd neutral() const {  // pinocchio::neutral
    VectorXd q(nq(), 0.);
    if (has_freeflyer()) q[6] = 1.;
    return q;
  }

  // host kinematics (pinocchio::forwardKinematics / updateFramePlacement / centerOfMass)
  std::vector<SE3> placements(const VectorXd& q) const {
    std::vector<SE3> out(njoints());
    for (int j = 1; j < njoints(); ++j) {
      const int iq = idx_q(j);
      SE3 Mj;
      if (kinds[j] == JOINT_FREEFLYER)
        Mj = SE3(quat_to_R(q[iq + 3], q[iq + 4], q[iq + 5], q[iq + 6]), Vec3(q[iq], q[iq + 1], q[iq + 2]));
      else if (kinds[j] == JOINT_PRISMATIC)
        Mj = SE3(Mat3::Identity(), axes[j] * q[iq]);
      else
        Mj = SE3(rot_axis(axes[j], q[iq]), Vec3());
      out[j] = out[parents[j]] * (jointPlacements[j] * Mj);
    }
    return out;
  }
  SE3 framePlacement(const VectorXd& q, int frame) const {
    const Frame& f = frames.at(frame);
    return placements(q)[f.parent] * f.placement;
  }
  Vec3 centerOfMass(const VectorXd& q) const {
    const std::vector<SE3> oM = placements(q);
    double mt = 0.;
    for (const Inertia& I : inertias) mt += I.mass;
    Vec3 c;
    for (int j = 0; j < njoints(); ++j) {
      const Inertia& I = inertias[j];
      c = c + (oM[j].translation + oM[j].rotation * I.lever) * I.mass;
    }
    return c / mt;
  }

  // gravity(3) armature(nv) then one 27-double record per joint:
  // [type, parent record (-1 universe), axis(3), placement R(9) p(3), mass, CoM(3), I(6)]
  void pack_robot(const VectorXd& armature, VectorXd& out) const {
    for (int i = 0; i < 3; ++i) out.push_back(gravity[i]);
    out.insert(out.end(), armature.begin(), armature.end());
    for (int j = 1; j < njoints(); ++j) {
      out.push_back(kinds[j]);
      out.push_back(parents[j] - 1);
      for (int i = 0; i < 3; ++i) out.push_back(axes[j][i]);
      jointPlacements[j].pack(out);
      const Inertia& I = inertias[j];
      out.push_back(I.mass);
      for (int i = 0; i < 3; ++i) out.push_back(I.lever[i]);
      const Mat3& Ic = I.inertia;
      for (double v : {Ic(0, 0), Ic(1, 1), Ic(2, 2), Ic(0, 1), Ic(0, 2), Ic(1, 2)}) out.push_back(v);
    }
  }
  // the frame payload of costs / contacts: [parent joint record, placement R(9) p(3)]
  void pack_frame(int frame, VectorXd& out) const {
    const Frame& f = frames.at(frame);
    if (f.parent == 0) throw Exception("Invalid argument: frames attached to the universe are not supported");
    out.push_back(f.parent - 1);
    f.placement.pack(out);
  }

 private:
  int add(int parent, int kind, const Vec3& ax, const SE3& placement, const std::string& name, int nvj) {
    if (parent < 0 || parent >= njoints()) throw Exception("Invalid argument: unknown parent joint");
    if (nv() + nvj > kMaxDofs) throw Exception("Invalid argument: the device path holds at most 64 dofs");
    names.push_back(name);
    parents.push_back(parent);
    kinds.push_back(kind);
    axes.push_back(ax);
    jointPlacements.push_back(placement);
    inertias.push_back(Inertia());
    return njoints() - 1;
  }
  VectorXd qlim(int k, double dflt) const {
    VectorXd out(nq(), dflt);
    for (int j = 1; j < njoints(); ++j) {
      auto it = limits_.find(j);
      if (kinds[j] != JOINT_FREEFLYER && it != limits_.end()) out[idx_q(j)] = it->second[k];
    }
    return out;
  }
  std::map<int, std::vector<double> > limits_;
};

// StateMultibody (multibody.hxx:14-34): x = (q, v), nx = nq + nv, ndx = 2 nv
class StateMultibody {
 public:
  explicit StateMultibody(std::shared_ptr<Model> model) : model_(model) {
    nq_ = model->nq();
    nv_ = model->nv();
    const int nq0 = model->has_freeflyer() ? 7 : 1;  // the first joint unbounded (multibody.hxx:23-34)
    const VectorXd lq = model->lowerPositionLimit(), uq = model->upperPositionLimit(), vl = model->velocityLimit();
    lb_ = lq;
    ub_ = uq;
    for (int i = 0; i < nv_; ++i) {
      lb_.push_back(-vl[i]);
      ub_.push_back(vl[i]);
    }
    for (int i = 0; i < nq0 && i < (int)lb_.size(); ++i) {
      lb_[i] = -INFINITY;
      ub_[i] = INFINITY;
    }
  }
  int get_nq() const { return nq_; }
  int get_nv() const { return nv_; }
  int get_nx() const { return nq_ + nv_; }
  int get_ndx() const { return 2 * nv_; }
  const VectorXd& get_lb() const { return lb_; }
  const VectorXd& get_ub() const { return ub_; }
  VectorXd zero() const {
    VectorXd x = model_->neutral();
    x.resize(nq_ + nv_, 0.);
    return x;
  }
  const std::shared_ptr<Model>& get_pinocchio() const { return model_; }

 private:
  std::shared_ptr<Model> model_;
  int nq_, nv_;
  VectorXd lb_, ub_;
};

struct ActuationModelAbstract {
  virtual ~ActuationModelAbstract() {}
  int nu = 0, nun = 0;  // controls; unactuated root dofs (floating base)
  virtual bool floating_base() const = 0;
  // dtau/du of a linear actuation (nv x nu, column-major: the block's actuation record), or
  // null: tau = [0_nun; u]
  virtual const VectorXd* matrix() const { return nullptr; }
  // the squashing part of the actuation record (lb, ub, a: nu entries each; squashing kind 1),
  // or null: none
  virtual const VectorXd* squashing() const { return nullptr; }
};
struct ActuationModelFull : ActuationModelAbstract {  // tau = u
  explicit ActuationModelFull(std::shared_ptr<StateMultibody> state) {
    if (state->get_pinocchio()->has_freeflyer()) throw Exception("Invalid argument: the first joint cannot be a free-flyer");
    nu = state->get_nv();
  }
  bool floating_base() const { return false; }
};
struct ActuationModelFloatingBase : ActuationModelAbstract {  // floating-base.hpp:29-61: tau = [0; u]
  explicit ActuationModelFloatingBase(std::shared_ptr<StateMultibody> state) {
    nun = state->get_pinocchio()->has_freeflyer() ? 6 : 1;
    nu = state->get_nv() - nun;
  }
  bool floating_base() const { return true; }
};

// tau = S u with a constant S = dtau/du (nv x nu, column-major, 1 <= nu <= nv). A project
// extension, not a class of the reference: it plays the part of a user's own
// ActuationModelAbstract subclass whose dtau_du is constant and whose dtau_dx is zero (the
// reference example's ActuationModelDoublePendulum).
struct ActuationModelLinear : ActuationModelAbstract {
  ActuationModelLinear(std::shared_ptr<StateMultibody> state, const VectorXd& S, int nu_) { set(state->get_nv(), S, nu_); }
  bool floating_base() const { return false; }
  const VectorXd* matrix() const { return &S_; }

 protected:
  ActuationModelLinear() {}
  void set(int nv, const VectorXd& S, int nu_) {
    if (nu_ < 1 || nu_ > nv)
      throw Exception("Invalid argument: the device path holds 1 <= nu <= nv (nu = " + std::to_string(nu_) +
                      ", nv = " + std::to_string(nv) + ")");
    if ((int)S.size() != nv * nu_)
      throw Exception("Invalid argument: S has wrong dimension (it should be " + std::to_string(nv) + " x nu)");
    for (double v : S)
      if (!std::isfinite(v)) throw Exception("Invalid argument: S has a non-finite entry");
    nu = nu_;
    S_ = S;
  }
  VectorXd S_;
};
// multicopter-base.hpp: a free-flyer base driven by n_rotors rotor thrusts through tau_f
// (6 x n_rotors, row-major here: one row of the reference's matrix after the other), the other
// joints actuated one to one: nu = nv - 6 + n_rotors, S = [[tau_f, 0], [0, I_{nv-6}]].
struct ActuationModelMultiCopterBase : ActuationModelLinear {
  ActuationModelMultiCopterBase(std::shared_ptr<StateMultibody> state, int n_rotors, const VectorXd& tau_f) {
    if (!state->get_pinocchio()->has_freeflyer()) throw Exception("Invalid argument: the first joint has to be free-flyer");
    if (n_rotors < 0 || (int)tau_f.size() != 6 * n_rotors)
      throw Exception("Invalid argument: tau_f has wrong dimension (it should be 6 x " + std::to_string(n_rotors) + ")");
    const int nv = state->get_nv(), m = nv - 6 + n_rotors;
    if (n_rotors > 6)
      throw Exception("Invalid argument: nu = " + std::to_string(m) + " exceeds nv = " + std::to_string(nv) +
                      ": the device path holds actuations with nu <= nv only");
    VectorXd S((size_t)nv * m, 0.);
    for (int i = 0; i < 6; ++i)
      for (int c = 0; c < n_rotors; ++c) S[(size_t)c * nv + i] = tau_f[(size_t)i * n_rotors + c];
    for (int i = 6; i < nv; ++i) S[(size_t)(n_rotors + i - 6) * nv + i] = 1.;
    set(nv, S, m);
  }
};

// core/actuation/squashing/smooth-sat.hpp: per control
//   s = 0.5 (sqrt((u - lb)^2 + a) - sqrt((u - ub)^2 + a) + lb + ub),  a = (smooth (ub - lb))^2,
// a smooth saturation of u into (lb, ub) with ds/du in (0, 1); smooth defaults to 0.1.
class SquashingModelSmoothSat {
 public:
  SquashingModelSmoothSat(const VectorXd& u_lb, const VectorXd& u_ub, int ns) : ns_(ns), smooth_(0.1) {
    set_bounds(u_lb, u_ub);
  }
  int get_ns() const { return ns_; }
  const VectorXd& get_s_lb() const { return lb_; }
  const VectorXd& get_s_ub() const { return ub_; }
  void set_s_lb(const VectorXd& lb) { set_bounds(lb, ub_); }
  void set_s_ub(const VectorXd& ub) { set_bounds(lb_, ub); }
  double get_smooth() const { return smooth_; }
  void set_smooth(double smooth) {
    if (smooth < 0.) throw Exception("Invalid argument: The smooth value has to be positive");
    smooth_ = smooth;
    set_bounds(lb_, ub_);
  }
  void calc(const VectorXd& u, VectorXd& s) const {
    s.resize(ns_);
    for (int c = 0; c < ns_; ++c)
      s[c] = 0.5 * (std::sqrt((u[c] - lb_[c]) * (u[c] - lb_[c]) + a_[c]) -
                    std::sqrt((u[c] - ub_[c]) * (u[c] - ub_[c]) + a_[c]) + lb_[c] + ub_[c]);
  }
  // the diagonal of ds/du
  void calcDiff(const VectorXd& u, VectorXd& ds_du) const {
    ds_du.resize(ns_);
    for (int c = 0; c < ns_; ++c)
      ds_du[c] = 0.5 * ((u[c] - lb_[c]) / std::sqrt((u[c] - lb_[c]) * (u[c] - lb_[c]) + a_[c]) -
                        (u[c] - ub_[c]) / std::sqrt((u[c] - ub_[c]) * (u[c] - ub_[c]) + a_[c]));
  }
  // lb, ub, a: the record's squashing part
  const VectorXd& packed() const { return packed_; }

 private:
  void set_bounds(const VectorXd& lb, const VectorXd& ub) {
    if ((int)lb.size() != ns_ || (int)ub.size() != ns_)
      throw Exception("Invalid argument: u_lb / u_ub has wrong dimension (it should be " + std::to_string(ns_) + ")");
    for (int c = 0; c < ns_; ++c) {
      if (!std::isfinite(lb[c]) || !std::isfinite(ub[c]))
        throw Exception("Invalid argument: the squashing bounds have a non-finite entry");
      if (!(lb[c] < ub[c])) throw Exception("Invalid argument: the squashing bounds need u_lb < u_ub");
    }
    lb_ = lb;
    ub_ = ub;
    a_.assign(ns_, 0.);
    for (int c = 0; c < ns_; ++c) a_[c] = (smooth_ * (ub[c] - lb[c])) * (smooth_ * (ub[c] - lb[c]));
    packed_ = lb_;
    packed_.insert(packed_.end(), ub_.begin(), ub_.end());
    packed_.insert(packed_.end(), a_.begin(), a_.end());
  }
  int ns_;
  double smooth_;
  VectorXd lb_, ub_, a_, packed_;
};
// core/actuation/actuation-squashing.hpp: tau = actuation(s(u)), here tau = S s(u) with
// dtau/du = S diag(ds/du). The inner actuation is a linear one (its S), or the full / floating-base
// one (S written as the selection matrix). Costs and control limits still act on u.
struct ActuationSquashingModel : ActuationModelAbstract {
  ActuationSquashingModel(std::shared_ptr<StateMultibody> state, std::shared_ptr<ActuationModelAbstract> actuation,
                          std::shared_ptr<SquashingModelSmoothSat> squashing, int nu_)
      : actuation_(actuation), squashing_(squashing) {
    if (actuation->squashing()) throw Exception("Invalid argument: ActuationSquashingModel wraps an unsquashed actuation");
    if (nu_ != actuation->nu)
      throw Exception("Invalid argument: nu has wrong dimension (it should be " + std::to_string(actuation->nu) + ")");
    if (squashing->get_ns() != nu_)
      throw Exception("Invalid argument: ns has wrong dimension (it should be " + std::to_string(nu_) + ")");
    nu = nu_;
    if (!actuation->matrix()) {  // tau = [0; u]: the selection matrix
      const int nv = state->get_nv();
      S_.assign((size_t)nv * nu, 0.);
      for (int c = 0; c < nu; ++c) S_[(size_t)c * nv + (nv - nu + c)] = 1.;
    }
  }
  bool floating_base() const { return false; }
  const VectorXd* matrix() const { return actuation_->matrix() ? actuation_->matrix() : &S_; }
  const VectorXd* squashing() const { return &squashing_->packed(); }
  const std::shared_ptr<ActuationModelAbstract>& get_actuation() const { return actuation_; }
  const std::shared_ptr<SquashingModelSmoothSat>& get_squashing() const { return squashing_; }

 private:
  std::shared_ptr<ActuationModelAbstract> actuation_;
  std::shared_ptr<SquashingModelSmoothSat> squashing_;
  VectorXd S_;
};

// ---- activations (core/activations/*.hpp) ----------------------------------
struct ActivationModelAbstract {
  virtual ~ActivationModelAbstract() {}
  virtual int kind() const = 0;
  virtual int get_nr() const = 0;
  virtual void params(VectorXd& out) const = 0;
};
struct ActivationModelQuad : ActivationModelAbstract {
  int nr;
  explicit ActivationModelQuad(int nr_) : nr(nr_) {}
  int kind() const { return ACT_QUAD; }
  int get_nr() const { return nr; }
  void params(VectorXd& out) const { out.insert(out.end(), nr, 1.); }
};
struct ActivationModelWeightedQuad : ActivationModelAbstract {
  VectorXd weights;
  explicit ActivationModelWeightedQuad(const VectorXd& w) : weights(w) {}
  int kind() const { return ACT_WEIGHTED_QUAD; }
  int get_nr() const { return (int)weights.size(); }
  void params(VectorXd& out) const { out.insert(out.end(), weights.begin(), weights.end()); }
};
// ActivationBounds(lb, ub, beta=1) (quadratic-barrier.hpp:24-68): stored shrunk around the midpoint
struct ActivationBounds {
  VectorXd lb, ub;
  double beta;
  ActivationBounds(const VectorXd& l, const VectorXd& u, double b = 1.) : beta(b) {
    if (l.size() != u.size()) throw Exception("Invalid argument: The lower and upper bounds don't have the same dimension");
    if (b < 0. || b > 1.) throw Exception("Invalid argument: The range of beta is between 0 and 1");
    for (size_t i = 0; i < l.size(); ++i)
      if (std::isfinite(l[i]) && std::isfinite(u[i]) && l[i] > u[i])
        throw Exception("Invalid argument: The lower and upper bounds are badly defined");
    lb.resize(l.size());
    ub.resize(l.size());
    for (size_t i = 0; i < l.size(); ++i) {
      const double m = 0.5 * (l[i] + u[i]), d = 0.5 * (u[i] - l[i]);
      lb[i] = m - b * d;
      ub[i] = m + b * d;
    }
  }
};
struct ActivationModelQuadraticBarrier : ActivationModelAbstract {
  ActivationBounds bounds;
  explicit ActivationModelQuadraticBarrier(const ActivationBounds& b) : bounds(b) {}
  int kind() const { return ACT_QUAD_BARRIER; }
  int get_nr() const { return (int)bounds.lb.size(); }
  void params(VectorXd& out) const {
    out.insert(out.end(), bounds.lb.begin(), bounds.lb.end());
    out.insert(out.end(), bounds.ub.begin(), bounds.ub.end());
  }
};
struct ActivationModelWeightedQuadraticBarrier : ActivationModelAbstract {
  ActivationBounds bounds;
  VectorXd weights;
  ActivationModelWeightedQuadraticBarrier(const ActivationBounds& b, const VectorXd& w) : bounds(b), weights(w) {
    if (w.size() != b.lb.size()) throw Exception("Invalid argument: weight vector has wrong dimension");
  }
  int kind() const { return ACT_WEIGHTED_QUAD_BARRIER; }
  int get_nr() const { return (int)bounds.lb.size(); }
  void params(VectorXd& out) const {
    out.insert(out.end(), bounds.lb.begin(), bounds.lb.end());
    out.insert(out.end(), bounds.ub.begin(), bounds.ub.end());
    out.insert(out.end(), weights.begin(), weights.end());
  }
};

// FrictionCone (friction-cone.hxx:24-96): lb <= A f <= ub, nf facets + the normal row
struct FrictionCone {
  int nf;
  double mu, min_nforce, max_nforce;
  bool inner_appr;
  Vec3 nsurf;
  std::vector<Vec3> A;  // nf + 1 rows
  VectorXd lb, ub;
  FrictionCone(const Vec3& normal = Vec3(0., 0., 1.), double mu_ = 0.7, int nf_ = 4, bool inner = true,
               double fmin = 0., double fmax = DBL_MAX)
      : nf(nf_ % 2 ? 4 : nf_) {
    update(normal, mu_, inner, fmin, fmax);
  }
  void update(const Vec3& normal, double mu_, bool inner, double fmin, double fmax) {
    Vec3 n = normal;
    const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (std::fabs(nn - 1.) > 1e-12) n = n / nn;
    nsurf = n;
    mu = mu_;
    inner_appr = inner;
    min_nforce = fmin >= 0 ? fmin : 0.;
    max_nforce = fmax >= 0 ? fmax : DBL_MAX;
    const double theta = 2. * M_PI / nf;
    if (inner_appr) mu *= std::cos(theta / 2.);
    const Mat3 cRo = from_two_vectors(n, Vec3(0., 0., 1.));
    A.assign(nf + 1, Vec3());
    lb.assign(nf + 1, 0.);
    ub.assign(nf + 1, 0.);
    for (int i = 0; i < nf / 2; ++i) {
      const Vec3 ti(std::cos(theta * i), std::sin(theta * i), 0.);
      const Vec3 a(ti[0], ti[1], -mu + ti[2]), b(-ti[0], -ti[1], -mu - ti[2]);
      for (int c = 0; c < 3; ++c) {  // row vector times cRo
        A[2 * i][c] = a[0] * cRo(0, c) + a[1] * cRo(1, c) + a[2] * cRo(2, c);
        A[2 * i + 1][c] = b[0] * cRo(0, c) + b[1] * cRo(1, c) + b[2] * cRo(2, c);
      }
      lb[2 * i] = lb[2 * i + 1] = -DBL_MAX;
    }
    A[nf] = n;
    lb[nf] = min_nforce;
    ub[nf] = max_nforce;
  }
  // Eigen Quaternion::setFromTwoVectors(a, b) as a rotation matrix; the
  // antiparallel case takes the axis orthogonal to a with the largest norm
  static Mat3 from_two_vectors(const Vec3& a, const Vec3& b) {
    auto unit = [](const Vec3& v) {
      const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      return v / n;
    };
    const Vec3 v0 = unit(a), v1 = unit(b);
    const double c = v1[0] * v0[0] + v1[1] * v0[1] + v1[2] * v0[2];
    double qx, qy, qz, qw;
    if (c < -1. + DBL_EPSILON) {
      Vec3 e(std::fabs(v0[0]) < 0.9 ? 1. : 0., std::fabs(v0[0]) < 0.9 ? 0. : 1., 0.);
      Vec3 ax(v0[1] * e[2] - v0[2] * e[1], v0[2] * e[0] - v0[0] * e[2], v0[0] * e[1] - v0[1] * e[0]);
      ax = unit(ax);
      const double w2 = (1. + std::max(c, -1.)) * 0.5, s = std::sqrt(1. - w2);
      qx = ax[0] * s, qy = ax[1] * s, qz = ax[2] * s, qw = std::sqrt(w2);
    } else {
      const Vec3 ax(v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]);
      const double s = std::sqrt((1. + c) * 2.);
      qx = ax[0] / s, qy = ax[1] / s, qz = ax[2] / s, qw = 0.5 * s;
    }
    return quat_to_R(qx, qy, qz, qw);
  }
};

// ---- frame references (multibody/frames.hpp) --------------------------------
struct FramePlacement {
  int id;
  SE3 placement;
  FramePlacement(int i, const SE3& p) : id(i), placement(p) {}
};
struct FrameTranslation {
  int id;
  Vec3 translation;
  FrameTranslation(int i, const Vec3& p) : id(i), translation(p) {}
};
struct Motion {
  Vec3 linear, angular;
  static Motion Zero() { return Motion(); }
};
enum ReferenceFrame { LOCAL = 0 };
struct FrameMotion {
  int id;
  Motion motion;
  FrameMotion(int i, const Motion& m, ReferenceFrame ref = LOCAL) : id(i), motion(m) {
    if (ref != LOCAL) throw Exception("crocoddyl_amd: frame velocities are covered in the LOCAL frame only");
  }
};
struct FrameForce {
  int id;
  double force[6];
  FrameForce(int i, const double* f) : id(i) {
    for (int k = 0; k < 6; ++k) force[k] = f[k];
  }
};
struct FrameFrictionCone {
  int id;
  FrictionCone cone;
  FrameFrictionCone(int i, const FrictionCone& c) : id(i), cone(c) {}
};
struct FrameRotation {
  int id;
  Mat3 rotation;
  FrameRotation(int i, const Mat3& R) : id(i), rotation(R) {}
};
// FrameCoPSupport(id, support_region) (the reference fork's frames.hpp): the foot's extent
// (L, W) along the contact frame's x and y, centred on the frame origin; A (4 x 6) on the
// wrench (fx, fy, fz, tx, ty, tz): A f >= 0 keeps the centre of pressure (-ty / fz, tx / fz)
// inside the region for fz > 0
struct FrameCoPSupport {
  int id;
  double support_region[2];
  double A[4][6];
  FrameCoPSupport(int i, double L, double W) : id(i) { update_A(L, W); }
  void update_A(double L, double W) {
    if (!(L > 0.) || !(W > 0.)) throw Exception("Invalid argument: the support region's extents have to be positive");
    support_region[0] = L;
    support_region[1] = W;
    const double a[4][6] = {{0., 0., L / 2, 0., -1., 0.},
                            {0., 0., L / 2, 0., 1., 0.},
                            {0., 0., W / 2, 1., 0., 0.},
                            {0., 0., W / 2, -1., 0., 0.}};
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 6; ++c) A[r][c] = a[r][c];
  }
};

// ---- costs (multibody/costs/*.hxx) -----------------------------------------
// A record: [type, weight (set by the sum), activation kind, size] + payload +
// activation parameters.
class CostModelAbstract {
 public:
  CostModelAbstract(std::shared_ptr<StateMultibody> state, std::shared_ptr<ActivationModelAbstract> act, int nr,
                    int nu)
      : state_(state), activation_(act ? act : std::make_shared<ActivationModelQuad>(nr)), nu_(nu) {
    if (activation_->get_nr() != nr) throw Exception("Invalid argument: nr is equals to " + std::to_string(nr));
  }
  virtual ~CostModelAbstract() {}
  virtual int type() const = 0;
  virtual int contact_frame() const { return -1; }  // the frame of a force / cone cost's contact
  // an Impulse* cost: it reads an impulse knot's multipliers / v+ (ActionModelImpulseFwdDynamics only)
  virtual bool impulse_cost() const { return false; }
  int get_nu() const { return nu_; }
  const std::shared_ptr<ActivationModelAbstract>& get_activation() const { return activation_; }
  void pack(double weight, VectorXd& out) const {
    const size_t o = out.size();
    out.insert(out.end(), {(double)type(), weight, (double)activation_->kind(), 0.});
    payload(out);
    activation_->params(out);
    out[o + 3] = (double)(out.size() - o);
  }

 protected:
  virtual void payload(VectorXd& out) const = 0;
  std::shared_ptr<StateMultibody> state_;
  std::shared_ptr<ActivationModelAbstract> activation_;
  int nu_;
};

// r = diff(xref, x) (state.hxx:130-169)
class CostModelState : public CostModelAbstract {
 public:
  CostModelState(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a, const VectorXd& xref,
                 int nu)
      : CostModelAbstract(s, a, s->get_ndx(), nu), xref_(xref) {
    if ((int)xref.size() != s->get_nx()) throw Exception("Invalid argument: xref has wrong dimension");
  }
  CostModelState(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a, const VectorXd& xref)
      : CostModelState(s, a, xref, s->get_nv()) {}
  CostModelState(std::shared_ptr<StateMultibody> s, const VectorXd& xref, int nu)
      : CostModelState(s, nullptr, xref, nu) {}
  int type() const { return COST_STATE; }

 protected:
  void payload(VectorXd& out) const { out.insert(out.end(), xref_.begin(), xref_.end()); }
  VectorXd xref_;
};

// r = u - uref (control.hxx:56-87)
class CostModelControl : public CostModelAbstract {
 public:
  CostModelControl(std::shared_ptr<StateMultibody> s, int nu)
      : CostModelAbstract(s, nullptr, nu, nu), uref_(nu, 0.) {}
  CostModelControl(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a, const VectorXd& uref)
      : CostModelAbstract(s, a, (int)uref.size(), (int)uref.size()), uref_(uref) {}
  CostModelControl(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a)
      : CostModelAbstract(s, a, a->get_nr(), a->get_nr()), uref_(a->get_nr(), 0.) {}
  int type() const { return COST_CONTROL; }

 protected:
  void payload(VectorXd& out) const { out.insert(out.end(), uref_.begin(), uref_.end()); }
  VectorXd uref_;
};

// r = log6(Mref^-1 oMf) (frame-placement.hxx:45-80)
class CostModelFramePlacement : public CostModelAbstract {
 public:
  CostModelFramePlacement(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                          const FramePlacement& Mref, int nu)
      : CostModelAbstract(s, a, 6, nu), Mref_(Mref) {}
  CostModelFramePlacement(std::shared_ptr<StateMultibody> s, const FramePlacement& Mref, int nu)
      : CostModelFramePlacement(s, nullptr, Mref, nu) {}
  int type() const { return COST_FRAME_PLACEMENT; }

 protected:
  void payload(VectorXd& out) const {
    state_->get_pinocchio()->pack_frame(Mref_.id, out);
    Mref_.placement.inverse().pack(out);
  }
  FramePlacement Mref_;
};

// r = oMf.translation - pref (frame-translation.hxx:50-81)
class CostModelFrameTranslation : public CostModelAbstract {
 public:
  CostModelFrameTranslation(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                            const FrameTranslation& xref, int nu)
      : CostModelAbstract(s, a, 3, nu), xref_(xref) {}
  CostModelFrameTranslation(std::shared_ptr<StateMultibody> s, const FrameTranslation& xref, int nu)
      : CostModelFrameTranslation(s, nullptr, xref, nu) {}
  int type() const { return COST_FRAME_TRANSLATION; }

 protected:
  void payload(VectorXd& out) const {
    state_->get_pinocchio()->pack_frame(xref_.id, out);
    for (int i = 0; i < 3; ++i) out.push_back(xref_.translation[i]);
  }
  FrameTranslation xref_;
};

// r = log3(Rref^T oRf) (frame-rotation.hxx); parity unpinned against the reference binary
class CostModelFrameRotation : public CostModelAbstract {
 public:
  CostModelFrameRotation(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                         const FrameRotation& Rref, int nu)
      : CostModelAbstract(s, a, 3, nu), Rref_(Rref) {}
  CostModelFrameRotation(std::shared_ptr<StateMultibody> s, const FrameRotation& Rref, int nu)
      : CostModelFrameRotation(s, nullptr, Rref, nu) {}
  int type() const { return COST_FRAME_ROTATION; }

 protected:
  void payload(VectorXd& out) const {  // Rref^T in the order the placement record keeps Mref^-1's rotation
    state_->get_pinocchio()->pack_frame(Rref_.id, out);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) out.push_back(Rref_.rotation(i, j));
  }
  FrameRotation Rref_;
};

// r = v_f - vref, LOCAL (frame-velocity.hxx:53-84)
class CostModelFrameVelocity : public CostModelAbstract {
 public:
  CostModelFrameVelocity(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                         const FrameMotion& vref, int nu)
      : CostModelAbstract(s, a, 6, nu), vref_(vref) {}
  CostModelFrameVelocity(std::shared_ptr<StateMultibody> s, const FrameMotion& vref, int nu)
      : CostModelFrameVelocity(s, nullptr, vref, nu) {}
  int type() const { return COST_FRAME_VELOCITY; }

 protected:
  void payload(VectorXd& out) const {
    state_->get_pinocchio()->pack_frame(vref_.id, out);
    for (int i = 0; i < 3; ++i) out.push_back(vref_.motion.linear[i]);
    for (int i = 0; i < 3; ++i) out.push_back(vref_.motion.angular[i]);
  }
  FrameMotion vref_;
};

// r = com(q) - cref (com-position.hxx:49-75)
class CostModelCoMPosition : public CostModelAbstract {
 public:
  CostModelCoMPosition(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                       const Vec3& cref, int nu)
      : CostModelAbstract(s, a, 3, nu), cref_(cref) {}
  CostModelCoMPosition(std::shared_ptr<StateMultibody> s, const Vec3& cref, int nu)
      : CostModelCoMPosition(s, nullptr, cref, nu) {}
  int type() const { return COST_COM_POSITION; }

 protected:
  void payload(VectorXd& out) const {
    for (int i = 0; i < 3; ++i) out.push_back(cref_[i]);
  }
  Vec3 cref_;
};

// r = hg(q, v) - href (centroidal-momentum.hxx): [linear; angular about the CoM], world axes;
// Euler knots only. Parity unpinned against the reference binary.
class CostModelCentroidalMomentum : public CostModelAbstract {
 public:
  CostModelCentroidalMomentum(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                              const VectorXd& href, int nu)
      : CostModelAbstract(s, a, 6, nu), href_(href) {
    if (href_.size() != 6) throw Exception("Invalid argument: href has wrong dimension (it should be 6)");
  }
  CostModelCentroidalMomentum(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                              const VectorXd& href)
      : CostModelCentroidalMomentum(s, a, href, s->get_nv()) {}
  CostModelCentroidalMomentum(std::shared_ptr<StateMultibody> s, const VectorXd& href, int nu)
      : CostModelCentroidalMomentum(s, nullptr, href, nu) {}
  CostModelCentroidalMomentum(std::shared_ptr<StateMultibody> s, const VectorXd& href)
      : CostModelCentroidalMomentum(s, nullptr, href, s->get_nv()) {}
  int type() const { return COST_CENTROIDAL_MOMENTUM; }
  const VectorXd& get_href() const { return href_; }
  void set_href(const VectorXd& href) {
    if (href.size() != 6) throw Exception("Invalid argument: href has wrong dimension (it should be 6)");
    href_ = href;
  }

 protected:
  void payload(VectorXd& out) const {
    for (int i = 0; i < 6; ++i) out.push_back(href_[i]);
  }
  VectorXd href_;
};

// r = lambda_contact - fref (contact-force.hxx:33-74); the contact's row offset is
// resolved by the DAM at packing
class CostModelContactForce : public CostModelAbstract {
 public:
  CostModelContactForce(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                        const FrameForce& fref, int nu)
      : CostModelAbstract(s, a, a ? a->get_nr() : 6, nu), fref_(fref) {
    if (activation_->get_nr() != 3 && activation_->get_nr() != 6)
      throw Exception("Invalid argument: nr has to be 3 or 6 (the contact's force)");
  }
  CostModelContactForce(std::shared_ptr<StateMultibody> s, const FrameForce& fref, int nc, int nu)
      : CostModelContactForce(s, std::make_shared<ActivationModelQuad>(nc), fref, nu) {}
  int type() const { return COST_CONTACT_FORCE; }
  int contact_frame() const { return fref_.id; }

 protected:
  void payload(VectorXd& out) const {
    out.push_back(-1.);
    out.push_back(activation_->get_nr());
    out.insert(out.end(), fref_.force, fref_.force + 6);
  }
  FrameForce fref_;
};

// r = A lambda_lin (contact-friction-cone.hxx:51-91)
class CostModelContactFrictionCone : public CostModelAbstract {
 public:
  CostModelContactFrictionCone(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                               const FrameFrictionCone& fref, int nu)
      : CostModelAbstract(s, a, fref.cone.nf + 1, nu), fref_(fref) {}
  CostModelContactFrictionCone(std::shared_ptr<StateMultibody> s, const FrameFrictionCone& fref, int nu)
      : CostModelContactFrictionCone(s, nullptr, fref, nu) {}
  int type() const { return COST_FRICTION_CONE; }
  int contact_frame() const { return fref_.id; }

 protected:
  void payload(VectorXd& out) const {  // [row0 (the DAM's), contact rows (the DAM's), nr, A row-major]
    out.push_back(-1.);
    out.push_back(0.);
    out.push_back((double)fref_.cone.A.size());
    for (const Vec3& r : fref_.cone.A)
      for (int c = 0; c < 3; ++c) out.push_back(r[c]);
  }
  FrameFrictionCone fref_;
};

// r = A lambda of the ContactModel6D on cop_support.id (the reference fork's
// contact-cop-position.hpp); QuadraticBarrier(0, DBL_MAX) by default. Parity unpinned
// against the reference binary.
class CostModelContactCoPPosition : public CostModelAbstract {
 public:
  CostModelContactCoPPosition(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                              const FrameCoPSupport& cop_support, int nu)
      : CostModelAbstract(s, a ? a : default_activation(), 4, nu), cop_support_(cop_support) {}
  CostModelContactCoPPosition(std::shared_ptr<StateMultibody> s, const FrameCoPSupport& cop_support, int nu)
      : CostModelContactCoPPosition(s, nullptr, cop_support, nu) {}
  int type() const { return COST_COP_POSITION; }
  int contact_frame() const { return cop_support_.id; }

 protected:
  static std::shared_ptr<ActivationModelAbstract> default_activation() {
    return std::make_shared<ActivationModelQuadraticBarrier>(ActivationBounds(VectorXd(4, 0.), VectorXd(4, DBL_MAX)));
  }
  void payload(VectorXd& out) const {  // [row0 (the DAM's), contact rows (the DAM's), nr, A row-major]
    out.push_back(-1.);
    out.push_back(0.);
    out.push_back(4.);
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 6; ++c) out.push_back(cop_support_.A[r][c]);
  }
  FrameCoPSupport cop_support_;
};

// ---- the impulse costs: the contact classes' records on the multipliers Lambda of an
// ActionModelImpulseFwdDynamics (nu = 0), and the change of the CoM velocity. Their Jacobians
// (d Lambda / dx = [H^T dtau_dq - S^-1 dv0_dq, -S^-1 Jc], the exact derivative at r_coeff = 0)
// are computed only with enable_force; the CoM cost's do not depend on it. Parity unpinned
// against the reference binary.
// r = Lambda_frame - fref (3 rows on an ImpulseModel3D, 6 on a 6D)
class CostModelContactImpulse : public CostModelContactForce {
 public:
  CostModelContactImpulse(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                          const FrameForce& fref)
      : CostModelContactForce(s, a, fref, 0) {}
  CostModelContactImpulse(std::shared_ptr<StateMultibody> s, const FrameForce& fref, int nr = 6)
      : CostModelContactForce(s, fref, nr, 0) {}
  bool impulse_cost() const { return true; }
};
// r = A Lambda_lin; the cone's barrier by default
class CostModelImpulseFrictionCone : public CostModelContactFrictionCone {
 public:
  CostModelImpulseFrictionCone(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                               const FrameFrictionCone& fref)
      : CostModelContactFrictionCone(s, a ? a : cone_barrier(fref.cone), fref, 0) {}
  CostModelImpulseFrictionCone(std::shared_ptr<StateMultibody> s, const FrameFrictionCone& fref)
      : CostModelImpulseFrictionCone(s, nullptr, fref) {}
  bool impulse_cost() const { return true; }

 private:
  static std::shared_ptr<ActivationModelAbstract> cone_barrier(const FrictionCone& c) {
    return std::make_shared<ActivationModelQuadraticBarrier>(ActivationBounds(c.lb, c.ub));
  }
};
// r = A Lambda of the ImpulseModel6D on cop_support.id; QuadraticBarrier(0, DBL_MAX) by default
class CostModelImpulseCoPPosition : public CostModelContactCoPPosition {
 public:
  CostModelImpulseCoPPosition(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a,
                              const FrameCoPSupport& cop_support)
      : CostModelContactCoPPosition(s, a, cop_support, 0) {}
  CostModelImpulseCoPPosition(std::shared_ptr<StateMultibody> s, const FrameCoPSupport& cop_support)
      : CostModelContactCoPPosition(s, nullptr, cop_support, 0) {}
  bool impulse_cost() const { return true; }
};
// r = Jcom(q) (v+ - v): record 13, an empty payload
class CostModelImpulseCoM : public CostModelAbstract {
 public:
  explicit CostModelImpulseCoM(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActivationModelAbstract> a = nullptr)
      : CostModelAbstract(s, a, 3, 0) {}
  int type() const { return COST_IMPULSE_COM; }
  bool impulse_cost() const { return true; }

 protected:
  void payload(VectorXd&) const {}
};

// CostModelSum (cost-sum.hxx:18-85): named costs in a std::map (evaluated in name order)
class CostModelSum {
 public:
  struct CostItem {
    std::string name;
    std::shared_ptr<CostModelAbstract> cost;
    double weight;
    bool active;
  };
  CostModelSum(std::shared_ptr<StateMultibody> s, int nu) : state_(s), nu_(nu) {}
  explicit CostModelSum(std::shared_ptr<StateMultibody> s) : CostModelSum(s, s->get_nv()) {}
  void addCost(const std::string& name, std::shared_ptr<CostModelAbstract> cost, double weight, bool active = true) {
    if (cost->get_nu() != nu_)
      throw Exception("Invalid argument: " + name + " cost item doesn't have the same control dimension");
    if (costs_.count(name)) throw Exception("Invalid argument: " + name + " cost item already existed");
    costs_[name] = CostItem{name, cost, weight, active};
  }
  void removeCost(const std::string& name) {
    if (!costs_.erase(name)) throw Exception("Invalid argument: " + name + " cost item doesn't exist");
  }
  void changeCostStatus(const std::string& name, bool active) {
    auto it = costs_.find(name);
    if (it == costs_.end()) throw Exception("Invalid argument: " + name + " cost item doesn't exist");
    it->second.active = active;
  }
  CostItem& get(const std::string& name) { return costs_.at(name); }
  const std::map<std::string, CostItem>& get_costs() const { return costs_; }
  int get_nu() const { return nu_; }
  int active_count() const {
    int n = 0;
    for (const auto& kv : costs_) n += kv.second.active ? 1 : 0;
    return n;
  }
  void pack(VectorXd& out) const {
    for (const auto& kv : costs_)
      if (kv.second.active) kv.second.cost->pack(kv.second.weight, out);
  }
  bool has_impulse_cost() const {
    for (const auto& kv : costs_)
      if (kv.second.active && kv.second.cost->impulse_cost()) return true;
    return false;
  }
  // Write row0 (and the rows of a cone / CoP record) of every force cost of the block packed
  // at out[c...]: rows maps a frame to (row0, rows) of the contact / impulse (`what`) on it.
  void resolve_force_rows(VectorXd& out, size_t c, const std::map<int, std::pair<double, int> >& rows,
                          const std::string& what) const {
    for (const auto& kv : costs_) {
      if (!kv.second.active) continue;
      const size_t size = (size_t)out[c + 3];
      const int ty = kv.second.cost->type();
      if (ty == COST_CONTACT_FORCE || ty == COST_FRICTION_CONE || ty == COST_COP_POSITION) {
        auto it = rows.find(kv.second.cost->contact_frame());
        if (it == rows.end())
          throw Exception("Invalid argument: there is not " + what + " defined for a force cost's frame");
        if (ty == COST_CONTACT_FORCE && it->second.second != kv.second.cost->get_activation()->get_nr())
          throw Exception("Invalid argument: the " + what + "-force cost and its " + what + " differ in size");
        if (ty == COST_COP_POSITION && it->second.second != 6)
          throw Exception("Invalid argument: the CoP position cost needs a " +
                          std::string(what == "contact" ? "ContactModel6D" : "ImpulseModel6D") + " on its frame");
        out[c + kCostHdr] = it->second.first;
        if (ty == COST_FRICTION_CONE || ty == COST_COP_POSITION) out[c + kCostHdr + 1] = it->second.second;
      }
      c += size;
    }
  }

 private:
  std::shared_ptr<StateMultibody> state_;
  int nu_;
  std::map<std::string, CostItem> costs_;
};

// ---- contacts (multibody/contacts/*.hxx) ------------------------------------
class ContactModelAbstract {
 public:
  ContactModelAbstract(std::shared_ptr<StateMultibody> s, int frame, int nu, const double* gains)
      : state_(s), frame_(frame), nu_(nu) {
    gains_[0] = gains ? gains[0] : 0.;
    gains_[1] = gains ? gains[1] : 0.;
  }
  virtual ~ContactModelAbstract() {}
  virtual int type() const = 0;
  virtual int get_nc() const = 0;
  int get_nu() const { return nu_; }
  int get_frame() const { return frame_; }
  void pack(VectorXd& out) const {
    const size_t o = out.size();
    out.insert(out.end(), {(double)type(), gains_[0], gains_[1], 0.});
    state_->get_pinocchio()->pack_frame(frame_, out);
    ref_payload(out);
    out[o + 3] = (double)(out.size() - o);
  }

 protected:
  virtual void ref_payload(VectorXd& out) const = 0;
  std::shared_ptr<StateMultibody> state_;
  int frame_, nu_;
  double gains_[2];
};
// ContactModel3D(state, xref, nu, gains) (contact-3d.hxx:12-43)
class ContactModel3D : public ContactModelAbstract {
 public:
  ContactModel3D(std::shared_ptr<StateMultibody> s, const FrameTranslation& xref, int nu, const double* gains = nullptr)
      : ContactModelAbstract(s, xref.id, nu, gains), xref_(xref) {}
  int type() const { return CONTACT_3D; }
  int get_nc() const { return 3; }

 protected:
  void ref_payload(VectorXd& out) const {
    for (int i = 0; i < 3; ++i) out.push_back(xref_.translation[i]);
  }
  FrameTranslation xref_;
};
// ContactModel6D(state, Mref, nu, gains) (contact-6d.hxx:12-45)
class ContactModel6D : public ContactModelAbstract {
 public:
  ContactModel6D(std::shared_ptr<StateMultibody> s, const FramePlacement& Mref, int nu, const double* gains = nullptr)
      : ContactModelAbstract(s, Mref.id, nu, gains), Mref_(Mref) {}
  int type() const { return CONTACT_6D; }
  int get_nc() const { return 6; }

 protected:
  void ref_payload(VectorXd& out) const { Mref_.placement.inverse().pack(out); }
  FramePlacement Mref_;
};
// ContactModelMultiple (multiple-contacts.hxx:14-88): std::map, active rows stacked in name order
class ContactModelMultiple {
 public:
  struct ContactItem {
    std::string name;
    std::shared_ptr<ContactModelAbstract> contact;
    bool active;
  };
  ContactModelMultiple(std::shared_ptr<StateMultibody> s, int nu) : state_(s), nu_(nu) {}
  void addContact(const std::string& name, std::shared_ptr<ContactModelAbstract> c, bool active = true) {
    if (c->get_nu() != nu_)
      throw Exception("Invalid argument: " + name + " contact item doesn't have the same control dimension");
    if (contacts_.count(name)) return;  // the reference warns and keeps the old item
    contacts_[name] = ContactItem{name, c, active};
  }
  void removeContact(const std::string& name) { contacts_.erase(name); }
  void changeContactStatus(const std::string& name, bool active) {
    auto it = contacts_.find(name);
    if (it != contacts_.end()) it->second.active = active;
  }
  int get_nu() const { return nu_; }
  int get_nc() const {
    int n = 0;
    for (const auto& kv : contacts_) n += kv.second.active ? kv.second.contact->get_nc() : 0;
    return n;
  }
  const std::map<std::string, ContactItem>& get_contacts() const { return contacts_; }

 private:
  std::shared_ptr<StateMultibody> state_;
  int nu_;
  std::map<std::string, ContactItem> contacts_;
};

// ---- differential action models ---------------------------------------------
// free-fwddyn.hxx:24-160: a = (M + diag(armature))^-1 (tau(u) - nle), costs(x, u).
// With a floating-base actuation it is the contact knot with no contacts.
class DifferentialActionModelFreeFwdDynamics : public DifferentialActionModelBase {
 public:
  DifferentialActionModelFreeFwdDynamics(std::shared_ptr<StateMultibody> s, std::shared_ptr<ActuationModelAbstract> a,
                                         std::shared_ptr<CostModelSum> costs)
      : state_(s), actuation_(a), costs_(costs), armature_(s->get_nv(), 0.) {
    if (costs->get_nu() != a->nu)
      throw Exception("Invalid argument: Costs doesn't have the same control dimension (it should be " +
                      std::to_string(a->nu) + ")");
  }
  int euler_kind() const {
    return actuation_->floating_base() || actuation_->matrix() ? FDDP_KNOT_EULER_CONTACTFWD : FDDP_KNOT_EULER_FREEFWD;
  }
  int nx() const { return state_->get_nx(); }
  int ndx() const { return state_->get_ndx(); }
  int nu() const { return actuation_->nu; }
  const VectorXd& get_armature() const { return armature_; }
  void set_armature(const VectorXd& a) {
    if ((int)a.size() != state_->get_nv()) throw Exception("Invalid argument: The armature dimension is wrong");
    armature_ = a;
  }
  const std::shared_ptr<CostModelSum>& get_costs() const { return costs_; }
  const std::shared_ptr<StateMultibody>& get_state() const { return state_; }
  void pack_euler(double dt, VectorXd& out) const {
    if (actuation_->matrix()) {  // section flag bit 4: no contacts, then the actuation record
      VectorXd sec{0., 0., 0., 4.};
      pack_actuation(sec);
      pack_mb(dt, sec.data(), sec.size(), out);
    } else if (actuation_->floating_base()) {
      const double sec[4] = {(double)actuation_->nun, 0., 0., 0.};
      pack_mb(dt, sec, 4, out);
    } else {
      pack_mb(dt, nullptr, 0, out);
    }
  }

 protected:
  // [dt, nv, ncost, size] robot, cost records, then the contact / impulse section;
  // returns the offset of the block in `out`
  size_t pack_mb(double dt, const double* sec, size_t nsec, VectorXd& out) const {
    if (costs_->has_impulse_cost())
      throw Exception("Invalid argument: impulse costs need an ActionModelImpulseFwdDynamics");
    const size_t o = out.size();
    out.insert(out.end(), {dt, (double)state_->get_nv(), (double)costs_->active_count(), 0.});
    state_->get_pinocchio()->pack_robot(armature_, out);
    costs_->pack(out);
    if (sec) out.insert(out.end(), sec, sec + nsec);
    out[o + 3] = (double)(out.size() - o);
    return o;
  }
  // the actuation record [20, 0, 0, 4 + nv nu] + S (column-major), after the contact records;
  // squashed: [20, 1, 0, 4 + nv nu + 3 nu] + S + lb + ub + a
  void pack_actuation(VectorXd& sec) const {
    const VectorXd& S = *actuation_->matrix();
    const VectorXd* sq = actuation_->squashing();
    sec.insert(sec.end(), {20., sq ? 1. : 0., 0., (double)(4 + S.size() + (sq ? sq->size() : 0))});
    sec.insert(sec.end(), S.begin(), S.end());
    if (sq) sec.insert(sec.end(), sq->begin(), sq->end());
  }
  std::shared_ptr<StateMultibody> state_;
  std::shared_ptr<ActuationModelAbstract> actuation_;
  std::shared_ptr<CostModelSum> costs_;
  VectorXd armature_;
};

// contact-fwddyn.hxx:24-207: [M Jc^T; Jc 0][a; -lambda] = [tau - nle; -a0]
class DifferentialActionModelContactFwdDynamics : public DifferentialActionModelFreeFwdDynamics {
 public:
  DifferentialActionModelContactFwdDynamics(std::shared_ptr<StateMultibody> s,
                                            std::shared_ptr<ActuationModelFloatingBase> a,
                                            std::shared_ptr<ContactModelMultiple> contacts,
                                            std::shared_ptr<CostModelSum> costs, double inv_damping = 0.,
                                            bool enable_force = false)
      : DifferentialActionModelFreeFwdDynamics(s, a, costs), contacts_(contacts),
        damping_(std::fabs(inv_damping)), enable_force_(enable_force) {
    if (contacts->get_nu() != a->nu) throw Exception("Invalid argument: Contacts doesn't have the same control dimension");
  }
  // (the reference's 1.4.0 signature takes the floating base only; this overload also takes the
  // linear actuations: ActuationModelMultiCopterBase, ActuationModelLinear)
  DifferentialActionModelContactFwdDynamics(std::shared_ptr<StateMultibody> s,
                                            std::shared_ptr<ActuationModelAbstract> a,
                                            std::shared_ptr<ContactModelMultiple> contacts,
                                            std::shared_ptr<CostModelSum> costs, double inv_damping = 0.,
                                            bool enable_force = false)
      : DifferentialActionModelFreeFwdDynamics(s, a, costs), contacts_(contacts),
        damping_(std::fabs(inv_damping)), enable_force_(enable_force) {
    if (!a->floating_base() && !a->matrix())
      throw Exception("Invalid argument: DifferentialActionModelContactFwdDynamics needs an ActuationModelFloatingBase, "
                      "an ActuationModelMultiCopterBase or an ActuationModelLinear");
    if (contacts->get_nu() != a->nu) throw Exception("Invalid argument: Contacts doesn't have the same control dimension");
  }
  int euler_kind() const { return FDDP_KNOT_EULER_CONTACTFWD; }
  const std::shared_ptr<ContactModelMultiple>& get_contacts() const { return contacts_; }
  void pack_euler(double dt, VectorXd& out) const {
    if (contacts_->get_nc() > kMaxContactRows)
      throw Exception("Invalid argument: the device path holds at most 24 contact rows");
    VectorXd sec;
    int nact = 0;
    for (const auto& kv : contacts_->get_contacts())
      if (kv.second.active) ++nact;
    const bool lin = actuation_->matrix() != nullptr;  // flag bit 4: the actuation record after the contacts
    sec.insert(sec.end(), {lin ? 0. : (double)actuation_->nun, damping_, (double)nact,
                           (enable_force_ ? 2. : 0.) + (lin ? 4. : 0.)});
    for (const auto& kv : contacts_->get_contacts())
      if (kv.second.active) kv.second.contact->pack(sec);
    if (lin) pack_actuation(sec);
    const size_t o = pack_mb(dt, sec.data(), sec.size(), out);
    // force / cone costs: the row offset (and rows) of the contact on their frame among
    // the active contacts; an existing but inactive contact has lambda = 0
    std::map<int, std::pair<double, int> > rows;
    int r0 = 0;
    for (const auto& kv : contacts_->get_contacts())
      if (kv.second.active) {
        rows.insert({kv.second.contact->get_frame(), {(double)r0, kv.second.contact->get_nc()}});
        r0 += kv.second.contact->get_nc();
      }
    for (const auto& kv : contacts_->get_contacts())
      if (!kv.second.active)
        rows.insert({kv.second.contact->get_frame(), {kInactiveForceRow, kv.second.contact->get_nc()}});
    const size_t c = o + FDDP_PARAM_HEADER + 3 + state_->get_nv() + kJointRec * (state_->get_pinocchio()->njoints() - 1);
    costs_->resolve_force_rows(out, c, rows, "contact");
  }

 private:
  std::shared_ptr<ContactModelMultiple> contacts_;
  double damping_;
  bool enable_force_;
};

// ---- impulses (multibody/impulses/*.hxx, actions/impulse-fwddyn.hxx) --------
class ImpulseModelAbstract {
 public:
  ImpulseModelAbstract(std::shared_ptr<StateMultibody> s, int frame) : state_(s), frame_(frame) {
    if (frame < 0 || frame >= (int)s->get_pinocchio()->frames.size()) throw Exception("Invalid argument: unknown frame");
  }
  virtual ~ImpulseModelAbstract() {}
  virtual int type() const = 0;
  virtual int get_ni() const = 0;
  int get_frame() const { return frame_; }
  void pack(VectorXd& out) const {
    const size_t o = out.size();
    out.insert(out.end(), {(double)type(), 0., 0., 0.});
    state_->get_pinocchio()->pack_frame(frame_, out);
    out[o + 3] = (double)(out.size() - o);
  }

 protected:
  std::shared_ptr<StateMultibody> state_;
  int frame_;
};
struct ImpulseModel3D : ImpulseModelAbstract {
  ImpulseModel3D(std::shared_ptr<StateMultibody> s, int frame) : ImpulseModelAbstract(s, frame) {}
  int type() const { return CONTACT_3D; }
  int get_ni() const { return 3; }
};
struct ImpulseModel6D : ImpulseModelAbstract {
  ImpulseModel6D(std::shared_ptr<StateMultibody> s, int frame) : ImpulseModelAbstract(s, frame) {}
  int type() const { return CONTACT_6D; }
  int get_ni() const { return 6; }
};
class ImpulseModelMultiple {
 public:
  struct ImpulseItem {
    std::string name;
    std::shared_ptr<ImpulseModelAbstract> impulse;
    bool active;
  };
  explicit ImpulseModelMultiple(std::shared_ptr<StateMultibody> s) : state_(s) {}
  void addImpulse(const std::string& name, std::shared_ptr<ImpulseModelAbstract> i, bool active = true) {
    if (!impulses_.count(name)) impulses_[name] = ImpulseItem{name, i, active};
  }
  void removeImpulse(const std::string& name) { impulses_.erase(name); }
  void changeImpulseStatus(const std::string& name, bool active) {
    auto it = impulses_.find(name);
    if (it != impulses_.end()) it->second.active = active;
  }
  int get_ni() const {
    int n = 0;
    for (const auto& kv : impulses_) n += kv.second.active ? kv.second.impulse->get_ni() : 0;
    return n;
  }
  const std::map<std::string, ImpulseItem>& get_impulses() const { return impulses_; }

 private:
  std::shared_ptr<StateMultibody> state_;
  std::map<std::string, ImpulseItem> impulses_;
};

// ActionModelImpulseFwdDynamics (impulse-fwddyn.hxx:15-127): nu = 0, xnext = (q, v+)
class ActionModelImpulseFwdDynamics : public ActionModelBase {
 public:
  ActionModelImpulseFwdDynamics(std::shared_ptr<StateMultibody> s, std::shared_ptr<ImpulseModelMultiple> impulses,
                                std::shared_ptr<CostModelSum> costs, double r_coeff = 0., double inv_damping = 0.,
                                bool enable_force = false)
      : state_(s), impulses_(impulses), costs_(costs), armature_(s->get_nv(), 0.), r_coeff_(r_coeff),
        damping_(inv_damping), enable_force_(enable_force) {
    if (r_coeff < 0.) throw Exception("Invalid argument: The restitution coefficient has to be positive, set to 0");
    if (inv_damping < 0.) throw Exception("Invalid argument: The damping factor has to be positive, set to 0");
    if (costs->get_nu() != 0) throw Exception("Invalid argument: impulse knots have no controls (CostModelSum(state, 0))");
  }
  int kind() const { return FDDP_KNOT_IMPULSEFWD; }
  int nx() const { return state_->get_nx(); }
  int ndx() const { return state_->get_ndx(); }
  int nu() const { return 0; }
  void set_r_coeff(double r) { r_coeff_ = r; }
  void set_JMinvJt_damping(double d) { damping_ = d; }
  void set_armature(const VectorXd& a) {
    if ((int)a.size() != state_->get_nv()) throw Exception("Invalid argument: The armature dimension is wrong");
    armature_ = a;
  }
  void pack(VectorXd& out) const {
    // the contact classes read a contact's data, which an impulse knot has not (their Impulse*
    // twins read the impulses'); frame velocities and the centroidal momentum are not covered
    // here (an impulse knot runs no kinematics at v)
    for (const auto& kv : costs_->get_costs()) {
      const int ty = kv.second.cost->type();
      if (kv.second.active && ty == COST_CENTROIDAL_MOMENTUM)
        throw Exception("crocoddyl_amd: centroidal-momentum costs on impulse knots are not covered");
      const bool force = ty == COST_CONTACT_FORCE || ty == COST_FRICTION_CONE || ty == COST_COP_POSITION;
      if (kv.second.active && (ty == COST_FRAME_VELOCITY || (force && !kv.second.cost->impulse_cost())))
        throw Exception("crocoddyl_amd: frame-velocity / force costs on impulse knots are not covered");
    }
    if (impulses_->get_ni() > kMaxContactRows) throw Exception("Invalid argument: the device path holds at most 24 impulse rows");
    VectorXd sec;
    int nact = 0;
    for (const auto& kv : impulses_->get_impulses()) nact += kv.second.active ? 1 : 0;
    sec.insert(sec.end(), {r_coeff_, damping_, (double)nact, enable_force_ ? 3. : 1.});
    for (const auto& kv : impulses_->get_impulses())
      if (kv.second.active) kv.second.impulse->pack(sec);
    const size_t o = out.size();
    out.insert(out.end(), {0., (double)state_->get_nv(), (double)costs_->active_count(), 0.});
    state_->get_pinocchio()->pack_robot(armature_, out);
    costs_->pack(out);
    out.insert(out.end(), sec.begin(), sec.end());
    out[o + 3] = (double)(out.size() - o);
    // costs on an impulse's multipliers: the row offset (and rows) of the impulse on their frame
    // among the active impulses, the first match in name order; an existing but inactive
    // impulse has Lambda = 0
    std::map<int, std::pair<double, int> > rows;
    int r0 = 0;
    for (const auto& kv : impulses_->get_impulses())
      if (kv.second.active) {
        rows.insert({kv.second.impulse->get_frame(), {(double)r0, kv.second.impulse->get_ni()}});
        r0 += kv.second.impulse->get_ni();
      }
    for (const auto& kv : impulses_->get_impulses())
      if (!kv.second.active) rows.insert({kv.second.impulse->get_frame(), {kInactiveForceRow, kv.second.impulse->get_ni()}});
    const size_t c = o + FDDP_PARAM_HEADER + 3 + state_->get_nv() + kJointRec * (state_->get_pinocchio()->njoints() - 1);
    costs_->resolve_force_rows(out, c, rows, "impulse");
  }

 private:
  std::shared_ptr<StateMultibody> state_;
  std::shared_ptr<ImpulseModelMultiple> impulses_;
  std::shared_ptr<CostModelSum> costs_;
  VectorXd armature_;
  double r_coeff_, damping_;
  bool enable_force_;
};

}  // namespace crocoddyl_amd

#endif  // CROCODDYL_AMD_MULTIBODY_HPP_
