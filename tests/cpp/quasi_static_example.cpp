// SolverFDDP::quasiStatic from C++: the Solo12 trotting problem of trot_example.cpp (its robot
// and gait builders are taken from that file, its program is not), states that differ from knot to
// knot, and the device's quasi-static controls of every running knot: the reference benchmark's
// warm start (quadrupedal-gaits-optctrl.cpp), which the facade could not form before.
//
// usage: quasi_static_example FILE [T]   write T, nx, nu_max (int32), xs ((T + 1) x nx), us (T x
//                                        nu_max, each row cut to its knot's nu and zero-padded)
#define main trot_example_main
#include "trot_example.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s FILE [T]\n", argv[0]);
    return 2;
  }
  (void)&trot_example_main;
  try {
    const int T = argc > 2 ? std::atoi(argv[2]) : 12;
    auto solo = sample_solo12();
    SimpleQuadrupedGaitProblem gait(solo, "FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT");
    const VectorXd x0 = solo->defaultState;
    std::vector<SimpleQuadrupedGaitProblem::Action> models =
        gait.createTrottingModels(x0, 0.15, 0.1, 1e-2, std::max(1, T / 2 - 3), 2);
    models.resize(T);
    auto problem = std::make_shared<croc::ShootingProblem>(x0, models, models.back());
    croc::SolverFDDP solver(problem);
    // the base shifted and the joints bent a little, differently at every knot (the quaternion
    // stays the default state's)
    const int nx = problem->get_nx(), nq = (nx + 1) / 2, m = problem->get_nu_max();
    std::vector<VectorXd> xs(T + 1, x0);
    for (int t = 0; t <= T; ++t) {
      for (int i = 0; i < 3; ++i) xs[t][i] += 0.01 * std::sin(1.0 + t + 2.0 * i);
      for (int i = 7; i < nq; ++i) xs[t][i] += 0.05 * std::sin(0.7 * t + i);
    }
    const std::vector<VectorXd> us = solver.quasiStatic(xs);
    const std::vector<VectorXd> us_T = solver.quasiStatic(std::vector<VectorXd>(xs.begin(), xs.begin() + T));
    if (us.size() != (size_t)T || us_T.size() != (size_t)T) return std::printf("wrong count\n"), 1;
    VectorXd flat;
    for (const auto& x : xs) flat.insert(flat.end(), x.begin(), x.end());
    for (int t = 0; t < T; ++t) {
      if ((int)us[t].size() != models[t]->nu() || us[t] != us_T[t]) return std::printf("knot %d: wrong row\n", t), 1;
      VectorXd row(m, 0.);
      for (size_t i = 0; i < us[t].size(); ++i) row[i] = us[t][i];
      flat.insert(flat.end(), row.begin(), row.end());
    }
    const int32_t dims[3] = {T, nx, m};
    if (!write_all(argv[1], {{dims, sizeof(dims)}, {flat.data(), 8 * flat.size()}})) return 3;
    // the warm start is usable as it stands
    const bool ok = solver.solve(xs, us, 1, false, 1e-9);
    std::printf("quasi-static T=%d nu_max=%d; solved=%d iter=%zu cost=%.12e\n", T, m, ok, solver.get_iter(),
                solver.get_cost());
    return 0;
  } catch (const croc::Exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}
