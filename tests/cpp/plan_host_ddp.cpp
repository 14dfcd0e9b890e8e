// Test harness (CPU), beside mb_host.cpp: the launch-plan rule the DDP solver kinds add
// (launch_plan.hpp rollout_for_kind), as the library evaluates it at every rollout launch
// (tests/test_ddp_plan_host.py).
#include "../../crocoddyl_amd/csrc/launch_plan.hpp"

extern "C" {

// the rollout variant (ktab::FWD_*) a handle planned onto `fwd` launches under `solver_kind`
int plan_host_rollout_for_kind(int fwd, int solver_kind) { return fddp::plan::rollout_for_kind(fwd, solver_kind); }

// whether the three-workgroups-per-CU multibody rollout is built with the DDP mode
int plan_host_mb3_has_ddp(void) { return FDDP_FWD_DDP_MB3; }
}
