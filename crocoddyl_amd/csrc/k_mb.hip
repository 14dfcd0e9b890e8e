// Multibody knot kernels (fddp_kernels.hpp mb_knot_kernel*), one variant per object:
// the Makefile compiles this file once per FDDP_TU_MB = ktab::MB_W2 .. MB_S2.
#ifndef FDDP_TU_MB
#error "k_mb.hip is compiled with -DFDDP_TU_MB=<variant>"
#endif
// the spilled-plan kernel (MB_S2: the large trees, two workgroups per CU) takes the shape
// arguments of the calcDiff's matrix-core products as scalars (multibody.hpp
// MB_MFMA_SCALAR_SHAPE): C5 calcDiff 25.40 -> 24.69 ms; measured neutral on the 128-thread
// kernel and 0.5 % slower on the 256-thread all-LDS kernel, which keep the vector arguments
#if FDDP_TU_MB == 4
#define MB_MFMA_SCALAR_SHAPE 1
// the spilled-plan kernel is built without the actuation record's phases (mb_base.hpp
// MB_ACTUATION): its code stays what the headline runs, and the launch plan gives a horizon with
// such a record the all-LDS plan, whose objects carry them (launch_plan.hpp plan_lds)
#define MB_ACTUATION 0
// ... and without the prismatic joint records (MB_PRISMATIC), routed the same way
#define MB_PRISMATIC 0
#endif
// (the rollout objects' MB_BLK_UNIFORM and MB_LANE_OPAQUE, k_fwd.hip, stay off in these
// objects: on the MB_S2 kernel they cost C5 calcDiff 24.0 -> 24.6 and 24.8 ms; that object
// is only built without the backend's loop-invariant code motion, csrc/Makefile)
#include "fddp_kernels.hpp"
#include "ktab.hpp"
static_assert(fddp::ktab::MB_S2 == 4, "MB_MFMA_SCALAR_SHAPE is set for the MB_S2 object");

namespace fddp {
namespace ktab {

namespace {
#if FDDP_TU_MB == 0
constexpr int kThreads = mb::kMbDiffNT;
const void* const kFn = (const void*)mb_knot_kernel;
#define MB_KERNEL mb_knot_kernel
#elif FDDP_TU_MB == 1
constexpr int kThreads = mb::kMbDiffNT;
const void* const kFn = (const void*)mb_knot_kernel_w1;
#define MB_KERNEL mb_knot_kernel_w1
#elif FDDP_TU_MB == 2
constexpr int kThreads = mb::kMbDiffNT / 2;
const void* const kFn = (const void*)mb_knot_kernel_x2;
#define MB_KERNEL mb_knot_kernel_x2
#elif FDDP_TU_MB == 3
constexpr int kThreads = 2 * mb::kMbDiffNT;
const void* const kFn = (const void*)mb_knot_kernel_x8;
#define MB_KERNEL mb_knot_kernel_x8
#else
constexpr int kThreads = mb::kMbDiffNT;
const void* const kFn = (const void*)mb_knot_kernel_s2;
#define MB_KERNEL mb_knot_kernel_s2
#endif
}  // namespace

#define MB_CAT2(a, b) a##b
#define MB_CAT(a, b) MB_CAT2(a, b)
// per-variant entry points, dispatched by ktab::mb_knot* in fddp_hip.hip
int MB_CAT(mb_knot_threads_, FDDP_TU_MB)() { return kThreads; }
const void* MB_CAT(mb_knot_fn_, FDDP_TU_MB)() { return kFn; }
hipError_t MB_CAT(mb_knot_, FDDP_TU_MB)(dim3 grid, size_t smem, hipStream_t s, const Dev& D, int sel_calc,
                                        int sel_diff) {
  hipLaunchKernelGGL(MB_KERNEL, grid, dim3(kThreads), smem, s, D, sel_calc, sel_diff);
  return hipGetLastError();
}

}  // namespace ktab
}  // namespace fddp
