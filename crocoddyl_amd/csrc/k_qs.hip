// Quasi-static controls of the multibody running knots (mb_quasistatic.hpp), one 256-thread
// workgroup per (running knot, element): us[b][t] = quasiStatic(model_t, xs[b][t]).
#include "fddp_device.hpp"
#include "ktab.hpp"
#include "mb_quasistatic.hpp"

namespace fddp {

// xs: B x (T + 1) x nx, or null: the element's current candidate states; us: B x T x nu_max.
// Dynamic LDS: the work area (wd doubles), the knot's state, the parameter block.
__global__ __launch_bounds__(mb::kQsThreads) void quasi_static_kernel(Dev D, const double* xs, double* us, int64_t wd) {
  const int t = blockIdx.x, b = blockIdx.y, tid = (int)threadIdx.x;
  const fddp_knot_desc kd = D.knots[t];
  double* uo = us + D.run(b, t) * D.m;
  // a knot without controls (the impulse knots): a zero row. Uniform, and before any barrier.
  if (kd.nu == 0 || kd.kind == FDDP_KNOT_IMPULSEFWD || !is_mb_kind(kd.kind)) {
    for (int e = tid; e < D.m; e += mb::kQsThreads) uo[e] = 0.;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const double* xg = xs ? xs + D.knot(b, t) * D.nx : D.xs[D.st[b].cur] + D.knot(b, t) * D.sX;
  double* xl = sm + wd;
  double* P = xl + pad2(D.nx);
  const double* Pg = D.pblock(b, t);
  const int psz = (int)Pg[3];
  for (int e = tid; e < D.nx; e += mb::kQsThreads) xl[e] = xg[e];
  for (int e = tid; e < psz; e += mb::kQsThreads) P[e] = Pg[e];
  __syncthreads();
  mb::knot_quasi_static_x(mb::DevExec{mb::kQsThreads}, P, lds_ptr(xl), uo, sm);
  for (int e = kd.nu + tid; e < D.m; e += mb::kQsThreads) uo[e] = 0.;
}

namespace ktab {
const void* quasi_static_fn() { return (const void*)quasi_static_kernel; }
hipError_t quasi_static(dim3 grid, size_t smem, hipStream_t s, const Dev& D, const double* xs, double* us, int64_t wd) {
  hipLaunchKernelGGL(quasi_static_kernel, grid, dim3(mb::kQsThreads), smem, s, D, xs, us, wd);
  return hipGetLastError();
}
}  // namespace ktab
}  // namespace fddp
