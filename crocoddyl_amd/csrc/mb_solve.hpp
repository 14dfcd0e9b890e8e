// Multibody knots, the phase executors (DevExec on the device, HostExec for the host
// emulation) and the dense SPD solves: the Gauss-Jordan family, the blocked sweep on the
// matrix cores (gj_mfma), mb_solve and mb_invert.
#pragma once

#include "mb_base.hpp"

namespace fddp {
namespace mb {

// Phase executor: run(f) calls f(lane) for every thread of the workgroup and
// then synchronises (device), or for lanes 0..nt-1 in order (host emulation,
// tests/test_multibody_host.py). Within one phase no lane reads what another
// lane writes, so both orders give the same result. run_w0(f): a phase only
// wave 0 works in, closed by a wave-level fence instead of a workgroup barrier
// (the other waves skip ahead to the next sync()); sync(): the barrier that
// hands wave-0 results back to the whole workgroup.
// Everything the device executor runs is inlined into the kernel: LDS pointers
// keep their address space only through inlining (an outlined phase or helper
// takes them as generic pointers and reaches LDS with flat instructions, at
// global-memory latency).
struct DevExec {
  int nt;
  template <class F>
  __device__ __forceinline__ void run(F f) const {
#if MB_LANE_OPAQUE
    [[clang::always_inline]] f(mb_launder((int)threadIdx.x));
#else
    [[clang::always_inline]] f((int)threadIdx.x);
#endif
    __syncthreads();
  }
  template <class F>
  __device__ __forceinline__ void run_w0(F f) const {
    if (threadIdx.x < 64) {
      [[clang::always_inline]] f((int)threadIdx.x);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __device__ void sync() const { __syncthreads(); }
  // an LDS pointer re-typed through the LDS address space (fddp_device.hpp lds_ptr)
  template <class T>
  __device__ __forceinline__ T* lds(T* p) const {
    return lds_ptr(p);
  }
};
struct HostExec {
  int nt;
  template <class F>
  void run(F f) const {
    for (int l = 0; l < nt; ++l) f(l);
  }
  template <class F>
  void run_w0(F f) const {
    for (int l = 0; l < 64 && l < nt; ++l) f(l);
  }
  void sync() const {}
  template <class T>
  T* lds(T* p) const {
    return p;
  }
};

// Gauss-Jordan on the column-major nr x nc matrix A (ld nr) without pivoting
// (the left nr x nr block is SPD): one column per lane (lane < nc), one pivot
// per phase; the left block's pivot column is only read in its step. Returns
// false if a pivot is not positive. Columns beyond 64 are taken by the same
// lanes in a second pass of each pivot step.
// Runs on wave 0 between wave-level fences; the caller's preceding phase must
// have ended in a workgroup barrier.
// Leading dimension of the nj-row matrices in LDS that are walked column per lane
// (mass matrix / KKT blocks): odd, so a wave's 64 column reads hit distinct banks.
MB_HD __forceinline__ int lda_of(int nj) { return nj | 1; }

// Device version: every thread of the workgroup takes columns tid, tid + nt, ...
// (one pass for nc <= nt), one workgroup barrier per pivot; plain arguments and no
// lambdas, so nothing of it lives in scratch. The column update runs in chunks of 8
// rows, loads first, so the LDS round trips overlap.
__device__ __forceinline__ bool gauss_jordan_dev(double* A, int nr, int ld, int nc, int* flag) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  A = lds_ptr(A);
  flag = lds_ptr(flag);
  __syncthreads();
  bool bad = false;
#pragma unroll 1
  for (int k = 0; k < nr; ++k) {
    const double piv = A[(int64_t)k * ld + k];
    bad = bad || !(piv > 0.);
    const double* pc = A + (int64_t)k * ld;
#pragma unroll 1
    for (int cc = tid; cc < nc; cc += nt) {
      if (cc <= k || bad) continue;
      double* col = A + (int64_t)cc * ld;
      const double akc = col[k] / piv;
      int r0 = 0;
#pragma unroll 1
      for (; r0 + 8 <= nr; r0 += 8) {
        double pv[8], cv[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          pv[r] = pc[r0 + r];
          cv[r] = col[r0 + r];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) col[r0 + r] = (r0 + r == k) ? akc : cv[r] - pv[r] * akc;
      }
#pragma unroll 1
      for (; r0 < nr; ++r0) col[r0] = (r0 == k) ? akc : col[r0] - pc[r0] * akc;
    }
    __syncthreads();
  }
  if (tid == 0) *flag = bad ? 1 : 0;
  __syncthreads();
  return !bad;
}

// v from lane l (uniform l) of the wave, as a scalar
__device__ __forceinline__ double readlane_d(double v, int l) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)bits, l);
  const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Gauss-Jordan with the rows in registers: lane r of every wave holds row r
// (nr <= 64) of the column slabs of CPW columns the wave owns (slab s of wave w:
// columns (w + s nw) CPW ..); per pivot k the wave owning column k publishes it
// through LDS (pb: 2 x 64 doubles, double-buffered, so one barrier per pivot), the
// pivot row comes from lane k by readlane. The pivot loop runs in chunks of CPW
// unrolled steps, so the owner's register of column k is static. No LDS traffic
// beyond the one published column per pivot. Returns false if a pivot is not
// positive (the LLT failure the reference reports).
// id0: A's columns from id0 on start as an identity block ([M | I]); their slabs
// are skipped until the pivot reaches them (the update is the identity there too).
template <int CPW, int SPW>
__device__ __forceinline__ bool gauss_jordan_rows(double* A, int nr, int ld, int nc, double* pb, int* flag,
                                                  int id0 = 1 << 30) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
  const int nslab = (nc + CPW - 1) / CPW;
  A = lds_ptr(A);
  pb = lds_ptr(pb);
  flag = lds_ptr(flag);
  double v[SPW][CPW];
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SPW; ++s) {
    const int slab = wave + s * nw;
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int c = slab * CPW + j;
      v[s][j] = (lane < nr && slab < nslab && c < nc) ? A[(int64_t)c * ld + lane] : 0.;
    }
  }
  bool bad = false;
#pragma unroll 1
  for (int kk = 0; kk < nr; kk += CPW) {
    const int kslab = kk / CPW, owner = kslab % nw, os = kslab / nw;
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int k = kk + j;
      if (k >= nr) continue;  // (uniform)
      double* pcol = pb + (k & 1) * 64;
      if (wave == owner) {
        double val = 0.;
#pragma unroll
        for (int s = 0; s < SPW; ++s)
          if (s == os) val = v[s][j];
        pcol[lane] = val;
      }
      __syncthreads();
      const double piv = pcol[k];
      const double ark = pcol[lane];  // A[r][k] of this lane's row
      bad = bad || !(piv > 0.);
      const double ipiv = 1. / piv;
#pragma unroll
      for (int s = 0; s < SPW; ++s) {
        // a slab left of the pivot holds unit columns (row k zero): the update is the
        // identity there, so it is skipped (wave-uniform)
        const int slab = wave + s * nw;
        if (slab >= nslab || slab * CPW + CPW <= k || slab * CPW - id0 > k) continue;
#pragma unroll
        for (int jj = 0; jj < CPW; ++jj) {
          const double akc = readlane_d(v[s][jj], k) * ipiv;  // pivot row, scaled
          v[s][jj] = lane == k ? akc : v[s][jj] - ark * akc;
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < SPW; ++s) {
    const int slab = wave + s * nw;
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int c = slab * CPW + j;
      if (lane < nr && slab < nslab && c < nc) A[(int64_t)c * ld + lane] = v[s][j];
    }
  }
  if (tid == 0) *flag = bad ? 1 : 0;
  __syncthreads();
  return !bad;
}

// the device executor takes the register version when the slabs fit (overload
// resolution prefers these to the template below, which serves the host emulation)
// The slab count per wave follows nc (the block is uniform): every unrolled register
// column costs a readlane pair and an FMA per pivot, so the [M | Jc^T | r] block of
// the calc (nc = nj + nc + 1) and the small Schur block do not pay for the 3 slabs
// per wave that the calcDiff's [M | I] needs.
// SPW: the call site's bound on the slabs per wave (one instantiation per call site
// keeps the register budget of the kernels it is inlined into); blocks wider than
// SPW slabs per wave take the LDS version.
template <int SPW>
__device__ __forceinline__ bool gauss_jordan_regs(double* A, int nr, int ld, int nc, int* flag, double* pb,
                                                  int id0 = 1 << 30) {
  if (nr <= 64 && nc <= SPW * 8 * (int)(blockDim.x >> 6)) return gauss_jordan_rows<8, SPW>(A, nr, ld, nc, pb, flag, id0);
  return gauss_jordan_dev(A, nr, ld, nc, flag);
}
template <int SPW>
__device__ __forceinline__ bool gauss_jordan(const DevExec&, double* A, int nr, int ld, int nc, int* flag,
                                             double* pb, int id0 = 1 << 30) {
  return gauss_jordan_regs<SPW>(A, nr, ld, nc, flag, pb, id0);
}

// no side work for the idle waves of gj_mfma
struct GjNoSide {
  __device__ void operator()(int, int, int) const {}
};
#if defined(__HIP_DEVICE_COMPILE__)
// Blocked Gauss-Jordan on the fp64 matrix cores. A: nr x nc column-major in LDS (ld),
// its left nr x nr block SPD. Pivot blocks of 16 rows; per block k:
//  A  every wave inverts the diagonal block D itself, in registers (the symmetric sweep:
//     a_pp <- -1/a_pp, a_ip <- a_ip/a_pp, a_pj <- a_pj/a_pp, a_ij <- a_ij - a_ip a_pj/a_pp;
//     after all 16 pivots N = -D^-1), so no barrier separates it from B;
//  B  the wave owning column tile j (j mod nw) forms R_j = N A_kj = -D^-1 A_kj and updates
//     its whole column: A_ij += A_ik R_j (i != k), A_kj <- -R_j (v_mfma_f64_16x16x4_f64);
//  C  (inverse) the diagonal column block, A_ik <- A_ik N, A_kk <- -N, deferred to its
//     owner's next pass (nobody else reads it before then): one workgroup barrier per
//     pivot block instead of one per pivot.
// N's registers serve as both MFMA operands: lane (i = lane & 15, g = lane >> 4) holds
// N[i][g + 4q], q = 0..3, which is the A fragment of k-chunk q (k = g + 4q) and, N being
// symmetric, the B fragment too; R_j's accumulators are the B fragments of the update
// with the same k order. Columns: the right-hand sides start at the 16-aligned virtual
// column nrp (their tiles never share a tile with the matrix). The pivots are the LDL^T
// pivots in order, so a non-positive one is the LLT failure the unblocked sweep reports.
// inverse: the left block becomes M^-1 in place; the right-hand sides M^-1 B either way.
// side(slot, lane, nlanes): independent work of the caller for the waves that own no
// column tile (wave >= nct), one slot per barrier interval (nbr + 1 of them), so the
// latency-bound pivot chain of the owners hides it.
template <class Side = GjNoSide>
__device__ __forceinline__ bool gj_mfma(double* A_, int nr, int ld, int nc, bool inverse, int* flag,
                                        Side side = Side{}) {
  typedef __attribute__((address_space(3))) double lds_d;
  typedef double f64x4 __attribute__((ext_vector_type(4)));
  lds_d* A = (lds_d*)lds_ptr(A_);
  // the shape in scalar registers (the callers read it from the LDS parameter block, i.e.
  // into vector registers): the sweep's `r0 + p < nr` then skips the padding pivots of the
  // last block by a scalar branch instead of running all 16 under a lane mask
  nr = __builtin_amdgcn_readfirstlane(nr);
  ld = __builtin_amdgcn_readfirstlane(ld);
  nc = __builtin_amdgcn_readfirstlane(nc);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int nrp = (nr + 15) & ~15, nbr = nrp >> 4, nct = (nrp + nc - nr + 15) >> 4;
  auto phys = [&](int v) { return v < nr ? v : (v < nrp ? -1 : v - nrp + nr); };
  // branch-free guarded load: an in-range address always, the value selected
  auto at = [&](int r, int c) -> double {
    const bool v = r < nr && c >= 0 && c < nc;
    const double x = A[(v ? r : 0) + ld * (v ? c : 0)];
    return v ? x : 0.;
  };
  // Without side work or the inverse's trailing column updates (mb_solve), the per-step
  // workgroup barrier is replaced by a progress counter: step k + 1 needs tile k + 1 as
  // updated by step k (its sweep reads the diagonal block, every wave's update its
  // column), and nothing else another wave writes — a pivot tile is never written again
  // once passed — so only its owner is waited for, and the other waves' updates of the
  // later tiles overlap the next sweep.
  constexpr bool kNoSide = std::is_same<Side, GjNoSide>::value;
  const bool flagged = kNoSide && !inverse;
  int* prog = flag + 1;   // diagonal block of tile k ready (its sweep may start)
  int* prog2 = flag + 2;  // all of tile k ready (the updates may read it)
  if (flagged && tid == 0) *prog = *prog2 = 0;
  __syncthreads();
  MB_GJ_MARK(0);
  bool bad = false;
  double Np[4] = {0., 0., 0., 0.};
  // C: column block kc <- A_ik N (i != kc), the diagonal block <- -N
  auto col_update = [&](int kc, const double* N) {
    const int c = 16 * kc + li;
#pragma unroll 1
    for (int i = 0; i < nbr; ++i) {
      if (i == kc) continue;
      f64x4 acc = {0., 0., 0., 0.};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int kk = 16 * kc + lk + 4 * q;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(at(16 * i + li, kk < nr ? kk : -1), N[q], acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = 16 * i + lk + 4 * q;
        if (r < nr && c < nr) A[r + ld * c] = acc[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 16 * kc + li, cc = 16 * kc + lk + 4 * q;
      if (r < nr && cc < nr) A[r + ld * cc] = -N[q];
    }
  };
#pragma unroll 1
  for (int k = 0; k < nbr; ++k) {
    const int r0 = 16 * k;
    double d[4] = {0., 0., 0., 0.};
    if (flagged && k > 0 && wave < nct) {  // tile k updated through step k - 1
      lds_wait_ge(prog, k);
      asm volatile("" ::: "memory");
    }
    // A: only the waves that own a column tile need N (one sweep per SIMD, not two);
    // the padding pivots beyond nr are skipped (their identity rows stay +1, which only
    // ever multiplies the zero-loaded padding)
    if (wave < nct) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = lk + 4 * q;
        const double x = at(r0 + li, r0 + c < nr ? r0 + c : -1);
        d[q] = (r0 + li < nr && r0 + c < nr) ? x : (li == c ? 1. : 0.);
      }
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        if (r0 + p < nr) {  // (uniform; the loop stays fully unrolled, d[] static)
          const int pq = p >> 2, pg = p & 3;
          const double app = readlane_d(d[pq], p + 16 * pg);
          const double aip = row_to_all_d(d[pq], pg);  // = __shfl(d[pq], li + 16 pg)
          double apc[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) apc[q] = row_bcast_d(d[q], p);  // = __shfl(d[q], p + 16 lk)
          bad = bad || !(app > 0.);
          // 1 / app from v_rcp_f64 (relative error up to ~2^-23) corrected to working
          // precision in three dependent fmas: with e = 1 - app x0, x0 (1 + e + e^2) has
          // relative error e^3 (one Newton step leaves e^2 ~ 1e-14, which the contact
          // KKT's conditioning, ~1e7, turned into 1e-7 trajectory errors). The pivot chain
          // is latency-bound (35 cycles per dependent f64 op), so not the IEEE division's
          // special-case scaling: app > 0 is all that is used.
          double ip = __builtin_amdgcn_rcp(app);
          {
            const double e = __builtin_fma(-app, ip, 1.);
            ip = __builtin_fma(ip, __builtin_fma(e, e, e), ip);
          }
          const double t = aip * ip;
          // row p: a_pc ip; the others: a_ic - t a_pc (one fma with per-lane factors);
          // column p (register pq of the lanes with lk == pg): t, the pivot itself -ip
          const bool rp = li == p;
          const double sf = rp ? ip : -t;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double v = __builtin_fma(sf, apc[q], rp ? 0. : d[q]);
            d[q] = (q == pq && lk == pg) ? (rp ? -ip : t) : v;
          }
        }
      }
    }
    MB_GJ_MARK(1 + 3 * k);
    if (flagged && k > 0 && wave < nct) {  // all of tile k updated through step k - 1
      lds_wait_ge(prog2, k);
      asm volatile("" ::: "memory");
    }
#pragma unroll 1
    for (int j = wave; j < nct; j += nw) {
      if (inverse && j == k - 1) col_update(j, Np);
      if (j == k || (!inverse && j < k)) continue;
      const int pc = phys(16 * j + li);
      f64x4 R = {0., 0., 0., 0.};
#pragma unroll
      for (int q = 0; q < 4; ++q) R = __builtin_amdgcn_mfma_f64_16x16x4f64(d[q], at(r0 + lk + 4 * q, pc), R, 0, 0, 0);
      // row blocks from k + 1 on (rotated): the next pivot tile's diagonal block first
#pragma unroll 1
      for (int ii = 0; ii < nbr; ++ii) {
        const int i = ii + k + 1 < nbr ? ii + k + 1 : ii + k + 1 - nbr;
        if (i == k) continue;
        f64x4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = at(16 * i + lk + 4 * q, pc);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int kk = r0 + lk + 4 * q;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(at(16 * i + li, kk < nr ? kk : -1), R[q], acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 16 * i + lk + 4 * q;
          if (r < nr && pc >= 0 && pc < nc) A[r + ld * pc] = acc[q];
        }
        if (flagged && j == k + 1 && i == k + 1) {  // the next sweep's block is ready
          if (lane == 0) lds_publish(prog, k + 1);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + lk + 4 * q;
        if (r < nr && pc >= 0 && pc < nc) A[r + ld * pc] = -R[q];
      }
      if (flagged && j == k + 1) {  // the whole next pivot tile is ready
        if (lane == 0) lds_publish(prog2, k + 1);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Np[q] = d[q];
    if (wave >= nct) side(k, tid - 64 * nct, (nw - nct) * 64);
    MB_GJ_MARK(2 + 3 * k);
    if (!flagged) __syncthreads();
    MB_GJ_MARK(3 + 3 * k);
  }
  if (inverse)
    for (int j = wave; j < nct; j += nw)
      if (j == nbr - 1) col_update(j, Np);
  if (wave >= nct) side(nbr, tid - 64 * nct, (nw - nct) * 64);
  if (tid == 0) *lds_ptr(flag) = bad ? 1 : 0;
  __syncthreads();
  MB_GJ_MARK(20);
  return !bad;
}
#endif

// whether mb_invert works in place (then [M | I] needs no identity half)
__device__ __forceinline__ constexpr bool mb_inv_inplace(const DevExec&) {
#if defined(__HIP_DEVICE_COMPILE__)
  return true;
#else
  return false;
#endif
}
// [M | B] (nr x nc, M SPD) -> M^-1 B in the columns beyond M (the left block is consumed)
__device__ __forceinline__ bool mb_solve(const DevExec&, double* A, int nr, int ld, int nc, int* flag, double* pb) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)pb;
  return gj_mfma(A, nr, ld, nc, false, flag);
#else
  return gauss_jordan_regs<2>(A, nr, ld, nc, flag, pb);
#endif
}
// [M | I] (nr x 2 nr, M SPD) -> M^-1, at *Minv (device: in place of M). side: work the
// idle waves run meanwhile (gj_mfma); *nslots: the slots it ran (0: none)
template <class Side = GjNoSide>
__device__ __forceinline__ bool mb_invert(const DevExec&, double* A, int nr, int ld, int* flag, double* pb,
                                          double** Minv, Side side = Side{}, int* nslots = nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)pb;
  *Minv = A;
  const int nbr = (nr + 15) >> 4, nw = (int)(blockDim.x >> 6);
  if (nslots) *nslots = nw > nbr ? nbr + 1 : 0;
  return gj_mfma(A, nr, ld, nr, true, flag, side);
#else
  (void)side;
  if (nslots) *nslots = 0;
  *Minv = A + (int64_t)ld * nr;
  return gauss_jordan_regs<3>(A, nr, ld, 2 * nr, flag, pb, nr);
#endif
}

template <int SPW, class X>
MB_HD __attribute__((noinline)) bool gauss_jordan(const X& ex, double* A, int nr, int ld, int nc, int* flag,
                                                 double* = nullptr, int = 0) {
  ex.run_w0([&](int lane) {
    if (lane == 0) *flag = 0;
  });
#pragma unroll 1
  for (int k = 0; k < nr; ++k) {
    ex.run_w0([&](int lane) {
      const double piv = A[(int64_t)k * ld + k];
      if (!(piv > 0.)) {
        if (lane == 0) *flag = 1;
        return;
      }
#pragma unroll 1
      for (int cc = lane; cc < nc; cc += 64) {
        if (cc <= k) continue;
        // pivot column and own column in chunks of 8 rows through registers
        // (independent loads, then the updates): no LDS round trip per row
        double* col = A + (int64_t)cc * ld;
        const double* pc = A + (int64_t)k * ld;
        const double akc = col[k] / piv;
#pragma unroll 1
        for (int r0 = 0; r0 < nr; r0 += 8) {
          double pv[8], cv[8];
#pragma unroll
          for (int r = 0; r < 8; ++r)
            if (r0 + r < nr) {
              pv[r] = pc[r0 + r];
              cv[r] = col[r0 + r];
            }
#pragma unroll
          for (int r = 0; r < 8; ++r)
            if (r0 + r < nr) col[r0 + r] = (r0 + r == k) ? akc : cv[r] - pv[r] * akc;
        }
      }
    });
  }
  ex.sync();
  return *flag == 0;
}
// the host emulation (and any other executor): the unblocked sweep on [M | B], [M | I]
template <class X>
MB_HD __forceinline__ constexpr bool mb_inv_inplace(const X&) {
  return false;
}
template <class X>
MB_HD __forceinline__ bool mb_solve(const X& ex, double* A, int nr, int ld, int nc, int* flag, double* pb) {
  return gauss_jordan<2>(ex, A, nr, ld, nc, flag, pb);
}
template <class X, class Side = int>
MB_HD __forceinline__ bool mb_invert(const X& ex, double* A, int nr, int ld, int* flag, double* pb, double** Minv,
                                     Side = Side{}, int* nslots = nullptr) {
  if (nslots) *nslots = 0;
  *Minv = A + (int64_t)ld * nr;
  return gauss_jordan<3>(ex, A, nr, ld, 2 * nr, flag, pb, nr);
}

}  // namespace mb
}  // namespace fddp
