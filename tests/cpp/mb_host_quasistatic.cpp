// Test harness (CPU), beside mb_host_squashing.cpp: the entry points the quasi-static tests need
// (tests/test_quasi_static_host.py). The device's knot_quasi_static_x under the sequential-lane
// executor, with the block, the configuration and the work area each in a heap allocation of
// exactly its own size (the work area: quasi_static_work_doubles, so that the stand-alone build
// of this file under the host's address sanitizer sees any access beyond it, and any read of the
// state's velocity part); the launch plan's LDS figures for a knot sequence.
//
// With -DQS_MAIN the file is a program of its own: qs_main <in> <out> reads
//   [n, then per case: block doubles, nq, the block, q]   (doubles)
// and writes, per case, nu, the work doubles and u.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../crocoddyl_amd/csrc/mb_quasistatic.hpp"
#include "../../crocoddyl_amd/csrc/launch_plan.hpp"

using namespace fddp::mb;

extern "C" {

// u_out[0..nu) of block P (psz doubles) at the configuration q (nq doubles); returns the work
// area's doubles. nt lanes (the kernel runs kQsThreads).
int64_t qs_host(const double* P, int64_t psz, const double* q, int nq, double* u_out, int nt) {
  std::vector<double> blk(P, P + psz), x(q, q + nq);
  const Blk b = parse(blk.data());
  const int nu = b.nj - b.nun;
  const int64_t wd = quasi_static_work_doubles(b.nj, b.nc, nu);
  std::vector<double> w(wd, 0.), u(nu > 0 ? nu : 1, 0.);
  knot_quasi_static_x(HostExec{nt}, blk.data(), x.data(), u.data(), w.data());
  for (int i = 0; i < nu; ++i) u_out[i] = u[i];
  return wd;
}

// out: nj, nc, nu of a block and the work doubles of that shape
void qs_host_shape(const double* P, int64_t* out) {
  const Blk b = parse(P);
  out[0] = b.nj;
  out[1] = b.nc;
  out[2] = b.nj - b.nun;
  out[3] = quasi_static_work_doubles(b.nj, b.nc, b.nj - b.nun);
}

// plan_lds of a knot sequence: out[0] LdsPlan::qsw, out[1] LdsPlan::qs_smem, out[2] 1 if the
// quasi-static call is refused. Returns 0, or 1 with the plan's refusal in msg.
int qs_host_plan(const fddp_dims* d, const fddp_knot_desc* knots, const double* params, int64_t n_params, int64_t* out,
                 char* msg, int cap) {
  const fddp::plan::Overrides ov;
  const fddp::plan::LdsPlan l = fddp::plan::plan_lds(*d, knots, params, n_params, ov);
  if (l.error) return std::snprintf(msg, cap, "%s", l.error), 1;
  out[0] = l.qsw;
  out[1] = (int64_t)l.qs_smem;
  out[2] = l.qs_error ? 1 : 0;
  return 0;
}
}

#ifdef QS_MAIN
int main(int argc, char** argv) {
  if (argc != 3) return std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]), 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  std::vector<double> in;
  double buf[512];
  for (size_t n; (n = std::fread(buf, sizeof(double), 512, f)) > 0;) in.insert(in.end(), buf, buf + n);
  std::fclose(f);
  std::vector<double> out;
  size_t at = 1;
  for (int c = 0; c < (int)in[0]; ++c) {
    const int64_t psz = (int64_t)in[at];
    const int nq = (int)in[at + 1];
    const double* P = in.data() + at + 2;
    const double* q = P + psz;
    at += 2 + psz + nq;
    int64_t shape[4];
    qs_host_shape(P, shape);
    std::vector<double> u(shape[2] > 0 ? shape[2] : 1);
    const int64_t wd = qs_host(P, psz, q, nq, u.data(), kQsThreads);
    out.push_back((double)shape[2]);
    out.push_back((double)wd);
    out.insert(out.end(), u.begin(), u.begin() + shape[2]);
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return 0;
}
#endif
