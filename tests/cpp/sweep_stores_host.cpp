// Host harness of crocoddyl_amd/csrc/sweep_stores.hpp (tests/test_sweep_stores_host.py): the
// bookkeeping the library keeps per handle, driven by event strings as fddp_hip.hip drives it.
//   D / d  fddp_set_debug(h, 1 / 0)         s  a backward launch (stores filled iff debug is on)
//   c  a calcDiff launch    k  fddp_set_knots    l  fddp_set_control_limits
//   K  a change of solver kind    m  fddp_mpc_shift
//   r  a read of FDDP_Q_VXX .. FDDP_Q_QUU_INV: its action is appended to `actions`; a replay is
//      launched as the library does (on_replay)
// Built as a shared object for ctypes, and with -DSWEEP_STORES_MAIN as a stand-alone program
// (for the sanitizers) that runs the issue's sequences itself.
#include <cstdio>
#include <cstring>

#include "../../crocoddyl_amd/csrc/sweep_stores.hpp"

using namespace fddp::stores;

extern "C" int sweep_stores_run(const char* events, int* actions, int cap) {
  SweepStores ss;
  bool debug = false;
  int n = 0;
  for (const char* e = events; *e; ++e) {
    switch (*e) {
      case 'D': debug = true; break;
      case 'd': debug = false; break;
      case 's': ss.on_sweep(debug); break;
      case 'c': case 'k': case 'l': case 'K': case 'm': ss.on_inputs_written(); break;
      case 'r': {
        const Action a = ss.on_read(debug);
        if (a == READ_REPLAY) ss.on_replay();
        if (n < cap) actions[n] = (int)a;
        ++n;
        break;
      }
      default: return -1;
    }
  }
  return n;
}

extern "C" const char* sweep_stores_message() { return overwritten_message(); }

extern "C" long long sweep_stores_doubles(long long B, long long T, long long sN, long long sM, long long sNN,
                                          long long sNM, long long sMM) {
  return store_doubles(B, T, sN, sM, sNN, sNM, sMM);
}

#ifdef SWEEP_STORES_MAIN
int main() {
  struct Case {
    const char* events;
    int n;
    int want[3];
  } cases[] = {
      {"r", 1, {READ_ZEROS}},
      {"kr", 1, {READ_ZEROS}},
      {"sr", 1, {READ_REPLAY}},
      {"Dsr", 1, {READ_COPY}},
      {"scr", 1, {READ_ERROR}},
      {"Dscr", 1, {READ_COPY}},
      {"Dsdcr", 1, {READ_COPY}},
      {"srr", 2, {READ_REPLAY, READ_COPY}},
      {"skr", 1, {READ_ERROR}},
      {"slr", 1, {READ_ERROR}},
      {"sKr", 1, {READ_ERROR}},
      {"smr", 1, {READ_ERROR}},
      {"srsr", 2, {READ_REPLAY, READ_REPLAY}},
      {"srcr", 2, {READ_REPLAY, READ_COPY}},
      {"srcsr", 2, {READ_REPLAY, READ_REPLAY}},
      {"Dsdsr", 1, {READ_REPLAY}},
      {"scsr", 1, {READ_REPLAY}},
  };
  int bad = 0;
  for (const Case& c : cases) {
    int got[3] = {-1, -1, -1};
    const int n = sweep_stores_run(c.events, got, 3);
    bool ok = n == c.n;
    for (int i = 0; ok && i < n; ++i) ok = got[i] == c.want[i];
    if (!ok) {
      std::printf("FAIL %s: %d reads, %d %d %d\n", c.events, n, got[0], got[1], got[2]);
      ++bad;
    }
  }
  if (sweep_stores_run("x", nullptr, 0) != -1) ++bad;
  if (!std::strstr(sweep_stores_message(), "overwritten") || !std::strstr(sweep_stores_message(), "fddp_set_debug(h, 1)"))
    ++bad;
  std::printf("%s\n", bad ? "sweep_stores: FAILED" : "sweep_stores: ok");
  return bad ? 1 : 0;
}
#endif
