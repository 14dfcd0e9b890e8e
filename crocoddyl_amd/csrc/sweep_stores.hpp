// Bookkeeping of the SolverDDP getters' stores (Vxx, Vx, Qxx, Qxu, Quu, Qx, Qu, Quu_inv):
// what fddp_get_quantity does for FDDP_Q_VXX .. FDDP_Q_QUU_INV. Host only, no HIP call: the
// library keeps one SweepStores per handle and tells it what it launches; the CPU tests drive
// the same header through event sequences (tests/test_sweep_stores_host.py).
//
// The stores are filled by a backward sweep whose Dev carries their pointers: every sweep of a
// handle in debug mode (fddp_set_debug), or else a replay of the last sweep (launch mode 2:
// backward_replay_kernel, backward_mfma_replay_kernel), launched at the first read. A replay
// reads what the sweep read (the derivative blocks, fs, the knots' nu, the limits' flags, the box
// QP's free sets, k, and the SweepRec of each element), so it is possible only while all of that
// is in place.
#ifndef CROCODDYL_AMD_SWEEP_STORES_HPP_
#define CROCODDYL_AMD_SWEEP_STORES_HPP_

#include <stdint.h>

namespace fddp {
namespace stores {

enum Action {
  READ_COPY = 0,    // the stores hold what the caller asks for (or debug mode: whatever they hold)
  READ_REPLAY = 1,  // replay the last sweep into the stores, then copy
  READ_ZEROS = 2,   // no sweep has ever run: zeros, as the reference's allocateData leaves them
  READ_ERROR = 3,   // the last sweep's inputs have been overwritten and its values were not stored
};

struct SweepStores {
  bool swept = false;           // a backward sweep has run on the handle
  bool replayable = false;      // every input the last sweep read is still in place
  bool stores_current = false;  // the stores hold the last sweep's values

  // a backward launch (modes 0 and 1), with the stores' pointers in its Dev or without
  void on_sweep(bool with_stores) {
    swept = true;
    replayable = true;
    stores_current = with_stores;
  }
  // anything that writes what a replay reads: a calcDiff launch, fddp_set_knots,
  // fddp_set_control_limits, a change of solver kind, fddp_mpc_shift
  void on_inputs_written() { replayable = false; }
  void on_replay() { stores_current = true; }

  Action on_read(bool debug) const {
    if (debug || stores_current) return READ_COPY;
    if (replayable) return READ_REPLAY;
    if (!swept) return READ_ZEROS;
    return READ_ERROR;
  }
};

inline const char* overwritten_message() {
  return "fddp_get_quantity: the derivatives of the last backward pass have been overwritten (by a calcDiff, "
         "new knots, new control limits, another solver kind or an MPC shift) and its values were not stored; "
         "read before that, or call fddp_set_debug(h, 1), which keeps the stores filled at every pass";
}

// Doubles of the eight stores (fddp_set_debug's sizes): what a first read allocates, zero-filled.
inline int64_t store_doubles(int64_t B, int64_t T, int64_t sN, int64_t sM, int64_t sNN, int64_t sNM, int64_t sMM) {
  return B * (T + 1) * (sNN + sN) + B * T * (sNN + sNM + sMM + sN + sM) + B * T * sMM;
}

}  // namespace stores
}  // namespace fddp

#endif  // CROCODDYL_AMD_SWEEP_STORES_HPP_
