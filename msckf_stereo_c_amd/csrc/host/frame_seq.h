// frame_seq.h — what the two frame sequences (ImageProcessor::runFrame, MsckfVio::runFrame) share with their callers: the phase
// indices of the accounting, the per-stream executor and the lap timer.
#pragma once
#include <chrono>
#include <functional>

namespace cg {

// phases of the front-end thread: PH_IMU .. PH_FE_QWAIT (without PH_EKF_*); of the filter thread: PH_EKF_QWAIT, PH_IMU_EKF, PH_EKF_A .. PH_POSVAR, PH_DIRECT (the direct updates' batches and their waits)
enum { PH_PUSH = 0, PH_PREP1, PH_TRACK1, PH_AFTER1, PH_TRACK2, PH_AFTER2, PH_EKF_A, PH_UPD1, PH_EKF_B, PH_UPD2, PH_EKF_C, PH_POSVAR, PH_IMU,
       PH_HANDOFF, PH_FE_QWAIT, PH_EKF_QWAIT, PH_IMU_EKF, PH_DIRECT, PH_COUNT };

// runs fn(i) for i in [0, n) and returns when all are done (a BatchGroup passes its ForkJoin); empty: a plain loop
typedef std::function<void(int, const std::function<void(int)> &)> ParFor;
inline void par_for(const ParFor &par, int n, const std::function<void(int)> &fn) { if (par) par(n, fn); else for (int i = 0; i < n; ++i) fn(i); }

// lap(ph): the wall seconds since the last lap go to acc[ph]; acc == nullptr: no accounting
struct PhaseLaps {
    double *acc;
    std::chrono::steady_clock::time_point tp;
    explicit PhaseLaps(double *a) : acc(a) { if (acc) tp = std::chrono::steady_clock::now(); }
    void operator()(int ph) { if (!acc) return; const auto t2 = std::chrono::steady_clock::now(); acc[ph] += std::chrono::duration<double>(t2 - tp).count(); tp = t2; }
};

// a failed C-ABI call inside a sequence: its name is the error text, its status the return value
#define FRAME_CHK(fn, args) do { const int rc_ = fn args; if (rc_ != MSKF_OK) { err = #fn; return rc_; } } while (0)

}  // namespace cg
