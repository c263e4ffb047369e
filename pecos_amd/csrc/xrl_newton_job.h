// What K16 (xrl_newton.hip) and K16D (xrl_newton_dense.hip: the same solver over a dense X) share on the device side: a launch's arguments,
// the order of the counters the wavefronts sum, and the test of an fp64 scalar.
#pragma once
#include "xrl_newton.h"
#include "xrl_train_job.h"

namespace xrl {

struct K16Args : TrainJobArgs {
    float* wx; float* tmp; uint32_t* I; float* tq; float* dots; uint32_t* tlist; float* vec;
    uint32_t n_jobs; uint32_t* next;
    unsigned long long* counters; uint32_t* bad_job;
};

enum { cNewton, cCg, cHv, cHalvings, cBefore, cGradient, cLine, cActred, cCap, cgDhd, cgQ, cgPositive, cgCap, cLaneRows, cWaveRows, cNonfinite, kCtr };
static_assert(kCtr == (int)kNewtonDeviceCounters, "the counters");

__device__ __forceinline__ bool k16_finite_d(double v) { return (__double_as_longlong(v) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll; }

// a launch's arguments over the slots of sc: jobs base.job0 .. + n_jobs - 1, next: a zeroed counter
K16Args newton_args(const TrainJobArgs& base, const NewtonScratch& sc, uint32_t n_jobs, uint32_t* next);

}  // namespace xrl
