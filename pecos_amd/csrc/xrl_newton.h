// K16 (xrl_newton.hip): one layer of XR-Linear's ranker trained in HBM with the reference's primal solver for the L2-loss SVC -- the
// preconditioned-CG Newton method of solve_l2r_l2_svc_primal (linear_solver.hpp:62-323, 407-417; utils/newton.hpp:98-273) between the job
// set-up and the emission that K13 shares (xrl_train_job.h).  The rule is stated in include/xrl_abi.h at xrl_train_layer_newton_device.
#pragma once
#include <string>

#include "xrl_train.h"

namespace xrl {

constexpr int kSolverL2LossPrimal = 2;
// the reference's bounds: NEWTON's own default (param.max_iter is not used), the line search's halvings
constexpr uint32_t kNewtonMaxIter = 1000, kNewtonMaxHalvings = 20;

// what ran (xrl_debug_newton_counters reports them in this order)
struct NewtonCounters {
    uint64_t jobs = 0, batches = 0, slots = 0, stride = 0;
    uint64_t newton_iters = 0, cg_iters = 0, hv_calls = 0, halvings = 0;
    uint64_t end_before_first = 0, end_gradient = 0, end_linesearch = 0, end_actred = 0, end_cap = 0;
    uint64_t cg_dhd = 0, cg_q = 0, cg_positive = 0, cg_cap = 0;
    uint64_t lane_rows = 0, wave_rows = 0, nonfinite_jobs = 0;
};
constexpr uint32_t kNewtonCounterCount = 20;
constexpr uint32_t kNewtonDeviceCounters = 16;                 // the last 16, summed by the wavefronts

// train_layer_device's operands and result, for solver_type == 2.  Fails besides on a non-finite value stored in X and on a job whose CG
// meets a non-finite step length (the first such label is named).
void train_layer_newton_device(const char* what, const QueriesDev& X, const QueriesDev& Yt, const float* r_val, const QueriesDev* Ct, const QueriesDev* Mt,
                               const TrainParams& p, hipStream_t s, DevCsr& out, NewtonCounters& counters);

// refusals that read no data: every solver but 2, each with its reason; `what` starts the message
void check_newton_params(const std::string& what, const TrainParams& p);

// ---- what the layer's driver (xrl_train.hip) uses
struct TrainJobArgs;

// the part of a slot that only K16 has, beside index / cost / y / w / the bitmap: wx and tmp by row, I and the values grad compacts and
// the rows' dot products by listed position, the ascending list of touched features, and g, M, s, r, d, Hd, z BY FEATURE
struct NewtonScratch {
    DevBuf wx, tmp, I, tq, dots, tlist, vec, ctr, bad;
    uint32_t N = 0, d = 0, index_cap = 0;
};
uint64_t newton_slot_bytes(uint32_t N, uint32_t d, uint32_t index_cap);
void newton_reserve(NewtonScratch& sc, uint32_t slots, uint32_t N, uint32_t d, uint32_t index_cap, hipStream_t s);
// jobs base.job0 .. + n_jobs - 1 on `blocks` wavefronts; next: a zeroed counter
void newton_launch(const TrainJobArgs& base, const NewtonScratch& sc, uint32_t n_jobs, uint32_t* next, uint32_t blocks, hipStream_t s);
// the lowest job that met a non-finite step length, or 0xFFFFFFFF
uint32_t newton_bad_job(const NewtonScratch& sc, hipStream_t s);
void newton_read_counters(const NewtonScratch& sc, NewtonCounters& c, hipStream_t s);
void newton_check_finite(const std::string& what, const QueriesDev& X, hipStream_t s);

}  // namespace xrl
