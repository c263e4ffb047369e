// K13 (xrl_train.hip): one layer of XR-Linear's ranker trained in HBM -- the reference's dual coordinate descent for the L1- and L2-loss
// SVC (linear_solver.hpp:420-528), its job set-up and emission (:667-779) over its job list (:797-860).  The rule is stated in
// include/xrl_abi.h at xrl_train_layer_device.
#pragma once
#include <string>

#include "xrl_kernels.h"

namespace xrl {

// the reference's solver table (linear_solver.hpp:36-45); only the two dual SVC solvers are served
constexpr int kSolverL2LossDual = 1, kSolverL1LossDual = 3;

// rows of this many entries and more have their x'x summed by the wavefront (64 squares a step, the adds one chain), shorter ones one per lane
constexpr uint32_t kTrainWaveRow = 64;
// the most wavefronts that train at once, each with a slot of scratch: 16 per CU of an MI355X (4 per SIMD, which k13_solve's registers admit)
constexpr uint32_t kTrainMaxSlots = 4096;
// scratch budget (slots; emission staging) and first length of the table of mt19937(0) outputs, unless the environment says otherwise
// (XRL_TRAIN_SCRATCH_BYTES, XRL_TRAIN_RANDOM_WORDS: tests)
constexpr uint64_t kTrainScratchBytes = 4ull << 30;
constexpr uint64_t kTrainRandomWords = 1ull << 22;
// a table is extended (x4) at most this often before the call gives up
constexpr uint32_t kTrainMaxExtensions = 24;

struct TrainParams {
    double threshold = 0.0;
    uint32_t max_nonzeros = 0;
    int solver_type = kSolverL1LossDual;
    double Cp = 1.0, Cn = 1.0;
    uint64_t max_iter = 1000;
    double eps = 0.1, bias = 1.0;
};

// what ran (xrl_debug_train_counters reports them in this order)
struct TrainCounters {
    uint64_t jobs = 0, batches = 0, slots = 0, stride = 0;
    uint64_t iters = 0, shrinks = 0, reactivations = 0, max_iter_stops = 0, clipped = 0;
    uint64_t lane_rows = 0, wave_rows = 0;
    uint64_t extensions = 0, reruns = 0;
};
constexpr uint32_t kTrainCounterCount = 13;

// X: N x d CSR, column ids strictly ascending per row.  Yt: labels x N, Ct: codes x labels (or null), Mt: codes x N (null with Ct),
// r_val: null or values over Yt's pattern.  out <- W^T, labels x (d + (bias > 0)), a label's entries by ascending feature.  Enqueues on
// s and synchronises it per batch.  Fails (after the check kernels) on unsorted or out-of-range ids and on a label listed twice in Ct.
void train_layer_device(const char* what, const QueriesDev& X, const QueriesDev& Yt, const float* r_val, const QueriesDev* Ct, const QueriesDev* Mt,
                        const TrainParams& p, hipStream_t s, DevCsr& out, TrainCounters& counters);

// fails unless B's row pointer and column ids are A's (the relevance matrix against Y^T; shapes and nnz already agree).  Synchronises s.
void same_pattern_device(const char* what, const QueriesDev& A, const QueriesDev& B, hipStream_t s);

// refusals that read no data (solver, sizes); `what` starts the message
void check_train_params(const std::string& what, const TrainParams& p);

}  // namespace xrl
