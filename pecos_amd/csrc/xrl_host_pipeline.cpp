// The host ABI (c_xlinear_predict_{csr,drm}_f32) hands over PAGEABLE host arrays.  Large inputs are cut into nnz-balanced
// row batches and pipelined: batch b+1 is copied into pinned staging memory by host threads and travels over PCIe on a copy
// stream while batch b's kernels run; every batch's results start their way back as soon as its last kernel is queued.
// The allocator callback is invoked once, synchronously, on the calling thread, after everything has finished
// (pecos/core/base.py:431-464 discipline).  Small inputs take the single-batch path.
#include "xrl_host_pipeline.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>

namespace xrl {
namespace {

// Host-side worker threads for the bulk copies of the host ABI (staging X into pinned memory, writing the result CSR):
// one thread moves ~6-10 GB/s, which would make a 300 MB X the slowest stage of the pipeline below.
// The workers are persistent (creating 16 threads per 32 MB chunk cost as much as the copy itself): a process-wide pool, never
// destroyed (its threads sleep on a condition variable until the process exits).  One job at a time owns the pool; a caller that
// finds it busy (the per-device host threads of a multi-device handle) spawns its own threads as before.
class CopyPool {
public:
    static CopyPool& get() { static CopyPool* p = new CopyPool(); return *p; }
    // runs fn(n*i/parts, n*(i+1)/parts) for i in [0, parts) on the workers and the caller; false: the pool is busy, nothing was run
    bool try_run(size_t n, unsigned parts, const std::function<void(size_t, size_t)>& fn) {
        std::unique_lock<std::mutex> owner(owner_, std::try_to_lock);
        if (!owner.owns_lock()) return false;
        {
            std::lock_guard<std::mutex> g(mu_);
            fn_ = &fn; n_ = n; parts_ = parts; next_ = 0; pending_ = parts; err_ = nullptr; ++gen_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [&] { return pending_ == 0; });
        fn_ = nullptr;
        if (err_) std::rethrow_exception(err_);
        return true;
    }
private:
    CopyPool() {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const unsigned nw = std::min(15u, hw > 1 ? hw - 1 : 0u);
        for (unsigned i = 0; i < nw; ++i) workers_.emplace_back([this] { loop(); });
        for (auto& t : workers_) t.detach();
    }
    void work() {
        for (;;) {
            unsigned i; const std::function<void(size_t, size_t)>* f; size_t n; unsigned parts;
            {
                std::lock_guard<std::mutex> g(mu_);
                if (!fn_ || next_ >= parts_) return;
                i = next_++; f = fn_; n = n_; parts = parts_;
            }
            std::exception_ptr e;
            try { (*f)(n * i / parts, n * (i + 1) / parts); } catch (...) { e = std::current_exception(); }
            std::lock_guard<std::mutex> g(mu_);
            if (e && !err_) err_ = e;
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return gen_ != seen; }); seen = gen_; }
            work();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex owner_, mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t, size_t)>* fn_ = nullptr;
    size_t n_ = 0; unsigned parts_ = 0, next_ = 0, pending_ = 0; uint64_t gen_ = 0;
    std::exception_ptr err_;
};

template <class F> void parallel_ranges(size_t n, size_t min_per_thread, F&& fn) {
    unsigned nt = (unsigned)std::min<size_t>(16, std::max<size_t>(1, n / std::max<size_t>(1, min_per_thread)));
    nt = std::min(nt, std::max(1u, std::thread::hardware_concurrency()));
    if (nt <= 1) { fn((size_t)0, n); return; }
    {
        const std::function<void(size_t, size_t)> f = [&](size_t b, size_t e) { fn(b, e); };
        if (CopyPool::get().try_run(n, nt, f)) return;
    }
    std::vector<std::thread> th;
    std::exception_ptr err; std::mutex emu;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            try { fn(n * t / nt, n * (t + 1) / nt); }
            catch (...) { std::lock_guard<std::mutex> g(emu); err = std::current_exception(); }
        });
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}
void parallel_copy(void* dst, const void* src, size_t bytes) {
    parallel_ranges(bytes, 1u << 20, [&](size_t b, size_t e) { std::memcpy((char*)dst + b, (const char*)src + b, e - b); });
}
// two equally long arrays at once (labels + scores, column ids + values): one set of threads, each takes its share of both
void parallel_copy2(void* dst0, const void* src0, void* dst1, const void* src1, size_t bytes_each) {
    parallel_ranges(bytes_each, 512u << 10, [&](size_t b, size_t e) {
        std::memcpy((char*)dst0 + b, (const char*)src0 + b, e - b);
        std::memcpy((char*)dst1 + b, (const char*)src1 + b, e - b);
    });
}

// XRL_HOST_TIMING=1: one stderr line per host-ABI call with the wall time of every stage of the pipeline (diagnostics only)
struct HostTimes { double prep = 0, stage = 0, slot_wait = 0, enqueue = 0, final_sync = 0, prefix = 0, alloc = 0, copy_out = 0; };
thread_local HostTimes g_ht;
bool host_timing() { static const bool on = [] { const char* e = std::getenv("XRL_HOST_TIMING"); return e && e[0] == '1'; }(); return on; }
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// (diagnostics, XRL_HOST_TIMING=1: which step of the preparation took long)
struct PrepLap {
    double t = now_ms();
    void operator()(const char* what) {
        if (host_timing() && now_ms() - t > 1.0) std::fprintf(stderr, "[xrl host]   prep: %s took %.2f ms\n", what, now_ms() - t);
        t = now_ms();
    }
};

// csr_t::create_pycsr (pecos/core/utils/matrix.hpp:300-316) over fixed-stride result rows that lie in several buffers, one per contiguous
// row range (the row shards of several devices, or one device's buffer cut into ranges): ONE synchronous allocator call on the calling
// thread, then every range's rows are copied to their place
struct ShardOut { uint32_t r0, r1; const uint32_t* idx; const float* val; const uint32_t* cnt; };
void emit_csr_shards(uint32_t rows, uint32_t cols, uint32_t stride, const std::vector<ShardOut>& sh, py_sparse_allocator_t alloc) {
    // nnz from partial sums (one per shard: the allocator needs nnz first), then the row pointers are written straight into the allocator's
    // array, every shard continuing from its partial sum, and all shards' rows are copied by one parallel pass over the global rows
    double t0 = now_ms();
    const size_t S = sh.size();
    std::vector<uint64_t> part(S + 1, 0);
    parallel_ranges(S, 1, [&](size_t sb, size_t se) {
        for (size_t i = sb; i < se; ++i) { uint64_t a = 0; const ShardOut& s = sh[i]; for (uint32_t r = s.r0; r < s.r1; ++r) a += std::min(s.cnt[r - s.r0], stride); part[i + 1] = a; }
    });
    for (size_t i = 0; i < S; ++i) part[i + 1] += part[i];
    const uint64_t nnz = part[S];
    uint32_t* o_idx = nullptr; uint64_t* o_ptr = nullptr; float* o_val = nullptr;
    g_ht.prefix += now_ms() - t0; t0 = now_ms();
    alloc(false, rows, cols, nnz, &o_idx, &o_ptr, &o_val);
    g_ht.alloc += now_ms() - t0; t0 = now_ms();
    if (!o_ptr || (nnz && (!o_idx || !o_val))) fail("allocator callback returned null buffers");
    o_ptr[0] = 0;
    parallel_ranges(S, 1, [&](size_t sb, size_t se) {
        for (size_t i = sb; i < se; ++i) { uint64_t run = part[i]; const ShardOut& s = sh[i]; for (uint32_t r = s.r0; r < s.r1; ++r) { run += std::min(s.cnt[r - s.r0], stride); o_ptr[r + 1] = run; } }
    });
    // every row full and the shards ranges of ONE buffer (a single device's result): the fixed-stride buffers ARE the CSR arrays
    bool one_buffer = S > 0 && sh[0].r0 == 0 && nnz == (uint64_t)rows * stride;
    for (size_t i = 1; i < S && one_buffer; ++i) one_buffer = sh[i].idx == sh[0].idx + (size_t)sh[i].r0 * stride && sh[i].val == sh[0].val + (size_t)sh[i].r0 * stride;
    if (one_buffer) {
        parallel_copy2(o_idx, sh[0].idx, o_val, sh[0].val, nnz * 4);
        g_ht.copy_out += now_ms() - t0;
        return;
    }
    // shard of a global row: the shards are contiguous and ordered
    std::vector<uint32_t> first(S);
    for (size_t i = 0; i < S; ++i) first[i] = sh[i].r0;
    parallel_ranges(rows, 1u << 15, [&](size_t b, size_t e) {
        size_t i = (size_t)(std::upper_bound(first.begin(), first.end(), (uint32_t)b) - first.begin()) - 1;
        for (size_t g = b; g < e; ++g) {
            while (i + 1 < S && g >= sh[i + 1].r0) ++i;
            const ShardOut& s = sh[i];
            const size_t r = g - s.r0, n = (size_t)(o_ptr[g + 1] - o_ptr[g]);
            std::memcpy(o_idx + o_ptr[g], s.idx + r * stride, n * 4);
            std::memcpy(o_val + o_ptr[g], s.val + r * stride, n * 4);
        }
    });
    g_ht.copy_out += now_ms() - t0;
}

// one device: its result buffer cut into P row ranges, so that the row lengths are summed and the row pointers written by P threads
void emit_csr(uint32_t rows, uint32_t cols, uint32_t stride, const uint32_t* idx, const float* val, const uint32_t* cnt, py_sparse_allocator_t alloc) {
    constexpr size_t P = 16;
    std::vector<ShardOut> sh(P);
    for (size_t p = 0; p < P; ++p) {
        const uint32_t r0 = (uint32_t)((size_t)rows * p / P), r1 = (uint32_t)((size_t)rows * (p + 1) / P);
        sh[p] = ShardOut{r0, r1, idx + (size_t)r0 * stride, val + (size_t)r0 * stride, cnt + r0};
    }
    emit_csr_shards(rows, cols, stride, sh, alloc);
}

// `batch` >= 0: the copies run on the handle's D2H stream behind an event recorded on the compute stream, so that they do not
// hold up the next batch's kernels (callers finish by synchronising both streams); -1: on the compute stream itself.
void download_rows(Model& m, uint32_t r0, uint32_t r1, uint32_t k, int batch = -1) {
    Workspace& ws = *m.ws;
    if (r1 <= r0) return;
    hipStream_t s = m.stream;
    if (batch >= 0) {
        if (!m.d2h_stream) XRL_HIP(hipStreamCreateWithFlags(&m.d2h_stream, hipStreamNonBlocking));
        while (m.d2h_events.size() <= (size_t)batch) { hipEvent_t e; XRL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); m.d2h_events.push_back(e); }
        XRL_HIP(hipEventRecord(m.d2h_events[batch], m.stream));
        XRL_HIP(hipStreamWaitEvent(m.d2h_stream, m.d2h_events[batch], 0));
        s = m.d2h_stream;
    }
    const size_t o = (size_t)r0 * k, n = (size_t)(r1 - r0) * k;
    XRL_HIP(hipMemcpyAsync(ws.h_idx.as<uint32_t>() + o, ws.out_idx.as<uint32_t>() + o, n * 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipMemcpyAsync(ws.h_val.as<float>() + o, ws.out_val.as<float>() + o, n * 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipMemcpyAsync(ws.h_cnt.as<uint32_t>() + r0, ws.out_cnt.as<uint32_t>() + r0, (size_t)(r1 - r0) * 4, hipMemcpyDeviceToHost, s));
}

// The direct path: X is on the device whole; predict every row on the handle's stream, download, wait.  Leaves the fixed-stride results
// in the handle's pinned host buffers and returns their stride.
uint32_t predict_all_rows(Model& m, const QueriesDev& X, const PredictOpts& o) {
    Workspace& ws = *m.ws;
    const uint32_t k = effective_topk(m, o.only_topk);
    reserve_outputs(m, X.rows, k);
    predict_device(m, X, o, ws.out_idx.as<uint32_t>(), ws.out_val.as<float>(), ws.out_cnt.as<uint32_t>(), k, m.stream, false);
    download_rows(m, 0, X.rows, k);
    XRL_HIP(hipStreamSynchronize(m.stream));
    return k;
}

constexpr int kStageSlots = 3;   // == the length of Workspace::stage
constexpr uint64_t kChunkBytes = 32ull << 20;   // the upload moves in chunks of at most this size, whatever the batch size

// The row batches of one call ALTERNATE between two compute streams (the handle's own and its auxiliary one), each with its own
// set of per-batch scratch buffers (Workspace::lane[0] / lane[1], swapped into place around the predict_device call) and its own
// "scratch in use until" event.  A row batch of 30-60 k queries ends in a tail of latency-bound wavefronts (the query-stationary kernel runs
// ~8 rounds of 67 us at that size); on one stream the next batch's first kernel waits for that tail, on two it fills the CUs the tail
// leaves idle.  Batches write disjoint rows of the result buffers; the uploads they wait for are ordered by the copy stream's events.
// XRL_HOST_STREAMS=1 restores the single compute stream.
// The lanes' events live in the handle (Model::host_lanes): they are destroyed with it, on its device.
int host_streams() {
    static const int n = [] { const char* e = std::getenv("XRL_HOST_STREAMS"); return (e && e[0] == '1') ? 1 : 2; }();
    return n;
}

// Lane L's scratch and its "in use until" event are in place while this lives; on every exit, an exception included, what the predict left
// in the handle goes back to the lane's record and lane 0 -- the handle's own bookkeeping -- is in place again.
struct LaneScope {
    Model& m; const int L;
    LaneScope(Model& m_, int L_) : m(m_), L(L_) {
        if (L) std::swap(m.ws->lane[0], m.ws->lane[1]);
        m.ws_done = m.host_lanes.done[L]; m.ws_stream = m.host_lanes.strm[L];
    }
    ~LaneScope() {
        Model::HostLanes& hl = m.host_lanes;
        hl.done[L] = m.ws_done; hl.strm[L] = m.ws_stream;
        if (L) std::swap(m.ws->lane[0], m.ws->lane[1]);
        m.ws_done = hl.done[0]; m.ws_stream = hl.strm[0];
    }
};

// The upload ring of one staged call: elements of X travel to their place in ws.x_idx / x_val on the copy stream in chunks of <= 32 MB,
// through kStageSlots pinned staging buffers or (option host_register) straight from the caller's page-locked arrays.  up[slot] is recorded
// behind every chunk.  Owns the events and the registration: both end with the scope (after the streams have been drained, on an error).
struct UploadRing {
    Model& m; const HostX& x;
    hipEvent_t up[kStageSlots] = {};
    const uint64_t chunk_elems;          // elements per chunk
    uint64_t chunk = 0;                  // chunks so far: slot = chunk % kStageSlots
    bool reg_idx = false, reg_val = false;

    UploadRing(Model& m_, const HostX& x_, uint64_t max_batch_elems, PrepLap& fine) : m(m_), x(x_), chunk_elems(kChunkBytes / x_.elem_bytes()) {
        for (int s = 0; s < kStageSlots; ++s) m.ws->stage[s].reserve(std::min(max_batch_elems, chunk_elems) * x.elem_bytes());
        fine("pinned staging ring");
        if (!m.copy_stream) XRL_HIP(hipStreamCreateWithFlags(&m.copy_stream, hipStreamNonBlocking));
        for (auto& e : up) XRL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (x.csr) {   // the compute streams start after the row pointer has arrived (matters only when X holds no element: no chunk event would order them)
            XRL_HIP(hipEventRecord(up[0], m.copy_stream));
            XRL_HIP(hipStreamWaitEvent(m.stream, up[0], 0));
            if (m.aux_stream) XRL_HIP(hipStreamWaitEvent(m.aux_stream, up[0], 0));
        }
        fine("copy stream + events");
    }
    ~UploadRing() {
        for (auto& e : up) (void)hipEventDestroy(e);
        if (reg_idx) (void)hipHostUnregister(const_cast<uint32_t*>(x.col_idx));
        if (reg_val) (void)hipHostUnregister(const_cast<float*>(x.val));
    }

    // option host_register: page-lock the caller's arrays in place for the duration of the call and let the copy engine read them
    // directly (no staging memcpy); falls back to staging when the registration fails
    void register_caller_arrays() {
        const uint64_t elems = x.elems();
        if (x.csr) {
            reg_idx = hipHostRegister(const_cast<uint32_t*>(x.col_idx), elems * 4, hipHostRegisterDefault) == hipSuccess;
            reg_val = reg_idx && hipHostRegister(const_cast<float*>(x.val), elems * 4, hipHostRegisterDefault) == hipSuccess;
            if (reg_idx && !reg_val) { (void)hipHostUnregister(const_cast<uint32_t*>(x.col_idx)); reg_idx = false; }
        } else {
            reg_val = hipHostRegister(const_cast<float*>(x.val), elems * 4, hipHostRegisterDefault) == hipSuccess;
        }
        (void)hipGetLastError();
    }
    bool direct() const { return reg_val; }

    // elements [c0, c0 + n) from `idx` / `val` (the caller's arrays, or a staging buffer's two halves) to the device
    void h2d(uint64_t c0, uint64_t n, const void* idx, const void* val) {
        Workspace& ws = *m.ws;
        if (x.csr) XRL_HIP(hipMemcpyAsync(ws.x_idx.as<uint32_t>() + c0, idx, n * 4, hipMemcpyHostToDevice, m.copy_stream));
        XRL_HIP(hipMemcpyAsync(ws.x_val.as<float>() + c0, val, n * 4, hipMemcpyHostToDevice, m.copy_stream));
    }
    // sends elements [c0, c0 + n), n <= chunk_elems, through the next slot and returns the slot
    int send_chunk(uint64_t c0, uint64_t n) {
        const int slot = (int)(chunk++ % (uint64_t)kStageSlots);
        if (direct()) {
            h2d(c0, n, x.csr ? x.col_idx + c0 : nullptr, x.val + c0);
            XRL_HIP(hipEventRecord(up[slot], m.copy_stream));
            return slot;
        }
        double t = now_ms();
        if (chunk > (uint64_t)kStageSlots) XRL_HIP(hipEventSynchronize(up[slot]));    // the slot's previous upload has left the staging buffer
        g_ht.slot_wait += now_ms() - t; t = now_ms();
        char* st = m.ws->stage[slot].as<char>();
        if (x.csr) parallel_copy2(st, x.col_idx + c0, st + n * 4, x.val + c0, n * 4);
        else parallel_copy(st, x.val + c0, n * 4);
        h2d(c0, n, st, x.csr ? st + n * 4 : st);
        XRL_HIP(hipEventRecord(up[slot], m.copy_stream));
        g_ht.stage += now_ms() - t;
        return slot;
    }
    // elements [e0, e1) of one row batch; the slot of its last chunk, whose event says "the batch has arrived" (the copy stream is in
    // order), or -1 when the batch holds no element
    int send(uint64_t e0, uint64_t e1) {
        int last_slot = -1;
        for (uint64_t c0 = e0; c0 < e1; c0 += chunk_elems) last_slot = send_chunk(c0, std::min(chunk_elems, e1 - c0));
        return last_slot;
    }
};

// one staged call on one device
struct HostCall {
    Model& m; const HostX& x;
    PredictOpts o;
    QueriesDev X{};                      // X's place on the device (filled by the ring while the batches run)
    std::vector<uint32_t> rb;            // row batch b = rows [rb[b], rb[b + 1])
    uint32_t k = 0;                      // stride of the result rows
    bool two = false;                    // the batches alternate between two compute lanes
    uint32_t n_batch() const { return (uint32_t)rb.size() - 1; }
};

// X's device arrays, sized for the whole call; the CSR row pointer starts its way at once
QueriesDev device_arrays(Model& m, const HostX& x, PrepLap& fine) {
    Workspace& ws = *m.ws;
    const uint64_t elems = x.elems();
    if (x.csr) {
        // the row pointer travels like the rest of X: through pinned staging, first on the copy stream (every row batch waits for a later event of that
        // stream).  A synchronous hipMemcpy from the caller's pageable array took 14-26 ms in the SECOND call of a process (the runtime pins the region it
        // sees again), 0.1 ms otherwise.
        const size_t pb = ((size_t)x.rows + 1) * 8;
        ws.x_ptr.reserve(pb); ws.stage_ptr.reserve(pb);
        if (!m.copy_stream) XRL_HIP(hipStreamCreateWithFlags(&m.copy_stream, hipStreamNonBlocking));
        parallel_copy(ws.stage_ptr.p, x.row_ptr, pb);
        XRL_HIP(hipMemcpyAsync(ws.x_ptr.p, ws.stage_ptr.p, pb, hipMemcpyHostToDevice, m.copy_stream));
        fine("row-pointer upload (pinned staging, copy stream)");
        ws.x_idx.reserve(elems * 4);
    }
    ws.x_val.reserve(elems * 4);
    return device_view(x, ws.x_ptr, ws.x_idx, ws.x_val);
}

// two lanes: the auxiliary one starts after everything queued on the handle's stream so far (an earlier asynchronous predict may still use the scratch)
void open_lanes(Model& m) {
    Model::HostLanes& hl = m.host_lanes;
    if (!m.aux_stream) XRL_HIP(hipStreamCreateWithFlags(&m.aux_stream, hipStreamNonBlocking));
    if (!hl.join) XRL_HIP(hipEventCreateWithFlags(&hl.join, hipEventDisableTiming));
    hl.done[0] = m.ws_done; hl.strm[0] = m.ws_stream;              // lane 0 = the handle's own bookkeeping; lane 1 keeps its event between calls
    XRL_HIP(hipEventRecord(hl.join, m.stream));
    XRL_HIP(hipStreamWaitEvent(m.aux_stream, hl.join, 0));
}

void launch_batch(HostCall& c, uint32_t b, int L, hipStream_t S) {
    Workspace& ws = *c.m.ws;
    std::optional<LaneScope> lane;
    if (c.two) lane.emplace(c.m, L);
    const double t_pd = now_ms();
    predict_device(c.m, c.X, c.o, ws.out_idx.as<uint32_t>(), ws.out_val.as<float>(), ws.out_cnt.as<uint32_t>(), c.k, S, false,
                   c.rb[b], c.rb[b + 1] - c.rb[b]);
    if (host_timing() && now_ms() - t_pd > 0.5)      // (diagnostics: a launch sequence that blocked -- an allocation, a code-object load)
        std::fprintf(stderr, "[xrl host]   batch %u/%u (%u rows, lane %d): enqueue took %.2f ms\n", b, c.n_batch(), c.rb[b + 1] - c.rb[b], L, now_ms() - t_pd);
}

// Results, called after batch b (which ran on lane L) has been queued: everything but the last batch goes back in ONE set of copies on
// the D2H stream, queued before the last batch's kernels (per-batch copies are blit kernels that held up the next batch's launch:
// 12 x 0.15 ms); the last batch follows behind an event of its own.
void queue_downloads(HostCall& c, uint32_t b, int L) {
    Model& m = c.m;
    Model::HostLanes& hl = m.host_lanes;
    const uint32_t n_batch = c.n_batch();
    if (b + 2 == n_batch) {
        if (c.two) {                                               // the copies wait for BOTH lanes' batches (download_rows adds the handle's stream)
            if (!m.d2h_stream) XRL_HIP(hipStreamCreateWithFlags(&m.d2h_stream, hipStreamNonBlocking));
            XRL_HIP(hipEventRecord(hl.join, m.aux_stream));
            XRL_HIP(hipStreamWaitEvent(m.d2h_stream, hl.join, 0));
        }
        const double t_dl = now_ms();
        download_rows(m, 0, c.rb[b + 1], c.k, 0);
        if (host_timing() && now_ms() - t_dl > 0.5) std::fprintf(stderr, "[xrl host]   download of rows [0, %u): enqueue took %.2f ms\n", c.rb[b + 1], now_ms() - t_dl);
    } else if (b + 1 == n_batch) {
        if (c.two && L) {                                          // the last batch ran on the auxiliary stream: its copies follow on the handle's stream
            XRL_HIP(hipEventRecord(hl.join, m.aux_stream));
            XRL_HIP(hipStreamWaitEvent(m.stream, hl.join, 0));
        }
        const double t_dl = now_ms();
        // (on the D2H stream behind an event, like the rest: queued on the compute stream itself the copies blocked the enqueuing thread for 5-9 ms in a
        //  process's first two calls)
        download_rows(m, n_batch > 1 ? c.rb[b] : 0, c.rb[b + 1], c.k, 1);
        if (host_timing() && now_ms() - t_dl > 0.5) std::fprintf(stderr, "[xrl host]   download of the last batch: enqueue took %.2f ms\n", now_ms() - t_dl);
    }
}

// per batch: upload, wait, launch, download policy; then the final sync
void run_batches(HostCall& c, UploadRing& ring) {
    Model& m = c.m;
    if (c.two) open_lanes(m);
    for (uint32_t b = 0; b < c.n_batch(); ++b) {
        const int last_slot = ring.send(c.x.elem_at(c.rb[b]), c.x.elem_at(c.rb[b + 1]));
        const double t_ph = now_ms();
        const int L = c.two ? (int)(b & 1u) : 0;
        hipStream_t S = L ? m.aux_stream : m.stream;
        if (last_slot >= 0) XRL_HIP(hipStreamWaitEvent(S, ring.up[last_slot], 0));   // batch b's kernels start when its rows have arrived
        if (c.rb[b + 1] > c.rb[b]) launch_batch(c, b, L, S);
        queue_downloads(c, b, L);
        g_ht.enqueue += now_ms() - t_ph;
    }
    const double t_ph = now_ms();
    if (c.two) XRL_HIP(hipStreamSynchronize(m.aux_stream));
    XRL_HIP(hipStreamSynchronize(m.stream));
    if (m.d2h_stream) XRL_HIP(hipStreamSynchronize(m.d2h_stream));
    g_ht.final_sync += now_ms() - t_ph;
}

// after an error: nothing of the call may still be in flight when its events are destroyed and the caller's arrays unregistered
void drain_streams(Model& m, bool two) {
    (void)hipStreamSynchronize(m.copy_stream); (void)hipStreamSynchronize(m.stream);
    if (two) (void)hipStreamSynchronize(m.aux_stream);
    if (m.d2h_stream) (void)hipStreamSynchronize(m.d2h_stream);
}

// Runs the whole host-ABI pipeline of ONE device for the rows of `x` and leaves the fixed-stride results in the handle's
// pinned host buffers (ws.h_idx / h_val / h_cnt, stride k); the caller holds m.mu and emits the CSR afterwards.
void host_compute(Model& m, const HostX& x, PredictOpts o) {
    use_device(m.device);
    if (!m.ws) m.ws = std::make_unique<Workspace>();
    const double t_prep = now_ms();
    const bool staged = staged_upload(x, m.opt.host_pipeline);
    HostCall c{m, x, o};
    c.rb = plan_row_batches(x, m.opt.host_batch_mb, staged);
    if (!staged) {
        upload_x(x, m.ws->x_ptr, m.ws->x_idx, m.ws->x_val, c.X);
        predict_all_rows(m, c.X, o);
        return;
    }
    uint64_t max_elems = 0;
    for (uint32_t b = 0; b < c.n_batch(); ++b) {
        max_elems = std::max(max_elems, x.elem_at(c.rb[b + 1]) - x.elem_at(c.rb[b]));
        c.o.reserve_rows = std::max(c.o.reserve_rows, c.rb[b + 1] - c.rb[b]);
    }
    PrepLap fine;
    fine("batch planning");
    c.X = device_arrays(m, x, fine);
    fine("device arrays of X");
    UploadRing ring(m, x, max_elems, fine);
    c.k = effective_topk(m, o.only_topk);
    reserve_outputs(m, x.rows, c.k);
    fine("result buffers (device + pinned host)");
    if (m.opt.host_register) ring.register_caller_arrays();
    // two compute lanes for the row batches (see host_streams above); the handle's lock is held by the caller
    // (overlap_min_rows > 0 makes predict_device itself run two lanes over ws.lane[0 / 1] and the auxiliary stream: the two schemes would share
    //  scratch and stream without an ordering between them, so the host lanes stand down)
    c.two = host_streams() == 2 && c.n_batch() >= 3 && !m.profiling && m.opt.overlap_min_rows == 0;
    g_ht.prep += now_ms() - t_prep;
    try { run_batches(c, ring); }
    catch (...) { drain_streams(m, c.two); throw; }      // ... and only then does `ring` end
}

// shard boundaries of a multi-device call: equal shares of the nnz (+1 per row so that empty rows still count); dense X: equal rows
std::vector<uint32_t> plan_device_shards(const HostX& x, size_t R) {
    const uint32_t rows = x.rows;
    std::vector<uint32_t> sb(R + 1, rows);
    sb[0] = 0;
    for (size_t d = 1; d < R; ++d) {
        if (x.csr) {
            const uint64_t total = x.row_ptr[rows] + rows, want = total * d / R;
            uint32_t lo = sb[d - 1], hi = rows;                          // first row r with row_ptr[r] + r >= want
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (x.row_ptr[mid] + mid < want) lo = mid + 1; else hi = mid; }
            sb[d] = lo;
        } else sb[d] = (uint32_t)((uint64_t)rows * d / R);
    }
    return sb;
}

// rows [r0, r1) of x as an X of their own; `rebased` keeps the shard's row pointer alive
HostX shard_of(const HostX& x, uint32_t r0, uint32_t r1, std::vector<uint64_t>& rebased) {
    HostX v = x;
    const uint64_t e0 = x.elem_at(r0);
    v.rows = r1 - r0; v.val = x.val + e0;
    if (x.csr) {
        rebased.resize((size_t)(r1 - r0) + 1);
        for (uint32_t r = r0; r <= r1; ++r) rebased[r - r0] = x.row_ptr[r] - e0;
        v.row_ptr = rebased.data(); v.col_idx = x.col_idx + e0;
    }
    return v;
}

// one host thread per device runs the single-device pipeline on its shard (its own stream, pinned staging and PCIe link; no inter-GPU
// traffic); the calling thread takes the handle's own device, whose lock the caller holds
void compute_shards(Model& m, const HostX& x, const PredictOpts& o, const std::vector<uint32_t>& sb) {
    const size_t R = sb.size() - 1;
    std::vector<std::exception_ptr> errs(R);
    std::vector<std::vector<uint64_t>> rebased(R);
    auto work = [&](size_t d) {
        try {
            Model& md = d == 0 ? m : *m.replicas[d - 1];
            std::unique_lock<std::mutex> lk(md.mu, std::defer_lock);
            if (d != 0) lk.lock();
            if (sb[d + 1] <= sb[d]) return;
            host_compute(md, shard_of(x, sb[d], sb[d + 1], rebased[d]), o);
        } catch (...) { errs[d] = std::current_exception(); }
    };
    std::vector<std::thread> th;
    for (size_t d = 1; d < R; ++d) th.emplace_back(work, d);
    work(0);
    for (auto& t : th) t.join();
    use_device(m.device);
    for (auto& e : errs) if (e) std::rethrow_exception(e);
}

}  // namespace

bool staged_upload(const HostX& x, int host_pipeline) { return host_pipeline && x.elems() * x.elem_bytes() >= kChunkBytes; }

// Compute batches: CSR -- ~24 MB of nnz each (the kernels' cost follows nnz); dense -- at least 64 k rows each, because the
// tiled SGEMM K1G needs many queries per parent (a 24 MB batch of 768-float rows would leave ~10 per leaf parent and fall
// back to the query-stationary kernel, 5x slower).
std::vector<uint32_t> plan_row_batches(const HostX& x, int host_batch_mb, bool staged) {
    const uint32_t rows = x.rows;
    const uint64_t elems = x.elems();
    // CSR: batches GROW (x1.6 from a third of host_batch_mb up to 3x host_batch_mb): the first kernels start after a few megabytes have
    // arrived, the later launches are large enough to fill the chip (a 40 k-row launch of the query-stationary kernel runs at 0.7x
    // the per-row rate of a 490 k-row one: measured with rocprofv3's copy + kernel trace, profiles/r03_pruning_topk.md section 4)
    std::vector<uint64_t> share;                                        // cumulative element targets of the batch ends
    if (staged && rows >= 8192) {
        if (x.csr) {
            const double mb = (double)(1u << 20) / 8.0;                    // elements per megabyte of (id, value) pairs
            double cur = std::max(1, host_batch_mb) / 3.0, pos = 0.0;
            const double cap = 3.0 * std::max(1, host_batch_mb);
            while (pos + cur * mb < (double)elems && share.size() < 31) { pos += cur * mb; share.push_back((uint64_t)pos); cur = std::min(cap, cur * 1.6); }
            // a short last batch joins the previous one (the tail after the upload ends is one launch either way)
            // (a TAPERED end -- last two batches of host_batch_mb and half of it, to shorten the tail after the last byte of X has
            //  arrived -- gave 9.57 -> 9.06 ms on Amazon-670K but 18.5 -> 19.2 ms on the hard workload, and the extra batches shift the pruning
            //  feedback's re-probe cadence; not kept: profiles/r05_host_abi.md)
            if (!share.empty() && (double)elems - (double)share.back() < 0.25 * cur * mb) share.pop_back();
        } else {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(1, rows / 65536u));
            for (uint32_t b = 1; b < nb; ++b) share.push_back(elems * b / nb);
        }
    }
    // batch boundaries: the first row at or past every share of the elements (CSR: of the nnz -- cost follows nnz, not rows)
    const uint32_t n_batch = (uint32_t)share.size() + 1;
    std::vector<uint32_t> rb(n_batch + 1, rows);
    rb[0] = 0;
    for (uint32_t b = 1; b < n_batch; ++b) {
        if (x.csr) rb[b] = (uint32_t)(std::lower_bound(x.row_ptr, x.row_ptr + rows + 1, share[b - 1]) - x.row_ptr);
        else rb[b] = (uint32_t)((uint64_t)rows * b / n_batch);
        rb[b] = std::min(std::max(rb[b], rb[b - 1]), rows);
    }
    return rb;
}

void reserve_outputs(Model& m, uint32_t rows, uint32_t k) {
    Workspace& ws = *m.ws;
    const size_t cells = (size_t)rows * k;
    ws.out_idx.reserve(cells * 4); ws.out_val.reserve(cells * 4); ws.out_cnt.reserve((size_t)rows * 4);
    ws.h_idx.reserve(cells * 4); ws.h_val.reserve(cells * 4); ws.h_cnt.reserve((size_t)rows * 4);
}

void run_and_emit(Model& m, const QueriesDev& X, const PredictOpts& o, py_sparse_allocator_t alloc) {
    Workspace& ws = *m.ws;
    const Layer& last = *m.layers.back();
    const uint32_t out_cols = last.reordered ? last.c_rows : last.w_cols;   // inference.hpp:1776-1784
    const uint32_t k = predict_all_rows(m, X, o);
    emit_csr(X.rows, out_cols, k, ws.h_idx.as<uint32_t>(), ws.h_val.as<float>(), ws.h_cnt.as<uint32_t>(), alloc);
}

// c_xlinear_predict_{csr,drm}_f32.  With replicas behind the handle (xrl_set_option "devices"): the rows are cut into nnz-balanced
// shards, every device runs the single-device pipeline above on its shard, and the results of all shards go into the arrays of the one
// allocator call.
void predict_host(void* ptr, const HostX& x, uint32_t beam, const char* pp, uint32_t topk, py_sparse_allocator_t alloc) {
    Model& m = *as_model(ptr);
    if (!alloc) fail("null allocator callback");
    if (!x.given) fail("null X");
    std::lock_guard<std::mutex> g(m.mu);
    PredictOpts o; o.beam_size = beam; o.only_topk = topk; o.post_processor = pp;
    const uint32_t rows = x.rows;
    const Layer& last = *m.layers.back();
    const uint32_t out_cols = last.reordered ? last.c_rows : last.w_cols;
    const uint32_t k = effective_topk(m, o.only_topk);
    const size_t R = 1 + m.replicas.size();
    if (R == 1 || rows < 2 * R) {
        const double t_call = now_ms();
        g_ht = HostTimes{};
        host_compute(m, x, o);
        Workspace& ws = *m.ws;
        emit_csr(rows, out_cols, k, ws.h_idx.as<uint32_t>(), ws.h_val.as<float>(), ws.h_cnt.as<uint32_t>(), alloc);
        if (host_timing())
            std::fprintf(stderr, "[xrl host] rows=%u total=%.2f ms: prep %.2f | stage-memcpy+h2d-enqueue %.2f | wait for a staging slot %.2f | kernel+d2h enqueue %.2f | "
                                 "final sync %.2f | row-pointer prefix %.2f | allocator callback %.2f | copy out %.2f\n",
                         rows, now_ms() - t_call, g_ht.prep, g_ht.stage, g_ht.slot_wait, g_ht.enqueue, g_ht.final_sync, g_ht.prefix, g_ht.alloc, g_ht.copy_out);
        return;
    }
    const std::vector<uint32_t> sb = plan_device_shards(x, R);
    compute_shards(m, x, o, sb);
    std::vector<ShardOut> sh;
    for (size_t d = 0; d < R; ++d) {
        if (sb[d + 1] <= sb[d]) continue;
        Workspace& ws = *(d == 0 ? m : *m.replicas[d - 1]).ws;
        sh.push_back(ShardOut{sb[d], sb[d + 1], ws.h_idx.as<uint32_t>(), ws.h_val.as<float>(), ws.h_cnt.as<uint32_t>()});
    }
    g_ht = HostTimes{};                                       // (the shards' pipelines ran on their own threads: only the shared tail is timed here)
    const double t_emit = now_ms();
    emit_csr_shards(rows, out_cols, k, sh, alloc);
    if (host_timing())
        std::fprintf(stderr, "[xrl host] rows=%u devices=%zu: result hand-off %.2f ms: row-pointer prefix %.2f | allocator callback %.2f | copy out %.2f\n",
                     rows, R, now_ms() - t_emit, g_ht.prefix, g_ht.alloc, g_ht.copy_out);
}

// Everything the host ABI needs that does not depend on the caller's X is created when a model is LOADED from a folder, not inside the first
// predict (a user's first call cost 42-66 ms, 25 of them allocations, 15 more the first launches): the copy-thread pool,
// the copy / auxiliary / D2H streams, the three pinned staging buffers of the upload ring, the code objects of the kernels the default
// policy runs, and BOTH scratch lanes sized for the row batches the pipeline cuts (a 36 MB batch of Amazon-shape rows is ~60 k queries).
// One tiny predict per lane does the last two.  XRL_WARM=0 skips it (tests that load hundreds of throw-away models may want to).
constexpr uint32_t kWarmRows = 65536;
void warm_handle(Model& m) {
    static const bool off = [] { const char* e = std::getenv("XRL_WARM"); return e && e[0] == '0'; }();
    if (off || m.layers.empty()) return;
    use_device(m.device);
    if (!m.ws) m.ws = std::make_unique<Workspace>();
    Workspace& ws = *m.ws;
    (void)CopyPool::get();
    if (!m.copy_stream) XRL_HIP(hipStreamCreateWithFlags(&m.copy_stream, hipStreamNonBlocking));
    if (!m.aux_stream) XRL_HIP(hipStreamCreateWithFlags(&m.aux_stream, hipStreamNonBlocking));
    if (!m.d2h_stream) XRL_HIP(hipStreamCreateWithFlags(&m.d2h_stream, hipStreamNonBlocking));
    for (int s2 = 0; s2 < kStageSlots; ++s2) ws.stage[s2].reserve((size_t)kChunkBytes);
    ws.stage_ptr.reserve((((size_t)1 << 19) + 1) * 8);
    // 256 one-feature queries through the default policy, once per scratch lane
    const uint32_t R = 256, D = std::max<uint32_t>(1, m.nr_features);
    std::vector<uint64_t> ptr(R + 1); std::vector<uint32_t> idx(R); std::vector<float> val(R, 1.0f);
    for (uint32_t r = 0; r <= R; ++r) ptr[r] = r;
    for (uint32_t r = 0; r < R; ++r) idx[r] = (uint32_t)(((uint64_t)r * 2654435761ull) % D);
    ScipyCsrF32 Xh{}; Xh.rows = R; Xh.cols = m.nr_features; Xh.row_ptr = ptr.data(); Xh.col_idx = idx.data(); Xh.val = val.data();
    QueriesDev X{};
    upload_x(HostX(&Xh), ws.x_ptr, ws.x_idx, ws.x_val, X);
    PredictOpts o; o.reserve_rows = kWarmRows;
    const uint32_t k = effective_topk(m, 0);
    // result buffers (device + PINNED host: 4-10 ms to allocate inside a first call) for calls of up to 2^19 rows / 2^23 result cells: 64 MiB pinned per handle at most
    reserve_outputs(m, std::max<uint32_t>(R, (uint32_t)std::min<uint64_t>(1u << 19, (1ull << 23) / std::max<uint32_t>(1u, k))), k);
    // (not a LaneScope: the warm-up runs on the handle's own stream and leaves ws_done / ws_stream alone; only the scratch changes places)
    for (int L = 0; L < 2 && !m.csc_route; ++L) {   // (the CSC route builds its device copy of W on first use: not here)
        if (L) std::swap(ws.lane[0], ws.lane[1]);
        try { predict_device(m, X, o, ws.out_idx.as<uint32_t>(), ws.out_val.as<float>(), ws.out_cnt.as<uint32_t>(), k, m.stream, true); }
        catch (...) { if (L) std::swap(ws.lane[0], ws.lane[1]); throw; }
        if (L) std::swap(ws.lane[0], ws.lane[1]);
    }
    // Every stream's FIRST copy pays for the runtime setting up its copy path (measured: 5.5 ms inside the first call's download on the D2H stream, 5.5 ms
    // again two calls later when the last row batch first lands on the other compute lane): one 1 MiB copy each way on each stream now, at load.
    const size_t nb = std::min<size_t>((size_t)1 << 20, std::min(ws.out_idx.cap, ws.h_idx.cap));
    for (hipStream_t st : {m.stream, m.aux_stream, m.d2h_stream, m.copy_stream}) {
        if (!st || !nb) continue;
        XRL_HIP(hipMemcpyAsync(ws.h_idx.p, ws.out_idx.p, nb, hipMemcpyDeviceToHost, st));
        XRL_HIP(hipMemcpyAsync(ws.out_idx.p, ws.stage[0].p, std::min(nb, ws.stage[0].cap), hipMemcpyHostToDevice, st));
        XRL_HIP(hipStreamSynchronize(st));
    }
    // The warm-up queries (one feature each) say nothing about the caller's data: what the pruning feedback learned from them is discarded -- their
    // later stages hold almost every item, which marked the leaf "unstaged" and made a fresh handle score all beam parents of every query until the first
    // re-probe, 32 row batches (~3 host-ABI calls) later.
    m.fb.reset();
}

}  // namespace xrl
