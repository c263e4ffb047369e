// Host-side model compiler: CSC W + C  ->  tiled rank-bitmap layout in HBM (see xrl_model.h).
//
// Mirrors the load-time work of the reference without sharing its data structures:
//   LayerData<chunked>::init                pecos/core/xmc/inference.hpp:1849-1883
//   check_if_contiguously_ordered           :658-668
//   rearrangement_t::initialize_from_codes  :1746-1761   (perm / perm_inv)
//   make_chunked_from_csc                   :557-650     (transpose-by-parent, rows ascending,
//                                                         columns ascending inside a row)
//   check_bias_explicit                     :500-502
#include "xrl_model.h"
#include "xrl_kernels.h"   // SelectTreeLayer (ensure_device_tree)

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <thread>

namespace xrl {

PostProc parse_post_processor(const char* name_c) {
    // PostProcessor<T>::get, inference.hpp:192-240.  Unknown names yield the default-constructed
    // processor there (identity transform, combiner keeps x) -> PP_NOOP here.
    PostProc pp;
    if (!name_c) return pp;
    const std::string name(name_c);
    auto ends = [&](const char* s) { const size_t n = std::strlen(s); return name.size() >= n && name.compare(name.size() - n, n, s) == 0; };
    if (name == "noop") return pp;
    if (name == "sigmoid") { pp.kind = PP_SIGMOID; return pp; }
    if (name == "log-sigmoid") { pp.kind = PP_LOG_SIGMOID; return pp; }
    if (name.rfind("log-l", 0) == 0 && ends("-hinge")) {
        pp.kind = PP_LOG_LP_HINGE;
        pp.p = std::atoi(name.substr(5, name.size() - 5 - 6).c_str());
        return pp;
    }
    if (name.rfind("l", 0) == 0 && ends("-hinge")) {
        pp.kind = PP_LP_HINGE;
        pp.p = std::atoi(name.substr(1, name.size() - 1 - 6).c_str());
        return pp;
    }
    return pp;
}

uint64_t Layer::cand_bound(uint32_t beam) const {
    uint64_t s = 0;
    for (uint32_t i = 0; i < beam && i < chunk_sizes_desc.size(); ++i) s += chunk_sizes_desc[i];
    return s;
}

uint64_t ConstraintView::cand_bound(uint32_t beam) const {
    uint64_t s = 0;
    for (uint32_t i = 0; i < beam && i < chunk_sizes_desc.size(); ++i) s += chunk_sizes_desc[i];
    return s;
}

Model::Model() {}
Model::~Model() {
    replicas.clear();                       // each replica releases its objects with ITS device current
    (void)hipSetDevice(device);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (host_lanes.done[1] && host_lanes.done[1] != ws_done) (void)hipEventDestroy(host_lanes.done[1]);   // (done[0] aliases ws_done)
    if (host_lanes.join) (void)hipEventDestroy(host_lanes.join);
    if (aux_stream) (void)hipStreamDestroy(aux_stream);
    if (ws_done) (void)hipEventDestroy(ws_done);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (d2h_stream) (void)hipStreamDestroy(d2h_stream);
    for (hipEvent_t e : d2h_events) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}
uint64_t Model::device_bytes() const {
    uint64_t b = 0;
    for (auto& l : layers) b += l->device_bytes;
    return b;
}

namespace {
template <class F> void parallel_for(size_t n, F&& fn) {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 4;
    if (nt > 64) nt = 64;
    if (n < 2 * nt) { for (size_t i = 0; i < n; ++i) fn(i); return; }
    std::atomic<size_t> next{0};
    std::exception_ptr err;
    std::mutex emu;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&] {
            try {
                for (;;) {
                    const size_t i0 = next.fetch_add(16);
                    if (i0 >= n) break;
                    for (size_t i = i0; i < std::min(n, i0 + 16); ++i) fn(i);
                }
            } catch (...) { std::lock_guard<std::mutex> g(emu); err = std::current_exception(); }
        });
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}
struct Nz { uint32_t row, col; float val; };
}  // namespace

// K1 packs {entry offset, count} of a row unit into 32 bits: tile-relative entry offsets stay below 2^25.
// XRL_MAX_TILE_ENTRIES lowers the limit (tests of the tile splitter).
static uint64_t max_tile_entries() {
    static const uint64_t v = [] {
        const char* e = std::getenv("XRL_MAX_TILE_ENTRIES");
        const uint64_t lim = (1ull << 25) - 64;
        if (!e) return lim;
        const uint64_t x = std::strtoull(e, nullptr, 10);
        return x >= 2 && x < lim ? x : lim;
    }();
    return v;
}

// Even split of a chunk of n columns into column tiles: the smallest count (starting from ceil(n / kMaxTileCols), grown
// by a quarter at a time) for which every tile [n*t/k, n*(t+1)/k) holds fewer than `limit` entries; cum[0..n] are the
// prefix sums of the columns' entry counts.  Returns 0 when even one column per tile does not fit.
uint32_t split_chunk(const uint64_t* cum, uint32_t n, uint64_t limit) {
    uint32_t nt = (n + kMaxTileCols - 1) / kMaxTileCols;
    if (n == 0) return nt;
    auto fits = [&](uint32_t k) {
        for (uint32_t t = 0; t < k; ++t)
            if (cum[(uint64_t)n * (t + 1) / k] - cum[(uint64_t)n * t / k] >= limit) return false;
        return true;
    };
    while (!fits(nt)) {
        if (nt >= n) return 0;
        nt = std::min<uint32_t>(n, nt + std::max<uint32_t>(1, nt / 4));
    }
    return nt;
}

// Placement of a tile's rows in its entry block.  rptr[0..nrows] are the rows' packed (CSR) starts; with `align` a row
// that would touch more 128-byte lines (16 entries) than its length requires starts at the next 16-entry boundary.
// Writes the packed extents (pack_row_extent) when ext != nullptr; returns the block's entry count, a multiple of 16.
uint64_t layout_tile_rows(const uint32_t* rptr, uint32_t nrows, bool align, uint32_t* ext) {
    uint64_t cur = 0;
    for (uint32_t r = 0; r < nrows; ++r) {
        const uint32_t len = rptr[r + 1] - rptr[r];
        if (len == 0 || len > kMaxTileCols) fail("layer: internal error, tile row length");
        if (align && ((cur & 15) + len + 15) / 16 > ((uint64_t)len + 15) / 16) cur = (cur + 15) & ~15ull;
        if (ext) ext[r] = pack_row_extent((uint32_t)(cur & 0x1FFFFFFu), len);
        cur += len;
    }
    return (cur + 15) & ~15ull;
}

uint64_t Layer::buffer_bytes() const {
    uint64_t b = 0;
    for (const DevBuf* d : {&d_csc_ptr, &d_csc_idx, &d_csc_val, &d_tiles, &d_ptile, &d_chunk_col, &d_bitmap, &d_row_ptr, &d_row_idx, &d_entries, &d_perm_inv,
                            &d_chunk_alg, &d_bias_prod, &d_bucket, &d_bitmap64, &d_wd, &d_dptile, &d_dtcol, &d_tile_parent, &d_pres, &d_wt, &d_wt_base, &d_sel_parent, &d_sel_crank,
                            &view.d_chunk_col, &view.d_perm_inv})
        b += d->cap;
    return b;
}

// ---- the stages of compile_layer: each owns one format or one decision, takes plain inputs and hands back host vectors
namespace {

bool env_enabled(const char* name) {   // on/off switches (A/B, tests): on unless the variable starts with '0'
    const char* e = std::getenv(name);
    return !(e && e[0] == '0');
}

bool free_hbm(uint64_t& free_b) {      // false when the runtime cannot tell
    size_t f = 0, total = 0;
    if (hipMemGetInfo(&f, &total) != hipSuccess) return false;
    free_b = f;
    return true;
}

// Room ONE optional format of one layer may take: the cap of `max_mb_var` (default 64 GiB), and never more than a quarter of the free HBM
uint64_t format_budget(const char* max_mb_var) {
    uint64_t cap_b = 64ull << 30, free_b = 0;
    if (const char* mb = std::getenv(max_mb_var)) cap_b = std::strtoull(mb, nullptr, 10) << 20;
    if (free_hbm(free_b)) cap_b = std::min<uint64_t>(cap_b, free_b / 4);
    return cap_b;
}

// A column with duplicate or unsorted row ids cannot be scattered into one cell per (feature, column): such a layer stays in the tile format
// without densely held rows.  (A weight whose bits equal the "no entry" marker -- an explicit -0.0 -- is stored as +0.0 by densify_kernel.)
bool columns_strictly_ascending(const HostCsc& W) {
    for (uint32_t c = 0; c < W.cols; ++c)
        for (uint64_t e = W.col_ptr[c] + 1; e < W.col_ptr[c + 1]; ++e)
            if (W.row_idx[e] <= W.row_idx[e - 1]) return false;
    return true;
}

struct TilePlan {
    const HostCsc* C;
    bool contiguous;                          // children already ordered by parent: rearranged column == original column
    std::vector<uint32_t> ptile, chunk_col;   // [P + 1]
    std::vector<TileDesc> tiles;              // col_begin / ncols / ent_base (packed) here; rows by gather_tile_rows, final ent_base by lay_out_entries
    std::vector<uint64_t> tile_nnz;
    uint64_t nnz;
    uint32_t orig_col(uint32_t c) const { return contiguous ? c : C->row_idx[c]; }
};

// Checks C, records the tree in L (child order, parent map, chunk sizes) and cuts every chunk into column tiles.
TilePlan plan_tiles(const HostCsc& W, const HostCsc& C, Layer& L) {
    TilePlan tp;
    tp.C = &C;
    const uint64_t c_nnz = C.nnz();
    if (c_nnz > 0xFFFFFFFFull) fail("layer: too many children");
    for (uint64_t i = 0; i < c_nnz; ++i) if (C.row_idx[i] >= W.cols) fail("layer: C row index out of range");

    // children must be contiguous by parent; otherwise rearrange (inference.hpp:658-668,1855-1872)
    tp.contiguous = (c_nnz == C.rows);
    if (tp.contiguous) for (uint64_t i = 0; i < c_nnz; ++i) if (C.row_idx[i] != i) { tp.contiguous = false; break; }
    L.reordered = !tp.contiguous;
    L.n_children = (uint32_t)c_nnz;
    const uint32_t P = C.cols;
    L.h_c_ptr = C.col_ptr; L.h_c_idx.assign(C.row_idx.begin(), C.row_idx.begin() + c_nnz);
    L.h_parent.assign(C.rows, 0xFFFFFFFFu);
    for (uint32_t p = 0; p < P; ++p) for (uint64_t c = C.col_ptr[p]; c < C.col_ptr[p + 1]; ++c) L.h_parent[C.row_idx[c]] = p;

    auto col_nnz = [&](uint32_t c) { const uint32_t oc = tp.orig_col(c); return W.col_ptr[oc + 1] - W.col_ptr[oc]; };
    tp.ptile.assign(P + 1, 0); tp.chunk_col.assign(P + 1, 0);
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t cb = (uint32_t)C.col_ptr[p], ce = (uint32_t)C.col_ptr[p + 1];
        tp.chunk_col[p] = cb;
        const uint32_t n = ce - cb;
        L.chunk_sizes_desc.push_back(n);
        L.max_chunk_cols = std::max(L.max_chunk_cols, n);
        // column tiles: at most kMaxTileCols children and fewer than max_tile_entries() weights each (K1 packs a
        // tile-relative entry offset into 25 bits); an even split, refined until every tile fits
        uint32_t nt = (n + kMaxTileCols - 1) / kMaxTileCols;
        if (n > 0) {
            std::vector<uint64_t> cum(n + 1, 0);
            for (uint32_t c = 0; c < n; ++c) cum[c + 1] = cum[c] + col_nnz(cb + c);
            nt = split_chunk(cum.data(), n, max_tile_entries());
            if (nt == 0) fail("layer: one weight column holds " + std::to_string(max_tile_entries()) + " or more entries");
        }
        for (uint32_t t = 0; t < nt; ++t) {
            TileDesc td{};
            const uint32_t b = cb + (uint32_t)((uint64_t)n * t / nt), e = cb + (uint32_t)((uint64_t)n * (t + 1) / nt);
            td.col_begin = b; td.ncols = e - b; td.bias_slot = kNoBias;
            L.max_tile_cols = std::max(L.max_tile_cols, td.ncols);
            tp.tiles.push_back(td);
        }
        tp.ptile[p + 1] = (uint32_t)tp.tiles.size();
        L.max_tiles_per_parent = std::max(L.max_tiles_per_parent, nt);
    }
    tp.chunk_col[P] = (uint32_t)c_nnz;
    std::sort(L.chunk_sizes_desc.begin(), L.chunk_sizes_desc.end(), std::greater<uint32_t>());

    // entry bases are known from column nnz alone
    const uint32_t T = (uint32_t)tp.tiles.size();
    tp.tile_nnz.assign(T, 0);
    tp.nnz = 0;
    for (uint32_t t = 0; t < T; ++t) {
        uint64_t n = 0;
        for (uint32_t c = tp.tiles[t].col_begin; c < tp.tiles[t].col_begin + tp.tiles[t].ncols; ++c) n += col_nnz(c);
        if (n >= max_tile_entries()) fail("layer: internal error, tile over the entry limit");
        tp.tile_nnz[t] = n;
        tp.tiles[t].ent_base = tp.nnz;
        tp.nnz += n;
    }
    L.n_tiles = T; L.nnz = tp.nnz;
    return tp;
}

enum LookupKind { LOOKUP_BITMAP32 = 0, LOOKUP_BUCKET = 1, LOOKUP_BITMAP64 = 2 };   // (the codes xrl_layer_info reports)

// Row lookup structure of a layer (policy only).  The rank-bitmap costs rows/4 bytes per tile (one load per probe); when that would
// take more than a quarter of the device's free HBM (many tiles x many features, e.g. 32768 leaf tiles over 337k features = 2.8 TB)
// the layer uses a bucket table + binary search over the tile's row ids instead (O(rows of the tile) memory).
// XRL_LOOKUP=bitmap|bitmap64|bucket forces one (tests).
LookupKind choose_lookup(uint32_t w_rows, const TilePlan& tp, bool structure_only) {
    const uint64_t T = tp.tiles.size(), nwords64 = ((uint64_t)w_rows + 63) / 64;
    const uint64_t bm_bytes = T * (((uint64_t)w_rows + 31) / 32) * 8;   // either bitmap: 8 bytes per 32 features
    uint64_t free_b = 0;
    const bool have = free_hbm(free_b);
    const char* lk = std::getenv("XRL_LOOKUP");
    LookupKind kind = LOOKUP_BITMAP32;
    if (structure_only) kind = LOOKUP_BUCKET;
    else if (lk && !std::strcmp(lk, "bucket")) kind = LOOKUP_BUCKET;
    else if (lk && !std::strcmp(lk, "bitmap")) kind = LOOKUP_BITMAP32;
    else if (lk && !std::strcmp(lk, "bitmap64")) kind = LOOKUP_BITMAP64;
    else if (have ? bm_bytes > free_b / 4 : bm_bytes > (48ull << 30)) kind = LOOKUP_BUCKET;
    else if (T > 0 && tp.nnz > 0) {
        // sparse tiles: at most ~4 rows per 64-feature word on average -> most hits are the first row of their word,
        // and the 64-feature word (same bytes per feature) hands back that row's extent with the probe
        uint64_t rows_ub = 0;   // sum over tiles of distinct rows <= sum of column nnz; exact count comes later, this is a cheap bound
        for (uint64_t t = 0; t < T; ++t) rows_ub += std::min<uint64_t>(tp.tile_nnz[t], w_rows);
        if (rows_ub <= 4ull * T * nwords64) kind = LOOKUP_BITMAP64;
    }
    const uint64_t need = (kind == LOOKUP_BUCKET ? 0 : bm_bytes) + tp.nnz * 8;
    if (have && need > (uint64_t)(free_b * 0.9))
        fail("layer: the device layout needs " + std::to_string(need >> 20) + " MiB (" + std::to_string(T) + " tiles x " + std::to_string(w_rows) +
             " features) but only " + std::to_string(free_b >> 20) + " MiB of HBM are free");
    if (kind == LOOKUP_BITMAP64 && w_rows >= (1u << 25)) kind = LOOKUP_BITMAP32;   // the hit queue packs a row slot into 25 bits in that mode
    return kind;
}

struct TileRows {
    std::vector<std::vector<uint32_t>> rows, rptr;   // per tile: its distinct feature rows (ascending), and their packed (CSR) starts [nrows + 1]
    std::vector<Entry> entries;                      // packed: tile t's rows back to back from the ent_base of plan_tiles
    std::vector<BmWord> bitmap;                      // [T * nwords] with want_bm32, else empty
    std::vector<uint32_t> row_idx;                   // rows[] of all tiles, concatenated, + one readable element past the end
    uint64_t total_rows = 0;
    uint32_t max_rows = 0;                           // largest nrows of a tile
};

// Transposes every tile (rows ascending, columns ascending inside a row) and completes its TileDesc: nrows, bias_slot, rowptr_base.
TileRows gather_tile_rows(const HostCsc& W, TilePlan& tp, bool has_bias, bool want_bm32, uint32_t nwords) {
    const uint32_t T = (uint32_t)tp.tiles.size();
    TileRows tr;
    tr.rows.resize(T); tr.rptr.resize(T);
    tr.entries.resize(tp.nnz);
    if (want_bm32) tr.bitmap.assign((uint64_t)T * nwords, BmWord{0, 0});
    parallel_for(T, [&](size_t t) {
        TileDesc& td = tp.tiles[t];
        std::vector<Nz> nz;
        nz.reserve(tp.tile_nnz[t]);
        for (uint32_t c = td.col_begin; c < td.col_begin + td.ncols; ++c) {
            const uint32_t oc = tp.orig_col(c);
            for (uint64_t e = W.col_ptr[oc]; e < W.col_ptr[oc + 1]; ++e) {
                const uint32_t r = W.row_idx[e];
                if (r >= W.rows) fail("layer: W row index out of range");
                nz.push_back(Nz{r, c - td.col_begin, W.val[e]});
            }
        }
        // rows ascending; inside a row the column order (ascending) is kept: stable
        std::stable_sort(nz.begin(), nz.end(), [](const Nz& a, const Nz& b) { return a.row < b.row; });
        auto& rows = tr.rows[t]; auto& rptr = tr.rptr[t];
        BmWord* bm = want_bm32 ? tr.bitmap.data() + t * (uint64_t)nwords : nullptr;
        Entry* ent = tr.entries.data() + td.ent_base;
        for (size_t i = 0; i < nz.size(); ++i) {
            if (i == 0 || nz[i].row != nz[i - 1].row) {
                rows.push_back(nz[i].row);
                rptr.push_back((uint32_t)i);
                if (bm) bm[nz[i].row >> 5].bits |= 1u << (nz[i].row & 31);
            }
            ent[i] = Entry{nz[i].col, nz[i].val};
        }
        rptr.push_back((uint32_t)nz.size());
        td.nrows = (uint32_t)rows.size();
        uint32_t run = 0;
        if (bm) for (uint32_t w = 0; w < nwords; ++w) { bm[w].rank = run; run += (uint32_t)__builtin_popcount(bm[w].bits); }
        // check_bias_explicit, inference.hpp:500-502: last row of the chunk is W's last row
        td.bias_slot = (has_bias && td.nrows > 0 && rows.back() == W.rows - 1) ? td.nrows - 1 : kNoBias;
    });
    for (uint32_t t = 0; t < T; ++t) {
        tp.tiles[t].rowptr_base = tr.total_rows;
        tr.total_rows += tp.tiles[t].nrows;
        tr.max_rows = std::max(tr.max_rows, tp.tiles[t].nrows);
    }
    tr.row_idx.assign(tr.total_rows + 1, 0u);
    parallel_for(T, [&](size_t t) {
        if (!tr.rows[t].empty()) std::memcpy(tr.row_idx.data() + tp.tiles[t].rowptr_base, tr.rows[t].data(), tr.rows[t].size() * 4);
    });
    return tr;
}

struct BucketTable { std::vector<uint32_t> table; uint32_t shift = 0, n = 0, levels = 0; };

// Bucket lookup: per tile, the first row slot of every feature-id range of 2^shift ids; a probe binary-searches `levels` steps inside its bucket.
BucketTable build_bucket_table(const std::vector<std::vector<uint32_t>>& tile_rows, uint32_t w_rows, uint32_t max_rows) {
    const size_t T = tile_rows.size();
    BucketTable b;
    uint32_t want = 16;                                        // ~4 rows per bucket on the fullest tile
    while (want < 4096 && want * 4 < max_rows) want <<= 1;
    while ((((uint64_t)w_rows - 1) >> b.shift) + 1 > want) ++b.shift;
    const uint32_t NBK = b.n = w_rows ? (uint32_t)((((uint64_t)w_rows - 1) >> b.shift) + 1) : 1;
    const uint32_t shift = b.shift;
    b.table.assign(T * (NBK + 1) + 1, 0u);                     // + one readable element past the end
    std::vector<uint32_t> tile_maxlen(T, 0);
    parallel_for(T, [&](size_t t) {
        const std::vector<uint32_t>& rows = tile_rows[t];
        uint32_t* bk = b.table.data() + t * (size_t)(NBK + 1);
        const uint32_t R = (uint32_t)rows.size();
        uint32_t r0 = 0, mx = 0;
        for (uint32_t k = 0; k < NBK; ++k) {
            while (r0 < R && (rows[r0] >> shift) < k) ++r0;
            bk[k] = r0;
            if (k > 0) mx = std::max(mx, bk[k] - bk[k - 1]);
        }
        bk[NBK] = R;
        tile_maxlen[t] = std::max(mx, R - bk[NBK - 1]);
    });
    uint32_t maxlen = 1;
    for (size_t t = 0; t < T; ++t) maxlen = std::max(maxlen, tile_maxlen[t]);
    while ((1u << b.levels) < maxlen) ++b.levels;              // steps of 2^(levels-1) .. 1 cover the longest bucket
    return b;
}

// 64-feature words: bits, the rank (row slot) of the word's first row, and that row's extent.
std::vector<BmWord64> build_bitmap64(const std::vector<std::vector<uint32_t>>& tile_rows, const std::vector<TileDesc>& tiles,
                                     const std::vector<uint32_t>& row_ext, uint32_t nwords64) {
    const size_t T = tiles.size();
    std::vector<BmWord64> bitmap64(T * nwords64 + 1, BmWord64{0u, 0u, 0u, 0u});
    parallel_for(T, [&](size_t t) {
        BmWord64* bw = bitmap64.data() + t * (size_t)nwords64;
        const std::vector<uint32_t>& rows = tile_rows[t];
        const uint32_t* ext = row_ext.data() + tiles[t].rowptr_base;
        for (uint32_t r = 0; r < (uint32_t)rows.size(); ++r) {
            BmWord64& w = bw[rows[r] >> 6];
            if ((w.lo | w.hi) == 0u) {                                         // first row of the word (rows ascend)
                w.rank = r;
                w.ext0 = (ext[r] >> 25) == 0x7Fu ? (0xFE000000u | r) : ext[r];   // a 128-entry row reads like the "slot" marker: send it through the table
            }
            const uint32_t b = rows[r] & 63u;
            if (b < 32) w.lo |= 1u << b; else w.hi |= 1u << (b - 32);
        }
        uint32_t run = 0;                                                   // empty words still need a rank (hits never read it)
        for (uint32_t k = 0; k < nwords64; ++k) { if ((bw[k].lo | bw[k].hi) == 0u) bw[k].rank = run; run = bw[k].rank + (uint32_t)__builtin_popcount(bw[k].lo) + (uint32_t)__builtin_popcount(bw[k].hi); }
    });
    return bitmap64;
}

struct EntryLayout { std::vector<uint32_t> row_ext; std::vector<Entry> entries; };

// Device layout of rows: {start, length} per row, and the entries re-laid so that NO ROW TOUCHES MORE 128-BYTE LINES THAN ITS LENGTH
// REQUIRES (a row that would straddle an extra line starts at the next 16-entry boundary).  K1 is bound by the number of cache lines
// its 8-byte gathers request from the L2; unaligned, a 27-entry row costs 2.7 lines on average instead of 2.  XRL_ROW_ALIGN=0 keeps
// rows packed.  Takes the packed entries (released on return) and moves every tile's ent_base to the new layout.
EntryLayout lay_out_entries(std::vector<TileDesc>& tiles, const std::vector<std::vector<uint32_t>>& tile_rptr, uint64_t total_rows, std::vector<Entry> packed) {
    const uint32_t T = (uint32_t)tiles.size();
    EntryLayout el;
    el.row_ext.assign(total_rows + 2, 0u);
    bool align = env_enabled("XRL_ROW_ALIGN");
    auto lay_out = [&](size_t t, uint32_t* ext) -> uint64_t { return layout_tile_rows(tile_rptr[t].data(), tiles[t].nrows, align, ext); };
    std::vector<uint64_t> dev_base((size_t)T + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint64_t> padded(T, 0);
        parallel_for(T, [&](size_t t) { padded[t] = lay_out(t, nullptr); });
        bool fits = true;
        for (uint32_t t = 0; t < T; ++t) { dev_base[t + 1] = dev_base[t] + padded[t]; fits = fits && padded[t] < (1ull << 25); }
        if (fits || !align) break;
        align = false;                                         // a tile would leave the 25-bit offset range: keep this layer packed
    }
    el.entries.assign(dev_base[T] + 64, Entry{0u, 0.0f});      // + readable elements past the end (unconditional loads)
    parallel_for(T, [&](size_t t) {
        uint32_t* ext = el.row_ext.data() + tiles[t].rowptr_base;
        lay_out(t, ext);
        const Entry* src = packed.data() + tiles[t].ent_base;
        Entry* dst = el.entries.data() + dev_base[t];
        const uint32_t* trp = tile_rptr[t].data();
        for (uint32_t r = 0; r < tiles[t].nrows; ++r) std::memcpy(dst + (ext[r] & 0x1FFFFFFu), src + trp[r], (size_t)((ext[r] >> 25) + 1u) * sizeof(Entry));
    });
    for (uint32_t t = 0; t < T; ++t) tiles[t].ent_base = dev_base[t];
    return el;
}

// Algorithmic bytes of the REFERENCE chunk layout per parent: 8*E_p (entries) + 4*R_p (row_idx) + 4*(R_p+1) (row_ptr as u32)
std::vector<float> chunk_alg_bytes(const TilePlan& tp, const std::vector<std::vector<uint32_t>>& tile_rows) {
    const uint32_t P = (uint32_t)tp.ptile.size() - 1;
    std::vector<float> chunk_alg(P, 0.f);
    for (uint32_t p = 0; p < P; ++p) {
        uint64_t E = 0, R = 0;
        const uint32_t t0 = tp.ptile[p], t1 = tp.ptile[p + 1];
        if (t1 - t0 == 1) { E = tp.tile_nnz[t0]; R = tp.tiles[t0].nrows; }
        else if (t1 > t0) {
            std::vector<uint32_t> u;
            for (uint32_t t = t0; t < t1; ++t) { E += tp.tile_nnz[t]; u.insert(u.end(), tile_rows[t].begin(), tile_rows[t].end()); }
            std::sort(u.begin(), u.end());
            R = std::unique(u.begin(), u.end()) - u.begin();
        }
        chunk_alg[p] = (float)(8.0 * E + 4.0 * R + (R ? 4.0 * (R + 1) : 0.0));
    }
    return chunk_alg;
}

// Bias contribution of every child column: the reference adds fl32(bias * w) to the column's accumulator (inference.hpp:806-811 /
// :824-830); columns without an explicit bias entry add nothing, and acc + (+0.0f) == acc for every reachable acc, so a dense vector
// is equivalent.
std::vector<float> bias_products(const HostCsc& W, const TilePlan& tp, uint32_t n_children, float bias) {
    std::vector<float> bias_prod(n_children, 0.0f);
    if (!(bias > 0.0f)) return bias_prod;
    for (uint32_t c = 0; c < n_children; ++c) {
        const uint32_t oc = tp.orig_col(c);
        for (uint64_t e = W.col_ptr[oc]; e < W.col_ptr[oc + 1]; ++e)
            if (W.row_idx[e] == W.rows - 1) { volatile float pr = bias * W.val[e]; bias_prod[c] = 0.0f + pr; }
    }
    return bias_prod;
}

// Largest weight magnitude times max(1, |bias|) (the bound-pruning guard, xrl_predict.cpp): any inf / NaN makes it +inf
float weight_absmax(const HostCsc& W, float bias) {
    float mx = 0.0f; bool fin = std::isfinite(bias);
    const uint64_t wn = W.col_ptr[W.cols];
    for (uint64_t e = 0; e < wn; ++e) { const float a = std::fabs(W.val[e]); if (!(a <= 3.0e38f)) { fin = false; break; } mx = std::max(mx, a); }
    const float v = fin ? mx * std::max(1.0f, std::fabs(bias)) : INFINITY;
    return v <= 3.0e38f ? v : INFINITY;
}

struct DensePlan {
    bool build = false;
    std::vector<uint32_t> ptile, tcol;   // LayerDev::d_ptile / d_tcol (tcol with two elements past the last tile); empty unless build
    uint32_t gp_log2 = 0, max_tiles = 0, pres_words = 0;
    uint64_t ld = 0;
    uint64_t n_tiles() const { return tcol.size() < 2 ? 0 : tcol.size() - 2; }
};

// DENSE row format (K1Q, xrl_k1q.hip) for layers whose padded dense matrix fits the HBM budget: chunks of <= 64 children are one dense
// tile (padded to a power of two), wider chunks are cut evenly into tiles of <= 32.  The tile format is kept too (it serves beams /
// top-k sizes K1Q cannot hold in registers).  XRL_DENSE=0 disables it, XRL_DENSE_MAX_MB caps one layer's matrix.  A layer the budget
// declines keeps reporting the geometry it would have had (xrl_layer_info).
DensePlan plan_dense_format(const HostCsc& W, const TilePlan& tp, uint32_t n_children, uint32_t max_chunk_cols, bool cols_sorted, bool structure_only) {
    DensePlan dp;
    const bool applies = env_enabled("XRL_DENSE") && n_children > 0 && W.rows > 0 && !structure_only && cols_sorted;
    if (applies) {
        const uint32_t P = (uint32_t)tp.chunk_col.size() - 1, wide = max_chunk_cols;
        uint32_t gp = 1;
        if (wide <= 64) { while (gp < wide) gp <<= 1; } else gp = 32;
        dp.ptile.assign(P + 1, 0);
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t cb = tp.chunk_col[p], n = tp.chunk_col[p + 1] - cb;
            const uint32_t nt = n == 0 ? 0u : (wide <= 64 ? 1u : (n + 31u) / 32u);
            for (uint32_t t = 0; t < nt; ++t) dp.tcol.push_back(cb + (uint32_t)((uint64_t)n * t / nt));
            dp.ptile[p + 1] = (uint32_t)dp.tcol.size();
            dp.max_tiles = std::max(dp.max_tiles, nt);
        }
        dp.tcol.push_back(n_children);
        dp.tcol.push_back(n_children);                     // one readable element past the end
        while ((1u << dp.gp_log2) < gp) ++dp.gp_log2;
        dp.ld = (dp.n_tiles() * gp + 31) & ~31ull;
    }
    // ((w_rows + 1) rows: + one all-kMissing row for features outside the layer)
    dp.build = applies && dp.n_tiles() > 0 && dp.ld < (1ull << 30) && ((uint64_t)W.rows + 1) * dp.ld * 4 <= format_budget("XRL_DENSE_MAX_MB");
    if (!dp.build) { dp.ptile.clear(); dp.tcol.clear(); return dp; }
    // presence words (LayerDev::pres): layers of many narrow dense tiles only (XRL_PRESENCE=0: none)
    if (dp.n_tiles() >= 16 && dp.gp_log2 >= 1 && dp.gp_log2 <= 5 && env_enabled("XRL_PRESENCE")) {
        dp.pres_words = 1; while ((uint64_t)dp.pres_words * 32 < dp.n_tiles()) dp.pres_words <<= 1;
        if (((uint64_t)W.rows + 1) * dp.pres_words * 4 >= (1ull << 31)) dp.pres_words = 0;   // K1Q addresses the whole array through ONE buffer resource
    }
    return dp;
}

struct DenseFlags { bool full = false, regular = false; };   // LayerDev::d_full / d_regular

// Builds the planned dense matrix ON the device from the CSC columns (memset to kMissing + scatter), its presence words and the
// tile -> parent map K1G walks; leaves them in L's buffers.
DenseFlags build_dense_format(const HostCsc& W, const TilePlan& tp, const DensePlan& dp, bool has_bias, Layer& L) {
    const uint32_t c_nnz = L.n_children, P = (uint32_t)tp.ptile.size() - 1;
    std::vector<uint32_t> src_col(c_nnz), dst_off(c_nnz);
    for (uint64_t dt = 0; dt < dp.n_tiles(); ++dt)
        for (uint32_t c = dp.tcol[dt]; c < dp.tcol[dt + 1]; ++c) { src_col[c] = tp.orig_col(c); dst_off[c] = (uint32_t)(dt << dp.gp_log2) + (c - dp.tcol[dt]); }
    DevBuf t_ptr, t_idx, t_val, t_src, t_dst;
    t_ptr.upload(W.col_ptr); t_idx.upload(W.row_idx); t_val.upload(W.val); t_src.upload(src_col); t_dst.upload(dst_off);
    L.d_wd.reserve(((size_t)W.rows + 1) * dp.ld * 4);
    launch_densify(t_ptr.as<uint64_t>(), t_idx.as<uint32_t>(), t_val.as<float>(), t_src.as<uint32_t>(), t_dst.as<uint32_t>(),
                   c_nnz, W.rows, dp.ld, L.d_wd.as<uint32_t>(), nullptr);
    if (dp.pres_words) {
        L.d_pres.reserve(((size_t)W.rows + 1) * dp.pres_words * 4);
        launch_presence(L.d_wd.as<uint32_t>(), dp.ld, W.rows + 1, dp.gp_log2, (uint32_t)dp.n_tiles(), dp.pres_words, L.d_pres.as<uint32_t>(), nullptr);
    }
    XRL_HIP(hipStreamSynchronize(nullptr));
    L.d_dptile.upload(dp.ptile); L.d_dtcol.upload(dp.tcol);
    L.dense_bytes = L.d_wd.cap;
    std::vector<uint32_t> tile_parent(tp.tiles.size(), 0);
    for (uint32_t p = 0; p < P; ++p) for (uint32_t t = tp.ptile[p]; t < tp.ptile[p + 1]; ++t) tile_parent[t] = p;
    L.d_tile_parent.upload(tile_parent);

    DenseFlags f;
    // does every kept child hold a weight for every feature row (dense-input models do)?
    const uint32_t n_feat = has_bias ? W.rows - 1 : W.rows;
    f.full = true;
    for (uint32_t c = 0; f.full && c < c_nnz; ++c) {
        const uint32_t oc = src_col[c];
        uint64_t n = W.col_ptr[oc + 1] - W.col_ptr[oc];
        if (has_bias && n > 0 && W.row_idx[W.col_ptr[oc + 1] - 1] == W.rows - 1) --n;
        f.full = n == n_feat;
    }
    if (dp.max_tiles == 1 && dp.tcol.size() >= (size_t)P + 1) {
        f.regular = (uint64_t)c_nnz == ((uint64_t)P << dp.gp_log2);
        for (uint32_t p = 0; f.regular && p <= P; ++p) f.regular = dp.ptile[p] == p && (p == P || dp.tcol[p] == (p << dp.gp_log2));
    }
    return f;
}

// Uploads the tile format and fills the kernels' view of the layer (LayerDev), dense-format fields included.
void upload_tile_format(Layer& L, const TilePlan& tp, LookupKind lookup, const TileRows& tr, const BucketTable& bucket, const std::vector<BmWord64>& bitmap64,
                        const EntryLayout& el, const std::vector<float>& chunk_alg, const std::vector<float>& bias_prod, const DensePlan& dp, DenseFlags flags) {
    const uint32_t P = (uint32_t)tp.ptile.size() - 1;
    L.d_bias_prod.upload(bias_prod);
    L.d_tiles.upload(tp.tiles); L.d_ptile.upload(tp.ptile); L.d_chunk_col.upload(tp.chunk_col);
    if (lookup == LOOKUP_BITMAP32) L.d_bitmap.upload(tr.bitmap);
    if (lookup == LOOKUP_BUCKET) L.d_bucket.upload(bucket.table);
    if (lookup == LOOKUP_BITMAP64) L.d_bitmap64.upload(bitmap64);
    L.d_row_ptr.upload(el.row_ext); L.d_row_idx.upload(tr.row_idx);
    L.d_entries.upload(el.entries); L.d_chunk_alg.upload(chunk_alg);
    if (!tp.contiguous) {
        std::vector<uint32_t> perm_inv(tp.C->row_idx.begin(), tp.C->row_idx.begin() + L.n_children);
        L.d_perm_inv.upload(perm_inv);
    }
    L.bk_shift = bucket.shift; L.bk_n = bucket.n; L.bk_levels = bucket.levels;

    LayerDev& d = L.dev;
    d.tiles = L.d_tiles.as<TileDesc>(); d.ptile = L.d_ptile.as<uint32_t>(); d.chunk_col = L.d_chunk_col.as<uint32_t>();
    d.bitmap = lookup == LOOKUP_BITMAP32 ? L.d_bitmap.as<BmWord>() : nullptr;
    d.bitmap64 = lookup == LOOKUP_BITMAP64 ? L.d_bitmap64.as<BmWord64>() : nullptr; d.nwords64 = (L.w_rows + 63) / 64;
    d.bucket = lookup == LOOKUP_BUCKET ? L.d_bucket.as<uint32_t>() : nullptr; d.bk_shift = L.bk_shift; d.bk_n = L.bk_n; d.bk_levels = L.bk_levels;
    d.row_ext = L.d_row_ptr.as<uint32_t>(); d.row_idx = L.d_row_idx.as<uint32_t>();
    d.entries = L.d_entries.as<Entry>(); d.perm_inv = tp.contiguous ? nullptr : L.d_perm_inv.as<uint32_t>();
    d.chunk_alg_bytes = L.d_chunk_alg.as<float>();
    d.bias_prod = L.d_bias_prod.as<float>();
    d.n_parents = P; d.n_children = L.n_children; d.n_tiles = L.n_tiles; d.nwords = L.nwords; d.w_rows = L.w_rows;
    d.max_tiles_per_parent = L.max_tiles_per_parent; d.max_tile_cols = L.max_tile_cols;
    d.bias = L.bias; d.has_bias = L.bias > 0.0f ? 1 : 0;
    d.wd = dp.build ? L.d_wd.as<uint32_t>() : nullptr; d.d_ld = dp.ld; d.d_gp_log2 = dp.gp_log2; d.d_max_tiles = dp.max_tiles;
    d.d_ptile = dp.build ? L.d_dptile.as<uint32_t>() : nullptr; d.d_tcol = dp.build ? L.d_dtcol.as<uint32_t>() : nullptr;
    {
        const uint64_t wp = (uint64_t)dp.max_tiles << dp.gp_log2;
        const double per_segment = (P && L.w_rows) ? (double)L.nnz / ((double)L.w_rows * (double)P) : 0.0;   // weights per (feature, parent)
        d.d_sparse_ok = (wp <= 32 || per_segment >= 1.0) ? 1 : 0;
    }
    d.pres = dp.pres_words ? L.d_pres.as<uint32_t>() : nullptr; d.pres_words = dp.pres_words;
    d.d_regular = flags.regular ? 1 : 0;
    d.d_full = flags.full ? 1 : 0; d.tile_parent = dp.build ? L.d_tile_parent.as<uint32_t>() : nullptr;
    d.wt = nullptr; d.wt_base = nullptr; d.wt_stride = 0; d.wt_bytes = 0;
}

// mmap model folders: W and C arrive in the rearranged child order, and `perm_inv` takes rearranged -> original ids
void apply_perm_override(Layer& L, const HostCsc& C, const std::vector<uint32_t>& perm_inv, uint32_t orig_rows) {
    if (perm_inv.size() != L.n_children) fail("layer: perm_inv size does not match C");
    L.d_perm_inv.upload(perm_inv);
    L.dev.perm_inv = L.d_perm_inv.as<uint32_t>();
    L.reordered = true;
    L.c_rows = orig_rows;          // predictions carry ORIGINAL ids; result CSR has perm.size() columns
    // host maps in original ids (predict_on_selected_outputs is CSC-only in the reference; mmap models
    // have no CSC copy, so K4 is unavailable for them, but the maps stay consistent)
    L.h_parent.assign(orig_rows, 0xFFFFFFFFu);
    for (uint32_t p = 0; p < C.cols; ++p) for (uint64_t c = C.col_ptr[p]; c < C.col_ptr[p + 1]; ++c) L.h_parent[perm_inv[C.row_idx[c]]] = p;
    for (auto& v : L.h_c_idx) v = perm_inv[v];
}

// TILE ROWS held densely (K1T, xrl_k1t.hip): built on the device from the tile format just uploaded.  Needs one cell per (row, column)
// (no duplicate row ids inside a weight column), a rank-bitmap lookup (the slots it returns index the rows) and room:
// (rows + tiles) x stride x 4 bytes within the budget of XRL_TILE_ROWS_MAX_MB (Amazon-670K's leaf -- 5 094 rows per 82-column tile,
// most of them single-entry -- takes 16 GB: 22 GB of model instead of 6, +0.2 s of load).  XRL_TILE_ROWS=0 disables it.
void build_tile_rows(Layer& L, const std::vector<TileDesc>& tiles, uint32_t max_rows, LookupKind lookup, bool cols_sorted, bool structure_only) {
    const uint32_t T = (uint32_t)tiles.size();
    if (!env_enabled("XRL_TILE_ROWS") || structure_only || lookup == LOOKUP_BUCKET || T == 0 || L.nnz == 0 || L.max_tile_cols > kMaxTileCols || !cols_sorted) return;
    int g = 0, nr = 0;
    k1t_shape(L.max_tile_cols, g, nr);
    const uint64_t stride = (uint64_t)g * nr;
    const uint64_t floats = (L.total_rows + T) * stride;
    if (nr > 4 || floats * 4 > format_budget("XRL_TILE_ROWS_MAX_MB") || ((uint64_t)max_rows + 1) * stride * 4 >= (1ull << 32)) return;   // (a row's byte offset inside its tile is 32 bits)
    std::vector<uint64_t> base(T);
    for (uint32_t t = 0; t < T; ++t) base[t] = (tiles[t].rowptr_base + t) * stride;
    L.d_wt_base.upload(base);
    L.d_wt.reserve(floats * 4 + 64);
    LayerDev& d = L.dev;
    d.wt_base = L.d_wt_base.as<uint64_t>(); d.wt_stride = (uint32_t)stride;
    launch_tile_rows(d, floats + 16, L.d_wt.as<uint32_t>(), nullptr);
    XRL_HIP(hipStreamSynchronize(nullptr));
    d.wt = L.d_wt.as<float>(); d.wt_bytes = floats * 4 + 64;
}

}  // namespace

std::unique_ptr<Layer> compile_layer(const HostCsc& W_full, const HostCsc& C, float bias, uint32_t only_topk,
                                     const std::string& post_processor, const std::vector<uint32_t>* perm_inv_override,
                                     uint32_t orig_rows, bool structure_only) {
    // structure_only: compile the same tree around an EMPTY weight pattern (no tile rows, no dense matrix, tiny bucket tables)
    HostCsc W_empty;
    if (structure_only) { W_empty.rows = W_full.rows; W_empty.cols = W_full.cols; W_empty.col_ptr.assign((size_t)W_full.cols + 1, 0); }
    const HostCsc& W = structure_only ? W_empty : W_full;
    auto L = std::make_unique<Layer>();
    L->w_rows = W.rows; L->w_cols = W.cols; L->c_rows = C.rows; L->c_cols = C.cols;
    L->bias = bias; L->only_topk = only_topk; L->pp_name = post_processor;
    L->pp = parse_post_processor(post_processor.c_str());
    if (C.rows != W.cols) fail("layer: C.rows (" + std::to_string(C.rows) + ") != W.cols (" + std::to_string(W.cols) + ")");
    L->nwords = (W.rows + 31) / 32;
    L->w_absmax = weight_absmax(W_full, bias);
    const bool has_bias = bias > 0.0f;
    const bool cols_sorted = columns_strictly_ascending(W);

    // tile format: column tiles -> row lookup -> rows of every tile -> line-aware entry layout
    TilePlan tp = plan_tiles(W, C, *L);
    const LookupKind lookup = choose_lookup(W.rows, tp, structure_only);
    TileRows tr = gather_tile_rows(W, tp, has_bias, lookup == LOOKUP_BITMAP32, L->nwords);
    L->total_rows = tr.total_rows;
    EntryLayout el = lay_out_entries(tp.tiles, tr.rptr, tr.total_rows, std::move(tr.entries));
    BucketTable bucket;
    std::vector<BmWord64> bitmap64;
    if (lookup == LOOKUP_BUCKET) bucket = build_bucket_table(tr.rows, W.rows, tr.max_rows);
    if (lookup == LOOKUP_BITMAP64) bitmap64 = build_bitmap64(tr.rows, tp.tiles, el.row_ext, (W.rows + 63) / 64);
    const std::vector<float> chunk_alg = chunk_alg_bytes(tp, tr.rows);
    std::vector<std::vector<uint32_t>>().swap(tr.rows);        // the per-tile vectors have had their last reader
    std::vector<std::vector<uint32_t>>().swap(tr.rptr);
    const std::vector<float> bias_prod = bias_products(W, tp, L->n_children, bias);

    // dense row format (K1Q) beside it, where it fits
    const DensePlan dp = plan_dense_format(W, tp, L->n_children, L->max_chunk_cols, cols_sorted, structure_only);
    const DenseFlags dense = dp.build ? build_dense_format(W, tp, dp, has_bias, *L) : DenseFlags{};

    upload_tile_format(*L, tp, lookup, tr, bucket, bitmap64, el, chunk_alg, bias_prod, dp, dense);
    const uint32_t max_rows = tr.max_rows;
    tr = {}; el = {}; bitmap64 = {}; bucket = {};              // the host copies are not held through the tile-row build
    if (tp.contiguous && perm_inv_override) apply_perm_override(*L, C, *perm_inv_override, orig_rows);
    build_tile_rows(*L, tp.tiles, max_rows, lookup, cols_sorted, structure_only);
    L->device_bytes = L->buffer_bytes();
    return L;
}

void ensure_device_csc(Layer& L) {
    if (L.csc_ready) return;
    HostCsc tmp;
    const HostCsc* W = L.w_host.get();
    if (!W) {
        if (L.w_path.empty()) fail("predict_on_selected_outputs: the layer's CSC weights are not available");
        load_csc_npz(L.w_path, tmp);
        W = &tmp;
    }
    const uint64_t models = L.device_bytes - L.buffer_bytes();   // the merged level-0/1 matrix, counted on the root layer (finalize_model)
    L.d_csc_ptr.upload(W->col_ptr); L.d_csc_idx.upload(W->row_idx); L.d_csc_val.upload(W->val);
    L.device_bytes = L.buffer_bytes() + models;
    L.csc_ready = true;
}

void ensure_device_tree(Model& m) {
    if (m.sel_tree_ready) return;
    std::vector<SelectTreeLayer> table(m.layers.size());
    for (size_t l = 0; l < m.layers.size(); ++l) {
        Layer& L = *m.layers[l];
        // from C as stored (original ids): a node's parent is the column that holds it, its crank the position inside that column
        std::vector<uint32_t> parent(L.c_rows, kSelectNone), crank(L.c_rows, 0u);
        std::vector<uint8_t> seen(L.c_rows, 0);
        for (uint32_t p = 0; p + 1 < L.h_c_ptr.size(); ++p)
            for (uint64_t c = L.h_c_ptr[p]; c < L.h_c_ptr[p + 1]; ++c) {
                const uint32_t j = L.h_c_idx[c];
                if (j >= L.c_rows) fail("layer " + std::to_string(l) + ": C holds a row id out of range");
                if (seen[j]) fail("layer " + std::to_string(l) + ": node " + std::to_string(j) + " appears under two parents (C is not a tree)");
                seen[j] = 1;
                parent[j] = (l == 0 && p != 0) ? kSelectNone : p;   // layer 0 hangs under the implicit root, parent 0
                crank[j] = (uint32_t)(c - L.h_c_ptr[p]);
            }
        const uint64_t models = L.device_bytes - L.buffer_bytes();   // (what ensure_device_csc keeps too)
        L.d_sel_parent.upload(parent); L.d_sel_crank.upload(crank);
        L.device_bytes = L.buffer_bytes() + models;
        table[l] = SelectTreeLayer{L.d_sel_parent.as<uint32_t>(), L.d_sel_crank.as<uint32_t>(), L.c_rows, 0u};
    }
    m.d_sel_tree.upload(table);
    m.layers[0]->device_bytes += m.d_sel_tree.cap;
    m.sel_tree_ready = true;
}

void finalize_model(Model& m) {
    if (m.layers.empty()) fail("model has no layers");
    const Layer& last = *m.layers.back();
    // MLModel::{label,code,feature}_count, inference.hpp:2241-2255 (chunked W.cols = #children kept)
    m.nr_labels = last.reordered ? last.n_children : last.w_cols;
    m.nr_codes = last.c_cols;
    m.nr_features = last.bias > 0.0f ? last.w_rows - 1 : last.w_rows;
    for (size_t l = 1; l < m.layers.size(); ++l) {
        const uint32_t prev_out = m.layers[l - 1]->reordered ? m.layers[l - 1]->c_rows : m.layers[l - 1]->w_cols;
        if (m.layers[l]->c_cols != prev_out)
            fail("layer " + std::to_string(l) + ": C.cols (" + std::to_string(m.layers[l]->c_cols) +
                 ") does not match the previous layer's label count (" + std::to_string(prev_out) + ")");
    }
    if (!m.stream) XRL_HIP(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    // levels 0 and 1 in one 64-column dense matrix (LayerDev::wd01): K1Q's fused walk of the two levels then issues ONE load per feature
    if (m.layers.size() >= 2) {
        Layer& L0 = *m.layers[0]; const Layer& L1 = *m.layers[1];
        const LayerDev& d0 = L0.dev; const LayerDev& d1 = L1.dev;
        if (env_enabled("XRL_K1Q_MERGE01") && d0.wd && d1.wd && d0.n_parents == 1 && d0.d_max_tiles == 1 && d0.w_rows == d1.w_rows && d1.n_parents == d0.n_children) {
            const uint64_t K0 = d0.n_children, c1 = (K0 * d1.d_max_tiles) << d1.d_gp_log2;
            // k1q_layer01m reads the merged matrix as ONE buffer resource with 32-bit byte offsets (it has no BIGW form): (w_rows + 1) rows of 256 bytes
            // must stay below the lane offset that switches a lane off, or num_records wraps (exactly 0 at w_rows + 1 == 2^24) and f * 256 aliases onto
            // low rows.  Larger models keep the two levels' own matrices and the two-load walk (k1q_layer01<BIGW>).
            if (K0 >= 1 && c1 + K0 <= 64 && c1 <= d1.d_ld && K0 <= d0.d_ld && k1q_merged01_addressable(d0.w_rows)) {
                m.d_wd01.reserve(((size_t)d0.w_rows + 1) * 64 * 4);
                launch_merge01(d0.wd, d0.d_ld, (uint32_t)K0, d1.wd, d1.d_ld, (uint32_t)c1, d0.w_rows + 1, m.d_wd01.as<uint32_t>(), nullptr);
                XRL_HIP(hipStreamSynchronize(nullptr));
                L0.dev.wd01 = m.d_wd01.as<uint32_t>(); L0.dev.wd01_c1 = (uint32_t)c1;
                L0.device_bytes += m.d_wd01.cap;
            }
        }
    }
}

std::unique_ptr<Model> load_model_from_disk(const std::string& path, int weight_matrix_type) {
    const JsonValue meta = parse_json_file(path + "/param.json");   // HierarchicalMLModelMetadata, inference.hpp:52-99
    const JsonValue* depth_v = meta.get("depth");
    if (!depth_v || depth_v->type != JsonValue::NUMBER) fail(path + "/param.json: missing \"depth\"");
    if (const JsonValue* mm = meta.get("is_mmap"))
        if (mm->type == JsonValue::BOOL && mm->b) fail("This folder contains mmap model. Cannot load in npz format.");
    const int depth = (int)depth_v->num;
    auto m = std::make_unique<Model>();
    XRL_HIP(hipGetDevice(&m->device));
    m->weight_matrix_type = weight_matrix_type;
    m->csc_route = weight_matrix_type == 0;
    for (int d = 0; d < depth; ++d) {
        const std::string lp = path + "/" + std::to_string(d) + ".model";
        const JsonValue p = parse_json_file(lp + "/param.json");     // MLModelMetadata, inference.hpp:101-157
        const JsonValue* bias = p.get("bias");
        const JsonValue* kw = p.get("pred_kwargs");
        if (!bias || bias->type != JsonValue::NUMBER || !kw) fail(lp + "/param.json: missing bias / pred_kwargs");
        const JsonValue* topk = kw->get("only_topk");
        const JsonValue* pp = kw->get("post_processor");
        if (!topk || !pp || pp->type != JsonValue::STRING) fail(lp + "/param.json: missing pred_kwargs.only_topk / post_processor");
        HostCsc W, C;
        load_csc_npz(lp + "/W.npz", W);
        if (d == 0 && !file_exists(lp + "/C.npz")) {   // inference.hpp:1580-1583: root without codes
            C.rows = W.cols; C.cols = 1;
            C.col_ptr = {0, W.cols};
            C.row_idx.resize(W.cols); C.val.assign(W.cols, 1.0f);
            for (uint32_t i = 0; i < W.cols; ++i) C.row_idx[i] = i;
        } else {
            load_csc_npz(lp + "/C.npz", C);
        }
        // weight_matrix_type CSC (pecos/core/base.py:49): the reference then runs w_ops<csc_t> (inference.hpp:1081-1149) --
        // bias first, dot product summed separately -- which differs from the chunked arithmetic in the last bits
        const bool csc = weight_matrix_type == 0;
        m->layers.push_back(compile_layer(W, C, (float)bias->num, (uint32_t)topk->num, pp->str, nullptr, 0, csc));
        m->layers.back()->w_path = lp + "/W.npz";
        if (csc) m->layers.back()->w_host = std::make_shared<HostCsc>(std::move(W));
    }
    finalize_model(*m);
    return m;
}

}  // namespace xrl
