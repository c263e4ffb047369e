// K9: the tokenizer and the term counts of the TF-IDF producer on the device (the host half is TfidfBase::count, xrl_tfidf.cpp; both
// read the same tables through the same lookups, xrl_tfidf_tables.h).
//
//   k9_count<BIG>    one wavefront per (document, base vectorizer) segment.  Lanes take consecutive bytes, 64 per step:
//                    word mode    ballot of ' '; a token starts at a non-space byte after a space or the document start (one carry bit
//                                 between steps); its ordinal is the running count + the starts below the lane; the lane that owns a start
//                                 finds the end (from the mask, or past the step by walking bytes) and looks the token up
//                    char modes   a token starts at every byte that is not 10xxxxxx and takes the size its lead byte names, cut at the buffer
//                                 end; the same lane checks that the bytes it covers are continuation bytes and that the next one is not:
//                                 the lowest position that fails sets the document's status (1 / 2, xrl_tokenize.h) and empties the row
//                    then every n in [min_ngram, min(max_ngram, max_n, T)] at every position through uni / packed / gen by the host's rule.
//                    BIG = false  (the LDS form: segments whose bounds are <= kTokCap) token indices and feature-id occurrences stay in LDS;
//                                 a bitonic sort, run heads by ballot, runs written to the batch's scratch at the prefix of the bounds
//                    BIG = true   (the global form) token indices in HBM; every (n, position) owns one slot of a key array pre-filled with a
//                                 sentinel and writes (segment << 32 | id) on a hit
//   global form, per batch: rocPRIM radix sort of the keys, run-length encode, k9_big_runs scatters the runs to the same scratch
//   k9_mask_bad      documents with a status keep no entry in any base
//   exclusive scan of the segment lengths (rocPRIM), the shared row copy (xrl_devprim.h) moves the runs to their final place
//
// No kernel reads a document byte at or past doc + len, and no lane writes outside the bound its segment was given (each index is below
// tft::token_bound / occurrence_bound of the document's length, which size the arrays).
#include "xrl_tokenize.h"
#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_token_walk.h"

#include <algorithm>
#include <cstdlib>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

namespace xrl {

namespace {

constexpr const char* kWhat = "tfidf (device tokenizer)";   // the family in a "grid too large" message

struct K9Args {
    tft::TokenView tv; tft::NgramView gv;
    int tok_type, n_lo, max_ngram, max_length;
    uint32_t col_off, nb, b;
    const uint8_t* text; const uint64_t* doc_off; const uint64_t* doc_len;
    uint32_t doc0;                                         // LDS form: block x serves document doc0 + x
    const uint32_t* big_doc; uint32_t big0;                // global form: block x serves document big_doc[big0 + x], its keys carry segment big0 + x
    const uint64_t* seg_base;                              // [batch segments + 1] run scratch prefix; segment (d - doc0) * nb + b
    uint32_t* run_col; float* run_cnt;
    uint64_t* seg_cnt;                                     // [nr_doc * nb + 1], by absolute segment
    uint32_t* status;                                      // [nr_doc]
    int32_t* g_tok; const uint64_t* tok_base; uint64_t* keys; const uint64_t* key_base;   // global form
};

// feature id + 1 of the n-gram at t (0: none), TfidfBase::count's rule
__device__ uint32_t ngram_id1(const tft::NgramView& G, const int32_t* t, int n, bool packable, bool in_packed, bool in_gen) {
    if (n == 1) {
        const int32_t x = t[0];
        if (x >= 0 && (uint64_t)x < G.uni_size) return G.uni[x];
        if (x >= 0) {
            if (in_packed && x <= G.max_tok) { const uint64_t k = (uint64_t)(uint32_t)x + 1u; return tft::find_packed(G, k, tft::packed_slot(G.p_shift, k)); }
            return tft::kNone;
        }
        return in_gen ? tft::find_gen(G, t, 1, tft::gen_hash(t, 1)) : tft::kNone;
    }
    bool good = true;                                      // the host's run[i] >= n
    for (int i = 0; i < n; ++i) good &= t[i] >= 0 && t[i] <= G.max_tok;
    if (in_packed && good) { const uint64_t k = tft::pack(G.pack_bits, t, n); return tft::find_packed(G, k, tft::packed_slot(G.p_shift, k)); }
    if (in_gen && (packable ? !good : (good || G.negative_keys))) return tft::find_gen(G, t, n, tft::gen_hash(t, n));
    return tft::kNone;
}

template <bool BIG>
__global__ void __launch_bounds__(64) k9_count(K9Args a) {
    __shared__ int32_t s_tok[BIG ? 1 : kTokCap];
    __shared__ uint32_t s_occ[BIG ? 1 : kTokCap];
    const uint32_t lane = threadIdx.x;
    const uint32_t d = BIG ? a.big_doc[a.big0 + blockIdx.x] : a.doc0 + blockIdx.x;
    const uint64_t len = a.doc_len[d];
    const bool big = tok_segment_is_big(a.tok_type, a.max_length, a.n_lo, a.max_ngram, a.gv.max_n, len);
    if (big != BIG) return;                                // (the host lists exactly the big documents for the global form)
    const uint64_t seg = (uint64_t)d * a.nb + a.b;
    const uint64_t tb = tft::token_bound(a.tok_type, a.max_length, len);
    const char* const doc = reinterpret_cast<const char*>(a.text) + a.doc_off[d];
    int32_t* const tok = BIG ? a.g_tok + a.tok_base[a.big0 + blockIdx.x] : s_tok;

    // ---- tokens (the walk: xrl_token_walk.h)
    uint32_t status = 0;
    const uint64_t count = tokw::walk_tokens(doc, len, a.tok_type, tb, lane, status, [&](uint64_t ord, uint64_t pos, uint64_t n) {
        int32_t t;
        if (n <= 8) {
            const uint64_t key = tft::load_key(doc + pos, (size_t)n, doc + len);
            t = tft::find_short(a.tv, key, (uint32_t)n, tft::short_slot(a.tv.s_shift, key, (uint32_t)n));
        } else t = tft::find_long(a.tv, doc + pos, (size_t)n, tft::hash_long(doc + pos, (size_t)n));
        tok[ord] = t;
    });
    if (status) {
        if (lane == 0) {
            a.seg_cnt[seg] = 0;
            if (status == 1) a.status[d] = 1u; else atomicCAS(&a.status[d], 0u, 2u);      // (1 wins: the host fails when any base does)
        }
        return;
    }
    const uint64_t T = count < tb ? count : tb;
    __syncthreads();                                       // one wavefront per workgroup: the tokens are written

    // ---- n-grams
    const int n_hi = tft::ngram_hi(a.max_ngram, a.gv.max_n, T);
    uint32_t nf = 0;
    uint64_t slot = BIG ? a.key_base[a.big0 + blockIdx.x] : 0;
    const uint64_t key_hi = (uint64_t)(a.big0 + blockIdx.x) << 32;
    for (int n = a.n_lo; n <= n_hi; ++n) {
        const uint64_t cnt = T - (uint64_t)n + 1;
        const bool packable = n <= a.gv.pack_max_n;
        const bool in_packed = packable && (a.gv.packed_n_mask & tft::n_bit(n)) != 0;
        const bool in_gen = (a.gv.gen_n_mask & tft::n_bit(n)) != 0 && (!packable || a.gv.negative_keys);
        for (uint64_t i0 = 0; i0 < cnt; i0 += 64u) {
            const uint64_t i = i0 + lane;
            const uint32_t id1 = i < cnt ? ngram_id1(a.gv, tok + i, n, packable, in_packed, in_gen) : tft::kNone;
            if (BIG) { if (id1) a.keys[slot + i] = key_hi | (uint64_t)(id1 - 1u); }
            else {
                const unsigned long long m = __ballot(id1 != 0);
                if (id1) s_occ[nf + lanes_below(m)] = id1 - 1u;
                nf += (uint32_t)__popcll(m);
            }
        }
        slot += cnt;
    }
    if (BIG) { if (lane == 0) a.seg_cnt[seg] = 0; return; }   // (k9_big_runs writes the length of a segment that holds a run)

    // ---- LDS form: sort, run heads, runs
    if (nf == 0) { if (lane == 0) a.seg_cnt[seg] = 0; return; }
    uint32_t P = 64;
    while (P < nf) P <<= 1;
    for (uint32_t i = nf + lane; i < P; i += 64u) s_occ[i] = 0xFFFFFFFFu;       // (a feature id is below nr_features <= 2^32 - 1)
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64u) {
                const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const uint32_t x = s_occ[lo], y = s_occ[hi];
                if ((x > y) == ((lo & k) == 0)) { s_occ[lo] = y; s_occ[hi] = x; }
            }
            __syncthreads();
        }
    uint32_t* const heads = reinterpret_cast<uint32_t*>(s_tok);                 // (the tokens are no longer read)
    uint32_t nr = 0;
    for (uint32_t i0 = 0; i0 < nf; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const bool head = i < nf && (i == 0 || s_occ[i] != s_occ[i - 1]);
        const unsigned long long m = __ballot(head);
        if (head) heads[nr + lanes_below(m)] = i;
        nr += (uint32_t)__popcll(m);
    }
    __syncthreads();
    const uint64_t base = a.seg_base[(uint64_t)(d - a.doc0) * a.nb + a.b];
    for (uint32_t r = lane; r < nr; r += 64u) {
        const uint32_t h = heads[r], e = r + 1 < nr ? heads[r + 1] : nf;
        a.run_col[base + r] = s_occ[h] + a.col_off;
        a.run_cnt[base + r] = (float)min(e - h, tft::kCountCap);
    }
    if (lane == 0) a.seg_cnt[seg] = nr;
}

__global__ void __launch_bounds__(256) k9_fill(uint64_t* p, uint64_t n, uint64_t v) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) p[i] = v;
}

// the runs of the sorted keys of the global form -> the batch's run scratch and the lengths of their segments
__global__ void __launch_bounds__(256)
k9_big_runs(const uint64_t* __restrict__ uniq, const uint32_t* __restrict__ runlen, const uint32_t* __restrict__ n_runs, uint32_t n_big,
            const uint64_t* __restrict__ big_seg, uint64_t seg0, const uint64_t* __restrict__ seg_base, const uint32_t* __restrict__ col_off, uint32_t nb,
            uint32_t* __restrict__ run_col, float* __restrict__ run_cnt, uint64_t* __restrict__ seg_cnt) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t nr = *n_runs;
    if (r >= nr) return;
    const uint64_t u = uniq[r];
    const uint64_t sb = u >> 32;
    if (sb >= n_big) return;                               // the sentinel's run
    const uint32_t first = lower_bound(uniq, nr, sb << 32);
    const uint64_t gseg = big_seg[sb];
    const uint64_t at = seg_base[gseg - seg0] + ((uint32_t)r - first);
    run_col[at] = (uint32_t)u + col_off[gseg % nb];
    run_cnt[at] = (float)min(runlen[r], tft::kCountCap);
    if ((uint32_t)r == first) seg_cnt[gseg] = lower_bound(uniq, nr, (sb + 1) << 32) - first;
}

__global__ void __launch_bounds__(256) k9_mask_bad(const uint32_t* __restrict__ status, uint64_t seg0, uint64_t n_seg, uint32_t nb, uint64_t* __restrict__ seg_cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_seg && status[(seg0 + i) / nb] != 0u) seg_cnt[seg0 + i] = 0;
}

__global__ void __launch_bounds__(256) k9_first_bad(const uint32_t* __restrict__ status, uint64_t n, unsigned long long* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = status[i];
    if (st == 1u || st == 2u) atomicMin(&first[st - 1u], (unsigned long long)i);
}

__global__ void __launch_bounds__(256) k9_row_ptr(const uint64_t* __restrict__ seg_ptr, uint32_t nb, uint32_t rows, uint64_t* __restrict__ row_ptr) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r <= rows) row_ptr[r] = seg_ptr[r * nb];
}

}  // namespace

void launch_seg_to_row_ptr(const uint64_t* seg_ptr, uint32_t nb, uint32_t rows, uint64_t* row_ptr, hipStream_t s) {
    hipLaunchKernelGGL(k9_row_ptr, dim3(blocks_of((uint64_t)rows + 1, 256, kWhat)), dim3(256), 0, s, seg_ptr, nb, rows, row_ptr);
    XRL_LAUNCH_CHECK();
}

void tokenize_count_device(const std::vector<TokBase>& bases, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                           const uint64_t* h_doc_len, uint64_t nr_doc, uint32_t* d_status, hipStream_t s, TokCounts& out) {
    const uint32_t nb = (uint32_t)bases.size();
    if (nb == 0) fail("tfidf (device tokenizer): no base vectorizer");
    if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
    const uint64_t n_seg = nr_doc * nb;
    std::vector<uint64_t> len_copy;
    if (!h_doc_len) {
        len_copy.resize(nr_doc);
        XRL_HIP(hipMemcpyAsync(len_copy.data(), d_doc_len, nr_doc * 8, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        h_doc_len = len_copy.data();
    }
    DevBuf d_seg_cnt, d_col_off, d_words, d_tmp;
    d_seg_cnt.reserve((n_seg + 1) * 8);
    XRL_HIP(hipMemsetAsync(d_seg_cnt.p, 0, (n_seg + 1) * 8, s));
    if (nr_doc) XRL_HIP(hipMemsetAsync(d_status, 0, nr_doc * 4, s));
    { std::vector<uint32_t> co(nb); for (uint32_t b = 0; b < nb; ++b) co[b] = bases[b].col_off; d_col_off.upload(co); }
    d_words.reserve(32);                                   // [0, 16) first_bad, [24, 28) the runs of a batch's global form
    XRL_HIP(hipMemsetAsync(d_words.p, 0xFF, 16, s));

    uint64_t budget = kTokScratchEntries;
    if (const char* e = std::getenv("XRL_TOK_SCRATCH_ENTRIES")) budget = std::strtoull(e, nullptr, 10);   // (tests: a small budget cuts a small corpus into batches)
    std::vector<DevCsr> pieces;                            // a batch's (idx, val, nnz); no ptr
    DevBuf d_seg_base, d_local_ptr, d_run_col, d_run_cnt, d_big_doc, d_big_seg, d_tok_base, d_key_base, d_tok, d_keys, d_keys2, d_uniq, d_runlen;
    std::vector<uint64_t> seg_base, tok_base, key_base, big_seg;
    std::vector<uint32_t> big_doc;
    std::vector<std::vector<uint32_t>> big(nb);
    std::vector<uint64_t> fb(nb);
    for (uint64_t d0 = 0; d0 < nr_doc;) {
        // ---- the batch: documents [d0, d1), the run scratch prefix of their segments, the documents of the global form per base
        seg_base.assign(1, 0);
        for (auto& v : big) v.clear();
        uint64_t d1 = d0;
        while (d1 < nr_doc && d1 - d0 < kTokBatchDocs) {
            uint64_t add = 0;
            for (uint32_t b = 0; b < nb; ++b) {
                const TokBase& B = bases[b];
                const uint64_t tb = tft::token_bound(B.tok_type, B.max_length, h_doc_len[d1]);
                fb[b] = tft::occurrence_bound(tb, B.min_ngram, tft::ngram_hi(B.max_ngram, B.gv.max_n, tb));
                add += fb[b];
            }
            if (d1 > d0 && seg_base.back() + add > budget) break;
            for (uint32_t b = 0; b < nb; ++b) {
                const TokBase& B = bases[b];
                seg_base.push_back(seg_base.back() + fb[b]);
                if (tok_segment_is_big(B.tok_type, B.max_length, B.min_ngram, B.max_ngram, B.gv.max_n, h_doc_len[d1])) big[b].push_back((uint32_t)d1);
            }
            ++d1;
        }
        const uint64_t nd = d1 - d0, seg0 = d0 * nb, nsb = nd * nb, scratch = seg_base.back();
        big_doc.clear(); big_seg.clear(); tok_base.assign(1, 0); key_base.assign(1, 0);
        std::vector<uint32_t> big0(nb, 0);
        for (uint32_t b = 0; b < nb; ++b) {
            const TokBase& B = bases[b];
            big0[b] = (uint32_t)big_doc.size();
            for (uint32_t d : big[b]) {
                const uint64_t tb = tft::token_bound(B.tok_type, B.max_length, h_doc_len[d]);
                big_doc.push_back(d); big_seg.push_back((uint64_t)d * nb + b);
                tok_base.push_back(tok_base.back() + tb);
                key_base.push_back(key_base.back() + tft::occurrence_bound(tb, B.min_ngram, tft::ngram_hi(B.max_ngram, B.gv.max_n, tb)));
            }
        }
        const uint64_t n_big = big_doc.size(), n_keys = key_base.back();
        if (n_keys > 0x7FFFFFFFull) fail("tfidf (device tokenizer): a document holds more than 2^31 n-gram positions; use the host tokenizer");
        out.global_segments += n_big; out.lds_segments += nsb - n_big; ++out.batches;

        d_seg_base.upload(seg_base);
        d_run_col.reserve(scratch * 4); d_run_cnt.reserve(scratch * 4);
        K9Args a{};
        a.text = d_text; a.doc_off = d_doc_off; a.doc_len = d_doc_len; a.doc0 = (uint32_t)d0; a.nb = nb;
        a.seg_base = d_seg_base.as<uint64_t>(); a.run_col = d_run_col.as<uint32_t>(); a.run_cnt = d_run_cnt.as<float>();
        a.seg_cnt = d_seg_cnt.as<uint64_t>(); a.status = d_status;
        if (n_big) {
            d_big_doc.upload(big_doc); d_big_seg.upload(big_seg); d_tok_base.upload(tok_base); d_key_base.upload(key_base);
            d_tok.reserve(tok_base.back() * 4); d_keys.reserve(n_keys * 8); d_keys2.reserve(n_keys * 8);
            a.big_doc = d_big_doc.as<uint32_t>(); a.g_tok = d_tok.as<int32_t>(); a.tok_base = d_tok_base.as<uint64_t>();
            a.keys = d_keys.as<uint64_t>(); a.key_base = d_key_base.as<uint64_t>();
            if (n_keys) { hipLaunchKernelGGL(k9_fill, dim3(blocks_of(n_keys, 256, kWhat)), dim3(256), 0, s, a.keys, n_keys, n_big << 32); XRL_LAUNCH_CHECK(); }
        }
        for (uint32_t b = 0; b < nb; ++b) {
            const TokBase& B = bases[b];
            a.tv = B.tv; a.gv = B.gv; a.tok_type = B.tok_type; a.n_lo = B.min_ngram; a.max_ngram = B.max_ngram; a.max_length = B.max_length;
            a.col_off = B.col_off; a.b = b; a.big0 = big0[b];
            if (big[b].size() < nd) { hipLaunchKernelGGL(k9_count<false>, dim3((uint32_t)nd), dim3(64), 0, s, a); XRL_LAUNCH_CHECK(); }
            if (!big[b].empty()) { hipLaunchKernelGGL(k9_count<true>, dim3((uint32_t)big[b].size()), dim3(64), 0, s, a); XRL_LAUNCH_CHECK(); }
        }
        if (n_keys) {
            // ---- global form: sort the (segment, id) keys (the sentinel n_big << 32 sorts last), run lengths, scatter
            unsigned end_bit = 33;
            while (end_bit < 64 && (n_big >> (end_bit - 32)) != 0) ++end_bit;
            with_rocprim_tmp(d_tmp, [&](void* t, size_t& bytes) {
                return rocprim::radix_sort_keys(t, bytes, d_keys.as<uint64_t>(), d_keys2.as<uint64_t>(), (unsigned int)n_keys, 0u, end_bit, s);
            });
            d_uniq.reserve(n_keys * 8); d_runlen.reserve(n_keys * 4);
            uint32_t* const d_n_runs = d_words.as<uint32_t>() + 6;
            with_rocprim_tmp(d_tmp, [&](void* t, size_t& bytes) {
                return rocprim::run_length_encode(t, bytes, d_keys2.as<uint64_t>(), (unsigned int)n_keys, d_uniq.as<uint64_t>(), d_runlen.as<uint32_t>(), d_n_runs, s);
            });
            hipLaunchKernelGGL(k9_big_runs, dim3(blocks_of(n_keys, 256, kWhat)), dim3(256), 0, s, d_uniq.as<uint64_t>(), d_runlen.as<uint32_t>(), d_n_runs, (uint32_t)n_big,
                               d_big_seg.as<uint64_t>(), seg0, d_seg_base.as<uint64_t>(), d_col_off.as<uint32_t>(), nb, a.run_col, a.run_cnt, a.seg_cnt);
            XRL_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k9_mask_bad, dim3(blocks_of(nsb, 256, kWhat)), dim3(256), 0, s, d_status, seg0, nsb, nb, a.seg_cnt);
        XRL_LAUNCH_CHECK();
        // ---- the batch's entries: lengths -> offsets inside the batch (the count after the batch's last is still zero), then the copy
        d_local_ptr.reserve((nsb + 1) * 8);
        DevCsr pc;
        pc.nnz = scan_total(d_tmp, a.seg_cnt + seg0, d_local_ptr.as<uint64_t>(), nsb, s);
        pc.idx.reserve(pc.nnz * 4); pc.val.reserve(pc.nnz * 4);
        if (pc.nnz) launch_copy_rows(d_local_ptr.as<uint64_t>(), nsb, d_seg_base.as<uint64_t>(), 0, a.run_col, a.run_cnt, pc.idx.as<uint32_t>(), pc.val.as<float>(), kWhat, s);
        pieces.push_back(std::move(pc));
        d0 = d1;
        if (d0 < nr_doc) XRL_HIP(hipStreamSynchronize(s));   // the next batch's uploads reuse the buffers this batch's kernels read
    }

    // ---- the whole call: the pieces side by side (one piece: it is the result), segment pointer, the lowest bad documents
    DevCsr& C = out.csr;
    if (pieces.size() == 1) C = std::move(pieces[0]);
    else {
        C.nnz = 0;
        for (const DevCsr& pc : pieces) C.nnz += pc.nnz;
        C.idx.reserve(C.nnz * 4); C.val.reserve(C.nnz * 4);
        uint64_t at = 0;
        for (const DevCsr& pc : pieces) {
            if (pc.nnz) {
                XRL_HIP(hipMemcpyAsync(C.idx.as<uint32_t>() + at, pc.idx.p, pc.nnz * 4, hipMemcpyDeviceToDevice, s));
                XRL_HIP(hipMemcpyAsync(C.val.as<float>() + at, pc.val.p, pc.nnz * 4, hipMemcpyDeviceToDevice, s));
            }
            at += pc.nnz;
        }
    }
    C.ptr.reserve((n_seg + 1) * 8);
    exclusive_scan(d_tmp, d_seg_cnt.as<uint64_t>(), C.ptr.as<uint64_t>(), (size_t)n_seg + 1, s);
    if (nr_doc) {
        hipLaunchKernelGGL(k9_first_bad, dim3(blocks_of(nr_doc, 256, kWhat)), dim3(256), 0, s, d_status, nr_doc, d_words.as<unsigned long long>());
        XRL_LAUNCH_CHECK();
    }
    XRL_HIP(hipMemcpyAsync(out.first_bad, d_words.p, 16, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
}

}  // namespace xrl
