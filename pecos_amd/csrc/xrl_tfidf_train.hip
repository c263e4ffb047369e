// K15: training of the TF-IDF vectorizer on the device (the rule: pecos/core/utils/tfidf.hpp:558-594, :452-499, :871-957).
//
//   k15_vocab        one wavefront per document walks ALL its tokens (xrl_token_walk.h, no max_length cut) and enters each into an
//                    open-addressing table in HBM.  A slot names a token by one occurrence: (offset in the text) << 24 | length, claimed by
//                    a 64-bit compare-and-swap.  The hash only routes: an occupied slot is compared BYTE BY BYTE against the token at hand,
//                    so the distinct set is exact under any hash (XRL_TFIDF_TRAIN_HASH_BITS cuts it to a few bits in the tests).  The table
//                    starts small and the pass is rerun with a larger one when it fills past one half.  Char-mode status 1 / 2 of the whole
//                    document is noted here.
//   host             the distinct tokens (bytes gathered by k15_vocab_bytes) are sorted with std::string's order: work proportional to the
//                    vocabulary, not the corpus.  Token id = rank.  TokenTable::build makes the lookup tables, uploaded for:
//   k15_df<BIG>      one wavefront per (document, base vectorizer): the walk cut at max_length, token ids through tft::find_short / find_long,
//                    then for every n every position enters a per-document set that holds POSITIONS (equality = the n token ids at the two
//                    positions, read from the token array, so no key is ever half-written); the position that claims a slot emits the
//                    n-gram's key -- the n ids packed most significant first at bits(|V| - 1) bits each, 128 bits -- to the batch's key
//                    array of that n at a wavefront-aggregated atomic offset.  BIG = false keeps tokens and set in LDS (documents of up to
//                    kTokCap tokens: 4 KiB + 8 KiB per wavefront), BIG = true in HBM scratch.
//   per batch and n  rocPRIM radix sort of the keys + run-length encode = (key, documents of the batch that hold it); batches are merged by
//                    sort + reduce-by-key
//   filter / order   the (key, df) lists of all n side by side in ascending n (each ascending by key) + one STABLE radix sort by df = the
//                    reference's order (df, n, token ids); the df range is a contiguous window of it, trimmed to max_feature from either
//                    end; only the kept features come to the host, which unpacks the ids, computes idf and builds NgramTable.
//
// Bounds: a token slot index is below tft::token_bound of the document's length, which sizes the token arrays; a set holds at least twice
// as many slots as positions; a key offset is below the sum of the documents' position counts, which sizes the key array; no document byte
// at or past doc + len is read.  Every probe loop is bounded by the table size.
#include "xrl_tfidf_train.h"
#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_token_walk.h"
#include "xrl_tokenize.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

namespace xrl {

namespace {

constexpr const char* kWhat = "tfidf training";
using key_t = __uint128_t;

struct K15VocabArgs {
    const uint8_t* text; const uint64_t* doc_off; const uint64_t* doc_len;
    uint32_t doc0; int tok_type;
    unsigned long long* table; uint64_t mask, hash_mask;
    unsigned long long* words;   // [0] lowest status-1 document, [1] status-2, [2] distinct tokens, [3] table over half full, [4] long compares, [5] token too long
};

__device__ void vocab_insert(const K15VocabArgs& a, uint64_t gpos, uint64_t n, uint64_t& cmp) {
    if (n > kTrainMaxTokenBytes) { a.words[5] = 1ull; return; }
    const char* const p = reinterpret_cast<const char*>(a.text) + gpos;
    uint64_t h = n <= 8 ? tft::mix(tft::load_le(p, (size_t)n) ^ (n << 56)) * 0xD6E8FEB86659FD93ull : tft::hash_long(p, (size_t)n);
    h = (h >> 20) & a.hash_mask;
    const unsigned long long rep = (unsigned long long)((gpos << 24) | n);
    uint64_t slot = h & a.mask;
    for (uint64_t probes = 0; probes <= a.mask; ++probes, slot = (slot + 1) & a.mask) {
        unsigned long long old = __atomic_load_n(&a.table[slot], __ATOMIC_RELAXED);   // (a frequent token is found by a load, not by an atomic on one hot slot)
        if (old == 0ull) old = atomicCAS(&a.table[slot], 0ull, rep);
        if (old == 0ull) {
            const unsigned long long c = atomicAdd(&a.words[2], 1ull);
            if (2 * (c + 1) > a.mask + 1) a.words[3] = 1ull;
            return;
        }
        if ((old & 0xFFFFFFull) == n) {
            if (n > 8) ++cmp;
            if (tft::same_bytes(reinterpret_cast<const char*>(a.text) + (old >> 24), p, (size_t)n)) return;
        }
    }
    a.words[3] = 1ull;                                     // every slot taken by another token
}

__global__ void __launch_bounds__(64) k15_vocab(K15VocabArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint64_t d = (uint64_t)a.doc0 + blockIdx.x;
    const uint64_t len = a.doc_len[d], off = a.doc_off[d];
    const char* const doc = reinterpret_cast<const char*>(a.text) + off;
    uint32_t status = 0;
    uint64_t cmp = 0;
    tokw::walk_tokens(doc, len, a.tok_type, tft::token_bound(a.tok_type, -1, len), lane, status,
                      [&](uint64_t, uint64_t pos, uint64_t n) { vocab_insert(a, off + pos, n, cmp); });
    if (status && lane == 0) atomicMin(&a.words[status - 1u], (unsigned long long)d);
    for (int o = 32; o > 0; o >>= 1) cmp += (uint64_t)__shfl_down((unsigned int)cmp, o, 64);   // (a count: 32 bits per wavefront are plenty)
    if (lane == 0 && cmp) atomicAdd(&a.words[4], (unsigned long long)(uint32_t)cmp);
}

__global__ void __launch_bounds__(256) k15_vocab_list(const unsigned long long* __restrict__ table, uint64_t slots, unsigned long long* __restrict__ reps,
                                                      uint64_t cap, unsigned long long* __restrict__ counter) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= slots) return;
    const unsigned long long v = table[i];
    if (!v) return;
    const unsigned long long at = atomicAdd(counter, 1ull);
    if (at < cap) reps[at] = v;
}

__global__ void __launch_bounds__(256) k15_vocab_bytes(const uint8_t* __restrict__ text, const unsigned long long* __restrict__ reps, const uint64_t* __restrict__ offs,
                                                       uint64_t n_tok, uint8_t* __restrict__ arena) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_tok) return;
    const uint64_t src = reps[i] >> 24, n = offs[i + 1] - offs[i], dst = offs[i];
    for (uint64_t j = 0; j < n; ++j) arena[dst + j] = text[src + j];
}

struct K15DfArgs {
    tft::TokenView tv;
    int tok_type, n_lo, n_hi, max_length;
    unsigned width; uint64_t hash_mask;
    const uint8_t* text; const uint64_t* doc_off; const uint64_t* doc_len;
    uint32_t doc0;                                         // LDS form: block x serves document doc0 + x
    const uint32_t* big_doc;                               // global form: block x serves document big_doc[x]
    int32_t* g_tok; const uint64_t* tok_base;              // global form: tokens of block x at tok_base[x]
    uint32_t* g_set; const uint64_t* set_base;             // global form: the set of block x, set_base[x + 1] - set_base[x] slots (a power of two)
    key_t* out; const uint64_t* n_base;                    // keys of n-grams of n ids from out[n_base[n - n_lo]]
    unsigned long long* n_cnt;                             // ... how many were written
    uint32_t* err;                                         // a token the vocabulary does not hold (cannot happen: the vocabulary pass saw it)
};

template <bool BIG>
__global__ void __launch_bounds__(64) k15_df(K15DfArgs a) {
    __shared__ int32_t s_tok[BIG ? 1 : kTokCap];
    __shared__ uint32_t s_set[BIG ? 1 : 2 * kTokCap];
    const uint32_t lane = threadIdx.x;
    const uint32_t d = BIG ? a.big_doc[blockIdx.x] : a.doc0 + blockIdx.x;
    const uint64_t len = a.doc_len[d];
    const uint64_t tb = tft::token_bound(a.tok_type, a.max_length, len);
    if ((tb > kTokCap) != BIG) return;                     // (the host lists exactly the long documents for the global form)
    const char* const doc = reinterpret_cast<const char*>(a.text) + a.doc_off[d];
    int32_t* const tok = BIG ? a.g_tok + a.tok_base[blockIdx.x] : s_tok;
    uint32_t* const set = BIG ? a.g_set + a.set_base[blockIdx.x] : s_set;
    const uint64_t slots = BIG ? a.set_base[blockIdx.x + 1] - a.set_base[blockIdx.x] : 2 * kTokCap;

    uint32_t status = 0;
    bool miss = false;
    const uint64_t count = tokw::walk_tokens(doc, len, a.tok_type, tb, lane, status, [&](uint64_t ord, uint64_t pos, uint64_t n) {
        int32_t t;
        if (n <= 8) {
            const uint64_t key = tft::load_key(doc + pos, (size_t)n, doc + len);
            t = tft::find_short(a.tv, key, (uint32_t)n, tft::short_slot(a.tv.s_shift, key, (uint32_t)n));
        } else t = tft::find_long(a.tv, doc + pos, (size_t)n, tft::hash_long(doc + pos, (size_t)n));
        tok[ord] = t;
        miss |= t < 0;
    });
    if (__ballot(miss)) { if (lane == 0) *a.err = 1u; return; }
    const uint64_t T = count < tb ? count : tb;
    __threadfence_block();
    __syncthreads();                                       // one wavefront per workgroup: the tokens are written

    const int n_hi = (uint64_t)a.n_hi < T ? a.n_hi : (int)T;
    for (int n = a.n_lo; n <= n_hi; ++n) {
        const uint64_t cnt = T - (uint64_t)n + 1;
        for (uint64_t i = lane; i < slots; i += 64u) set[i] = 0u;
        __threadfence_block();
        __syncthreads();
        for (uint64_t i0 = 0; i0 < cnt; i0 += 64u) {
            const uint64_t i = i0 + lane;
            bool win = false;
            if (i < cnt) {
                uint64_t slot = ((tft::gen_hash(tok + i, n) >> 20) & a.hash_mask) & (slots - 1);
                for (uint64_t probes = 0; probes < slots; ++probes, slot = (slot + 1) & (slots - 1)) {
                    const uint32_t old = atomicCAS(&set[slot], 0u, (uint32_t)i + 1u);
                    if (old == 0u) { win = true; break; }
                    if (tft::same_tokens(tok + (old - 1u), tok + i, n)) break;
                }
            }
            const unsigned long long m = __ballot(win);
            if (m) {
                const int leader = __builtin_ctzll(m);
                unsigned long long base = 0;
                if ((int)lane == leader) base = atomicAdd(&a.n_cnt[n - a.n_lo], (unsigned long long)__popcll(m));
                const uint32_t blo = (uint32_t)__shfl((int)(uint32_t)base, leader, 64), bhi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), leader, 64);
                if (win) {
                    key_t key = 0;
                    for (int j = 0; j < n; ++j) key = (key << a.width) | (key_t)(uint32_t)tok[i + j];
                    a.out[a.n_base[n - a.n_lo] + (((uint64_t)bhi << 32) | blo) + lanes_below(m)] = key;
                }
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k15_iota_n(uint32_t* __restrict__ idx, uint32_t* __restrict__ nn, uint64_t at, uint64_t n, uint32_t n_val) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) { idx[at + i] = (uint32_t)(at + i); nn[at + i] = n_val; }
}

// of the ascending df[0, m): how many are below lo, how many are at most hi
__global__ void __launch_bounds__(256) k15_df_window(const uint32_t* __restrict__ df, uint64_t m, uint64_t lo, uint64_t hi, unsigned long long* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool in = i < m;
    const uint64_t v = in ? df[i] : 0;
    const unsigned long long below = __ballot(in && v < lo), atmost = __ballot(in && v <= hi);
    if ((threadIdx.x & 63u) == 0) {
        if (below) atomicAdd(&out[0], (unsigned long long)__popcll(below));
        if (atmost) atomicAdd(&out[1], (unsigned long long)__popcll(atmost));
    }
}

__global__ void __launch_bounds__(256) k15_gather(const key_t* __restrict__ keys, const uint32_t* __restrict__ nn, const uint32_t* __restrict__ df_sorted,
                                                  const uint32_t* __restrict__ perm, uint64_t start, uint64_t n, key_t* __restrict__ o_key, uint32_t* __restrict__ o_n,
                                                  uint32_t* __restrict__ o_df) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = perm[start + i];
    o_key[i] = keys[p]; o_n[i] = nn[p]; o_df[i] = df_sorted[start + i];
}

uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = std::getenv(name);
    return e && *e ? std::strtoull(e, nullptr, 10) : dflt;
}
uint64_t hash_mask_from_env() {
    const uint64_t bits = env_u64("XRL_TFIDF_TRAIN_HASH_BITS", 44);
    return bits >= 44 ? (1ull << 44) - 1 : (1ull << bits) - 1;
}
uint64_t now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
uint64_t pow2_at_least(uint64_t n) { uint64_t p = 1; while (p < n) p <<= 1; return p; }

// a (key, count) list in HBM
struct KeyList { DevBuf keys, cnt; uint64_t n = 0; };

// ---- the vocabulary pass: the distinct tokens of all documents under tok_type, sorted
void train_vocab(int tok_type, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, const uint64_t* h_doc_len, uint64_t nr_doc, hipStream_t s,
                 TrainForms& forms, uint64_t first_bad[2], std::vector<std::string>& tokens) {
    uint64_t bound = 0;
    for (uint64_t d = 0; d < nr_doc; ++d) bound += tft::token_bound(tok_type, -1, h_doc_len[d]);
    uint64_t slots = std::min<uint64_t>(pow2_at_least(2 * bound + 2), 1ull << 22);
    slots = std::max<uint64_t>(64, std::min(slots, pow2_at_least(env_u64("XRL_TFIDF_TRAIN_SCRATCH_ENTRIES", slots))));
    DevBuf d_table, d_words;
    d_words.reserve(64);
    unsigned long long w[6];
    for (;;) {
        d_table.reserve(slots * 8);
        XRL_HIP(hipMemsetAsync(d_table.p, 0, slots * 8, s));
        XRL_HIP(hipMemsetAsync(d_words.p, 0xFF, 16, s));
        XRL_HIP(hipMemsetAsync(d_words.as<char>() + 16, 0, 48, s));
        K15VocabArgs a{};
        a.text = d_text; a.doc_off = d_doc_off; a.doc_len = d_doc_len; a.tok_type = tok_type;
        a.table = d_table.as<unsigned long long>(); a.mask = slots - 1; a.hash_mask = hash_mask_from_env(); a.words = d_words.as<unsigned long long>();
        for (uint64_t d0 = 0; d0 < nr_doc; d0 += kTrainBatchDocs) {
            a.doc0 = (uint32_t)d0;
            hipLaunchKernelGGL(k15_vocab, dim3((uint32_t)std::min<uint64_t>(kTrainBatchDocs, nr_doc - d0)), dim3(64), 0, s, a);
            XRL_LAUNCH_CHECK();
        }
        XRL_HIP(hipMemcpyAsync(w, d_words.p, sizeof(w), hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        forms.vocab_docs += nr_doc;
        if (w[5]) fail("xrl_tfidf_train: a token of more than " + std::to_string(kTrainMaxTokenBytes) + " bytes");
        if (!w[3]) break;
        if (slots > (1ull << 40)) fail("xrl_tfidf_train: vocabulary table too large");
        slots <<= 2; ++forms.table_grows;
    }
    forms.long_compares += w[4];
    first_bad[0] = std::min<uint64_t>(first_bad[0], w[0]); first_bad[1] = std::min<uint64_t>(first_bad[1], w[1]);
    tokens.clear();
    const uint64_t nv = w[2];
    if (first_bad[0] != ~0ull || first_bad[1] != ~0ull || nv == 0) return;
    // ---- the distinct tokens to the host: representatives, then their bytes side by side
    DevBuf d_reps, d_offs, d_arena;
    d_reps.reserve(nv * 8);
    XRL_HIP(hipMemsetAsync(d_words.p, 0, 8, s));
    hipLaunchKernelGGL(k15_vocab_list, dim3(blocks_of(slots, 256, kWhat)), dim3(256), 0, s, d_table.as<unsigned long long>(), slots, d_reps.as<unsigned long long>(), nv,
                       d_words.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    std::vector<unsigned long long> reps(nv);
    XRL_HIP(hipMemcpyAsync(reps.data(), d_reps.p, nv * 8, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    std::vector<uint64_t> offs(nv + 1, 0);
    for (uint64_t i = 0; i < nv; ++i) offs[i + 1] = offs[i] + (reps[i] & 0xFFFFFFull);
    d_offs.upload(offs);
    d_arena.reserve(offs[nv]);
    hipLaunchKernelGGL(k15_vocab_bytes, dim3(blocks_of(nv, 256, kWhat)), dim3(256), 0, s, d_text, d_reps.as<unsigned long long>(), d_offs.as<uint64_t>(), nv, d_arena.as<uint8_t>());
    XRL_LAUNCH_CHECK();
    std::string arena(offs[nv], '\0');
    XRL_HIP(hipMemcpyAsync(&arena[0], d_arena.p, offs[nv], hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    tokens.reserve(nv);
    for (uint64_t i = 0; i < nv; ++i) tokens.emplace_back(arena.data() + offs[i], offs[i + 1] - offs[i]);
    std::sort(tokens.begin(), tokens.end());               // std::string::operator<: unsigned bytes, a prefix before its extensions (tfidf.hpp:583-590)
    forms.distinct_tokens += nv;
}

// keys[0, n) (unsorted, overwritten) -> ascending distinct keys and how often each occurred
void sort_and_count(DevBuf& tmp, key_t* keys, uint64_t n, unsigned key_bits, hipStream_t s, KeyList& out) {
    if (n > 0x7FFFFFFFull) fail("xrl_tfidf_train: more than 2^31 n-gram keys in one sort; lower XRL_TFIDF_TRAIN_SCRATCH_ENTRIES");
    DevBuf sorted, uniq, runs, n_runs;
    sorted.reserve(n * 16); uniq.reserve(n * 16); runs.reserve(n * 4); n_runs.reserve(8);
    with_rocprim_tmp(tmp, [&](void* t, size_t& bytes) { return rocprim::radix_sort_keys(t, bytes, keys, sorted.as<key_t>(), (unsigned int)n, 0u, key_bits, s); });
    with_rocprim_tmp(tmp, [&](void* t, size_t& bytes) {
        return rocprim::run_length_encode(t, bytes, sorted.as<key_t>(), (unsigned int)n, uniq.as<key_t>(), runs.as<uint32_t>(), n_runs.as<uint32_t>(), s);
    });
    uint32_t nr = 0;
    XRL_HIP(hipMemcpyAsync(&nr, n_runs.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    out.n = nr;
    out.keys.reserve((size_t)nr * 16); out.cnt.reserve((size_t)nr * 4);
    if (nr) {
        XRL_HIP(hipMemcpyAsync(out.keys.p, uniq.p, (size_t)nr * 16, hipMemcpyDeviceToDevice, s));
        XRL_HIP(hipMemcpyAsync(out.cnt.p, runs.p, (size_t)nr * 4, hipMemcpyDeviceToDevice, s));
        XRL_HIP(hipStreamSynchronize(s));
    }
}

// several (key, count) lists -> one, ascending by key, counts of equal keys added
void merge_lists(DevBuf& tmp, std::vector<KeyList>& pieces, unsigned key_bits, hipStream_t s, KeyList& out) {
    if (pieces.empty()) { out.n = 0; return; }
    if (pieces.size() == 1) { out = std::move(pieces[0]); return; }
    uint64_t n = 0;
    for (const KeyList& p : pieces) n += p.n;
    if (n > 0x7FFFFFFFull) fail("xrl_tfidf_train: more than 2^31 distinct n-grams of one length over the batches");
    DevBuf k0, c0, k1, c1, n_out;
    k0.reserve(n * 16); c0.reserve(n * 4); k1.reserve(n * 16); c1.reserve(n * 4); n_out.reserve(8);
    uint64_t at = 0;
    for (const KeyList& p : pieces) {
        if (!p.n) continue;
        XRL_HIP(hipMemcpyAsync(k0.as<key_t>() + at, p.keys.p, p.n * 16, hipMemcpyDeviceToDevice, s));
        XRL_HIP(hipMemcpyAsync(c0.as<uint32_t>() + at, p.cnt.p, p.n * 4, hipMemcpyDeviceToDevice, s));
        at += p.n;
    }
    with_rocprim_tmp(tmp, [&](void* t, size_t& bytes) {
        return rocprim::radix_sort_pairs(t, bytes, k0.as<key_t>(), k1.as<key_t>(), c0.as<uint32_t>(), c1.as<uint32_t>(), (unsigned int)n, 0u, key_bits, s);
    });
    with_rocprim_tmp(tmp, [&](void* t, size_t& bytes) {
        return rocprim::reduce_by_key(t, bytes, k1.as<key_t>(), c1.as<uint32_t>(), (unsigned int)n, k0.as<key_t>(), c0.as<uint32_t>(), n_out.as<uint32_t>(),
                                      rocprim::plus<uint32_t>(), rocprim::equal_to<key_t>(), s);
    });
    uint32_t nr = 0;
    XRL_HIP(hipMemcpyAsync(&nr, n_out.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    out.n = nr; out.keys = std::move(k0); out.cnt = std::move(c0);
    pieces.clear();
}

// ---- one base vectorizer: df pass, filter, order, trim -> B.features, B.idf
void train_base(TfidfBase& B, const TfidfBaseVectorizerParam& P, const std::vector<std::string>& tokens, const uint8_t* d_text, const uint64_t* d_doc_off,
                const uint64_t* d_doc_len, const uint64_t* h_doc_len, uint64_t nr_doc, hipStream_t s, TrainForms& forms) {
    const uint64_t V = tokens.size();
    const uint64_t t0 = now_us();
    {
        std::vector<std::pair<std::string, int32_t>> items;
        items.reserve(V);
        for (uint64_t i = 0; i < V; ++i) items.emplace_back(tokens[i], (int32_t)i);
        B.vocab.build(items);
    }
    forms.us_vocab += now_us() - t0;
    const uint64_t t1 = now_us();
    unsigned width = 1;
    while (width < 32 && ((V ? V - 1 : 0) >> width) != 0) ++width;
    if ((uint64_t)P.max_ngram * width > (uint64_t)kTrainKeyBits)
        fail("xrl_tfidf_train: n-grams of " + std::to_string(P.max_ngram) + " tokens at " + std::to_string(width) + " bits each (a vocabulary of " + std::to_string(V) +
             " tokens) need more than 128 bits; the largest n that fits is " + std::to_string(kTrainKeyBits / width));
    const int n_lo = P.min_ngram, nN = P.max_ngram - P.min_ngram + 1;
    std::vector<std::vector<KeyList>> pieces((size_t)nN);
    DevBuf d_tmp;

    if (V) {
        // the lookup tables in HBM
        DevBuf d_s, d_l, d_arena, d_words;
        tft::TokenView tv = B.vocab.view();
        d_s.upload_raw(B.vocab.s.data(), B.vocab.s.size() * sizeof(tft::ShortEntry)); tv.s = d_s.as<tft::ShortEntry>();
        if (!B.vocab.l.empty()) { d_l.upload_raw(B.vocab.l.data(), B.vocab.l.size() * sizeof(tft::LongEntry)); tv.l = d_l.as<tft::LongEntry>(); }
        d_arena.upload_raw(B.vocab.arena.data(), B.vocab.arena.size()); tv.arena = d_arena.as<char>();
        d_words.reserve(8);
        XRL_HIP(hipMemsetAsync(d_words.p, 0, 8, s));

        const uint64_t budget = std::max<uint64_t>(1, env_u64("XRL_TFIDF_TRAIN_SCRATCH_ENTRIES", kTrainScratchEntries));
        DevBuf d_out, d_n_base, d_n_cnt, d_big_doc, d_tok_base, d_set_base, d_tok, d_set;
        std::vector<uint64_t> n_base, cntn((size_t)nN), tok_base, set_base, h_cnt((size_t)nN);
        std::vector<uint32_t> big_doc;
        for (uint64_t d0 = 0; d0 < nr_doc;) {
            std::fill(cntn.begin(), cntn.end(), 0);
            big_doc.clear(); tok_base.assign(1, 0); set_base.assign(1, 0);
            uint64_t d1 = d0, total = 0;
            while (d1 < nr_doc && d1 - d0 < kTrainBatchDocs) {
                const uint64_t tb = tft::token_bound(P.tok_type, P.max_length, h_doc_len[d1]);
                const uint64_t add = tft::occurrence_bound(tb, n_lo, tft::ngram_hi(P.max_ngram, P.max_ngram, tb));
                if (d1 > d0 && total + add > budget) break;
                if (tb >= 0x7FFFFFFFull) fail("xrl_tfidf_train: document " + std::to_string(d1) + " may hold 2^31 tokens or more");
                total += add;
                for (int ni = 0; ni < nN && (uint64_t)(n_lo + ni) <= tb; ++ni) cntn[(size_t)ni] += tb - (uint64_t)(n_lo + ni) + 1;
                if (tb > kTokCap) { big_doc.push_back((uint32_t)d1); tok_base.push_back(tok_base.back() + tb); set_base.push_back(set_base.back() + pow2_at_least(2 * tb)); }
                ++d1;
            }
            const uint64_t nd = d1 - d0;
            n_base.assign(1, 0);
            for (int ni = 0; ni < nN; ++ni) n_base.push_back(n_base.back() + cntn[(size_t)ni]);
            forms.df_global += big_doc.size(); forms.df_lds += nd - big_doc.size(); ++forms.batches;

            d_out.reserve(n_base.back() * 16);
            d_n_base.upload(n_base);
            d_n_cnt.reserve((size_t)nN * 8);
            XRL_HIP(hipMemsetAsync(d_n_cnt.p, 0, (size_t)nN * 8, s));
            K15DfArgs a{};
            a.tv = tv; a.tok_type = P.tok_type; a.n_lo = n_lo; a.n_hi = P.max_ngram; a.max_length = P.max_length; a.width = width; a.hash_mask = hash_mask_from_env();
            a.text = d_text; a.doc_off = d_doc_off; a.doc_len = d_doc_len; a.doc0 = (uint32_t)d0;
            a.out = d_out.as<key_t>(); a.n_base = d_n_base.as<uint64_t>(); a.n_cnt = d_n_cnt.as<unsigned long long>(); a.err = d_words.as<uint32_t>();
            if (big_doc.size() < nd) { hipLaunchKernelGGL(k15_df<false>, dim3((uint32_t)nd), dim3(64), 0, s, a); XRL_LAUNCH_CHECK(); }
            if (!big_doc.empty()) {
                d_big_doc.upload(big_doc); d_tok_base.upload(tok_base); d_set_base.upload(set_base);
                d_tok.reserve(tok_base.back() * 4); d_set.reserve(set_base.back() * 4);
                a.big_doc = d_big_doc.as<uint32_t>(); a.g_tok = d_tok.as<int32_t>(); a.tok_base = d_tok_base.as<uint64_t>();
                a.g_set = d_set.as<uint32_t>(); a.set_base = d_set_base.as<uint64_t>();
                hipLaunchKernelGGL(k15_df<true>, dim3((uint32_t)big_doc.size()), dim3(64), 0, s, a);
                XRL_LAUNCH_CHECK();
            }
            uint32_t err = 0;
            XRL_HIP(hipMemcpyAsync(h_cnt.data(), d_n_cnt.p, (size_t)nN * 8, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipMemcpyAsync(&err, d_words.p, 4, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipStreamSynchronize(s));              // (also: the next batch's uploads reuse the buffers this batch's kernels read)
            if (err) fail("xrl_tfidf_train: internal error: the df pass met a token the vocabulary pass did not");
            for (int ni = 0; ni < nN; ++ni) {
                if (h_cnt[(size_t)ni] > cntn[(size_t)ni]) fail("xrl_tfidf_train: internal error: more keys than positions");
                if (!h_cnt[(size_t)ni]) continue;
                KeyList kl;
                sort_and_count(d_tmp, d_out.as<key_t>() + n_base[(size_t)ni], h_cnt[(size_t)ni], std::min<unsigned>(128u, (unsigned)(n_lo + ni) * width), s, kl);
                pieces[(size_t)ni].push_back(std::move(kl));
            }
            d0 = d1;
        }
    }

    forms.us_df += now_us() - t1;
    const uint64_t t2 = now_us();
    // ---- (key, df) of every n side by side in ascending n
    std::vector<KeyList> per_n((size_t)nN);
    uint64_t M = 0;
    for (int ni = 0; ni < nN; ++ni) {
        merge_lists(d_tmp, pieces[(size_t)ni], std::min<unsigned>(128u, (unsigned)(n_lo + ni) * width), s, per_n[(size_t)ni]);
        M += per_n[(size_t)ni].n;
    }
    forms.distinct_ngrams += M;
    if (M > 0xFFFFFFFFull) fail("xrl_tfidf_train: more than 2^32 distinct n-grams");
    uint64_t real_min, real_max;
    tfidf_df_bounds(P, nr_doc, real_min, real_max);
    std::vector<key_t> h_key; std::vector<uint32_t> h_n, h_df;
    uint64_t nr_feat = 0;
    if (M) {
        DevBuf d_keys, d_df, d_nn, d_idx, d_df2, d_perm, d_win;
        d_keys.reserve(M * 16); d_df.reserve(M * 4); d_nn.reserve(M * 4); d_idx.reserve(M * 4); d_df2.reserve(M * 4); d_perm.reserve(M * 4); d_win.reserve(16);
        uint64_t at = 0;
        for (int ni = 0; ni < nN; ++ni) {
            const KeyList& L = per_n[(size_t)ni];
            if (!L.n) continue;
            XRL_HIP(hipMemcpyAsync(d_keys.as<key_t>() + at, L.keys.p, L.n * 16, hipMemcpyDeviceToDevice, s));
            XRL_HIP(hipMemcpyAsync(d_df.as<uint32_t>() + at, L.cnt.p, L.n * 4, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(k15_iota_n, dim3(blocks_of(L.n, 256, kWhat)), dim3(256), 0, s, d_idx.as<uint32_t>(), d_nn.as<uint32_t>(), at, L.n, (uint32_t)(n_lo + ni));
            XRL_LAUNCH_CHECK();
            at += L.n;
        }
        // the stable sort by df keeps (n, key) inside equal df: the reference's order
        with_rocprim_tmp(d_tmp, [&](void* t, size_t& bytes) {
            return rocprim::radix_sort_pairs(t, bytes, d_df.as<uint32_t>(), d_df2.as<uint32_t>(), d_idx.as<uint32_t>(), d_perm.as<uint32_t>(), (unsigned int)M, 0u, 32u, s);
        });
        XRL_HIP(hipMemsetAsync(d_win.p, 0, 16, s));
        hipLaunchKernelGGL(k15_df_window, dim3(blocks_of(M, 256, kWhat)), dim3(256), 0, s, d_df2.as<uint32_t>(), M, real_min, real_max, d_win.as<unsigned long long>());
        XRL_LAUNCH_CHECK();
        unsigned long long win[2];
        XRL_HIP(hipMemcpyAsync(win, d_win.p, 16, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        const uint64_t lo = win[0], hi = std::max<uint64_t>(win[0], win[1]), kept = hi - lo;
        nr_feat = P.max_feature > 0 ? std::min<uint64_t>((uint64_t)P.max_feature, kept) : kept;
        const uint64_t start = P.keep_frequent_feature ? hi - nr_feat : lo;
        if (nr_feat) {
            DevBuf o_key, o_n, o_df;
            o_key.reserve(nr_feat * 16); o_n.reserve(nr_feat * 4); o_df.reserve(nr_feat * 4);
            hipLaunchKernelGGL(k15_gather, dim3(blocks_of(nr_feat, 256, kWhat)), dim3(256), 0, s, d_keys.as<key_t>(), d_nn.as<uint32_t>(), d_df2.as<uint32_t>(),
                               d_perm.as<uint32_t>(), start, nr_feat, o_key.as<key_t>(), o_n.as<uint32_t>(), o_df.as<uint32_t>());
            XRL_LAUNCH_CHECK();
            h_key.resize(nr_feat); h_n.resize(nr_feat); h_df.resize(nr_feat);
            XRL_HIP(hipMemcpyAsync(h_key.data(), o_key.p, nr_feat * 16, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipMemcpyAsync(h_n.data(), o_n.p, nr_feat * 4, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipMemcpyAsync(h_df.data(), o_df.p, nr_feat * 4, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipStreamSynchronize(s));
        }
    }
    // ---- the kept features on the host: token ids out of the keys, idf, the lookup table
    std::vector<int32_t> flat; std::vector<uint64_t> off(1, 0); std::vector<uint32_t> ids;
    B.idf.assign(nr_feat, 0.0f);
    off.reserve(nr_feat + 1); ids.reserve(nr_feat); flat.reserve(nr_feat * (size_t)std::min(P.max_ngram, 4));
    const key_t field = ((key_t)1 << width) - 1;
    for (uint64_t f = 0; f < nr_feat; ++f) {
        const uint32_t n = h_n[f];
        for (uint32_t j = 0; j < n; ++j) flat.push_back((int32_t)(uint32_t)((h_key[f] >> (width * (n - 1 - j))) & field));
        off.push_back(flat.size()); ids.push_back((uint32_t)f);
        B.idf[f] = tfidf_idf(nr_doc, h_df[f], P.smooth_idf, P.add_one_idf);
    }
    B.nr_features = (uint32_t)nr_feat;
    B.features.build(flat, off, ids, V);
    B.sort_shift = 0;
    while (B.sort_shift < 24 && ((nr_feat - (nr_feat > 0)) >> B.sort_shift) > 255) ++B.sort_shift;
    forms.us_order += now_us() - t2;
}

}  // namespace

void tfidf_df_bounds(const TfidfBaseVectorizerParam& p, uint64_t nr_doc, uint64_t& real_min, uint64_t& real_max) {
    const float nd = (float)nr_doc;
    const float lo = p.min_df_ratio * nd, hi = p.max_df_ratio * nd;
    real_min = std::max<uint64_t>((uint64_t)(int64_t)p.min_df_cnt, (uint64_t)std::round(lo));
    real_max = (uint64_t)std::round(hi);
    if (p.max_df_cnt > 0) real_max = std::min<uint64_t>((uint64_t)p.max_df_cnt, real_max);
}

float tfidf_idf(uint64_t nr_doc, uint64_t df, bool smooth_idf, bool add_one_idf) {
    const float q = (float)nr_doc / (float)(df + (uint64_t)smooth_idf);
    return (float)(std::max(std::log((double)q), 0.0) + (double)(float)add_one_idf);
}

void tfidf_train_device(std::vector<TfidfBase>& bases, const std::vector<TfidfBaseVectorizerParam>& params, const uint8_t* d_text, const uint64_t* d_doc_off,
                        const uint64_t* d_doc_len, const uint64_t* h_doc_off, const uint64_t* h_doc_len, uint64_t nr_doc, hipStream_t s, TrainForms& forms,
                        uint64_t first_bad[2]) {
    first_bad[0] = first_bad[1] = ~0ull;
    for (uint64_t d = 0; d < nr_doc; ++d)
        if (h_doc_len[d] > kTrainMaxTextBytes || h_doc_off[d] > kTrainMaxTextBytes - h_doc_len[d])   // (no sum: it could wrap)
            fail("xrl_tfidf_train: text beyond 2^40 bytes (document " + std::to_string(d) + ")");
    std::map<int, std::vector<std::string>> vocab;         // one vocabulary pass per tokenizer type
    const uint64_t t0 = now_us();
    for (const auto& P : params)
        if (!vocab.count(P.tok_type)) train_vocab(P.tok_type, d_text, d_doc_off, d_doc_len, h_doc_len, nr_doc, s, forms, first_bad, vocab[P.tok_type]);
    forms.us_vocab += now_us() - t0;
    if (first_bad[0] != ~0ull || first_bad[1] != ~0ull) return;
    for (size_t b = 0; b < bases.size(); ++b)
        train_base(bases[b], params[b], vocab[params[b].tok_type], d_text, d_doc_off, d_doc_len, h_doc_len, nr_doc, s, forms);
}

}  // namespace xrl
