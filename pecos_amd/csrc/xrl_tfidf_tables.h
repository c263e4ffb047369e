// The TF-IDF producer's lookups, stated once for the host tokenizer (xrl_tfidf.cpp) and the device tokenizer (K9, xrl_tokenize.hip):
// the table entries, plain-pointer views of the tables, and the hash / slot / probe functions over those views.  The host classes of
// xrl_tfidf.h own the memory and call these; TfidfHandle's device copy holds the same bytes in HBM behind the same views.
//
// Reading document bytes: the host takes one unaligned 8-byte load where 8 bytes are readable (p + 8 <= last) and copies n bytes
// otherwise; device code is built from byte loads only and never reads at or past `last`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XRL_HD __host__ __device__ inline
#else
#define XRL_HD inline
#endif

namespace xrl {
namespace tft {

struct ShortEntry { uint64_t key; uint32_t len; int32_t idx; };                    // tokens of 1..8 bytes: the bytes themselves, zero-extended; len 0 = empty slot
struct LongEntry { uint64_t hash; uint32_t off, len; int32_t idx; uint32_t pad; };   // longer tokens: hash, bytes in the token arena
struct PackedEntry { uint64_t key; uint32_t id1; uint32_t pad; };                  // id1 = feature id + 1; 0 = empty slot
struct GenEntry { uint64_t hash; uint32_t off, n, id1, pad; };

constexpr uint32_t kNone = 0;
constexpr uint32_t kCountCap = 1u << 24;             // a count is the reference's float incremented once per occurrence: += 1.0f stops moving here

// token bytes -> token index
struct TokenView {
    const ShortEntry* s = nullptr; const LongEntry* l = nullptr; const char* arena = nullptr;
    uint64_t s_mask = 0, l_mask = 0;                 // table size - 1 (l == nullptr: no long token)
    unsigned s_shift = 63, l_shift = 63;
};

// n-gram of token indices -> feature id + 1
struct NgramView {
    const uint32_t* uni = nullptr; uint64_t uni_size = 0;
    const PackedEntry* packed = nullptr; const GenEntry* gen = nullptr; const int32_t* arena = nullptr;
    uint64_t p_mask = 0, g_mask = 0;
    unsigned p_shift = 63, g_shift = 63;
    int32_t max_tok = -1;
    unsigned pack_bits = 1;
    int pack_max_n = 0;
    uint64_t packed_n_mask = 0, gen_n_mask = 0;
    bool negative_keys = false;
    int max_n = 0;
};

XRL_HD uint64_t mix(uint64_t x) { x *= 0x9E3779B97F4A7C15ull; return x ^ (x >> 29); }
XRL_HD uint64_t n_bit(int n) { return 1ull << (n < 63 ? n : 63); }

// n (0..8) bytes at p as a little-endian word, zero-extended
XRL_HD uint64_t load_le(const char* p, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t v = 0;
    for (size_t i = 0; i < n; ++i) v |= (uint64_t)(uint8_t)p[i] << (8 * i);
    return v;
#else
    uint64_t v = 0;
    std::memcpy(&v, p, n);
    return v;
#endif
}

// the first n (1..8) bytes at p, zero-extended; the host takes one unaligned load when 8 bytes are readable
XRL_HD uint64_t load_key(const char* p, size_t n, const char* last) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (p + 8 <= last) {
        uint64_t v;
        std::memcpy(&v, p, 8);
        return n == 8 ? v : v & ((1ull << (8 * n)) - 1);
    }
#endif
    (void)last;
    return load_le(p, n);
}

XRL_HD uint64_t hash_long(const char* p, size_t n) {
    uint64_t h = 0x2545F4914F6CDD1Dull ^ (uint64_t)n;
    while (n >= 8) { h = mix(h ^ load_le(p, 8)) + 0x9E3779B97F4A7C15ull; p += 8; n -= 8; }
    if (n) h = mix(h ^ load_le(p, n)) + 0x9E3779B97F4A7C15ull;
    return h * 0xD6E8FEB86659FD93ull;
}

XRL_HD bool same_bytes(const char* a, const char* b, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (size_t i = 0; i < n; ++i) if (a[i] != b[i]) return false;
    return true;
#else
    return std::memcmp(a, b, n) == 0;
#endif
}
XRL_HD bool same_tokens(const int32_t* a, const int32_t* b, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int i = 0; i < n; ++i) if (a[i] != b[i]) return false;
    return true;
#else
    return std::memcmp(a, b, (size_t)n * 4) == 0;
#endif
}

XRL_HD size_t short_slot(unsigned s_shift, uint64_t key, uint32_t len) {
    return (size_t)(mix(key ^ ((uint64_t)len << 56) ^ 0x5bd1e995u) * 0xD6E8FEB86659FD93ull >> s_shift);
}
XRL_HD int32_t find_short(const TokenView& V, uint64_t key, uint32_t len, size_t slot) {
    for (;; slot = (slot + 1) & V.s_mask) {
        const ShortEntry& e = V.s[slot];
        if (e.len == 0) return -1;
        if (e.key == key && e.len == len) return e.idx;
    }
}
XRL_HD int32_t find_long(const TokenView& V, const char* p, size_t n, uint64_t h) {
    if (!V.l) return -1;
    for (size_t slot = (size_t)(h >> V.l_shift);; slot = (slot + 1) & V.l_mask) {
        const LongEntry& e = V.l[slot];
        if (e.len == 0) return -1;
        if (e.hash == h && e.len == n && same_bytes(V.arena + e.off, p, n)) return e.idx;
    }
}

XRL_HD uint64_t pack(unsigned pack_bits, const int32_t* t, int n) {
    uint64_t k = 0;
    for (int i = 0; i < n; ++i) k |= (uint64_t)((uint32_t)t[i] + 1u) << (pack_bits * (unsigned)i);
    return k;
}
XRL_HD size_t packed_slot(unsigned p_shift, uint64_t key) { return (size_t)(mix(key) * 0xD6E8FEB86659FD93ull >> p_shift); }
XRL_HD uint32_t find_packed(const NgramView& V, uint64_t key, size_t slot) {
    for (;; slot = (slot + 1) & V.p_mask) {
        const PackedEntry& e = V.packed[slot];
        if (e.id1 == kNone) return kNone;
        if (e.key == key) return e.id1;
    }
}
XRL_HD uint64_t gen_hash(const int32_t* t, int n) {
    uint64_t h = 0x2545F4914F6CDD1Dull ^ (uint64_t)n;
    for (int i = 0; i < n; ++i) h = mix(h ^ (uint32_t)t[i]) + 0x9E3779B97F4A7C15ull;
    return h * 0xD6E8FEB86659FD93ull;
}
XRL_HD size_t gen_slot(unsigned g_shift, uint64_t h) { return (size_t)(h >> g_shift); }
XRL_HD uint32_t find_gen(const NgramView& V, const int32_t* t, int n, uint64_t h) {
    if (!V.gen) return kNone;
    for (size_t slot = gen_slot(V.g_shift, h);; slot = (slot + 1) & V.g_mask) {
        const GenEntry& e = V.gen[slot];
        if (e.id1 == kNone) return kNone;
        if (e.hash == h && e.n == (uint32_t)n && same_tokens(V.arena + e.off, t, n)) return e.id1;
    }
}

// ---- what is known of a document before it is read: the bounds both tokenizers size their arrays with
// tokens kept of a document of len bytes: a word document has at most (len + 1) / 2 tokens, a character one len; max_length > 0 cuts
XRL_HD uint64_t token_bound(int tok_type, int max_length, uint64_t len) {
    const uint64_t by_len = tok_type == 10 ? (len + 1) / 2 : len;
    return max_length > 0 && (uint64_t)max_length < by_len ? (uint64_t)max_length : by_len;
}
// the largest n looked up in a document of T tokens
XRL_HD int ngram_hi(int max_ngram, int max_n, uint64_t T) {
    const int m = max_ngram < max_n ? max_ngram : max_n;
    return (uint64_t)m < T ? m : (int)T;
}
// n-gram positions of a document of T tokens: sum over n in [n_lo, n_hi] of T - n + 1 (the most feature occurrences it can hold)
XRL_HD uint64_t occurrence_bound(uint64_t T, int n_lo, int n_hi) {
    if (n_hi < n_lo) return 0;
    const uint64_t k = (uint64_t)(n_hi - n_lo + 1);
    return k * (T + 1) - ((uint64_t)n_lo + (uint64_t)n_hi) * k / 2;
}

}  // namespace tft
}  // namespace xrl
