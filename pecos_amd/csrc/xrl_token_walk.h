// The token walk of the TF-IDF kernels, stated once for K9 (xrl_tokenize.hip: lookups against a loaded vocabulary) and K15
// (xrl_tfidf_train.hip: the vocabulary and document-frequency passes of training).
//
// One wavefront walks one document, lanes on consecutive bytes, 64 per step:
//   word mode    ballot of ' '; a token starts at a non-space byte after a space or the document start (one carry bit between steps); its
//                ordinal is the running count + the starts below the lane; the lane that owns a start finds the end (from the mask, or
//                past the step by walking bytes)
//   char modes   a token starts at every byte that is not 10xxxxxx and takes the size its lead byte names, cut at the buffer end; the same
//                lane checks that the bytes it covers are continuation bytes and that the next one is not: the lowest position that fails
//                gives the document's status (1: the host's next character starts on a continuation byte -- the host tokenizer fails;
//                2: a lead byte followed by too few continuation bytes -- the host's sequential decode takes another path)
// The walk stops once `tb` tokens were seen (the max_length cut; positions past it are not checked, nor does the host check them).
// on_token(ord, pos, n) runs on the lane that owns token `ord` (< tb): n bytes from doc + pos.  No byte at or past doc + len is read.
#pragma once
#include "xrl_device.h"

namespace xrl {
namespace tokw {

__device__ __forceinline__ bool is_cont(uint8_t c) { return (c & 0xC0u) == 0x80u; }

// returns the tokens seen (>= tb when the cut stopped the walk); status: 0, or the char-mode status of the lowest failing position
template <class F>
__device__ __forceinline__ uint64_t walk_tokens(const char* doc, uint64_t len, int tok_type, uint64_t tb, uint32_t lane, uint32_t& status, F&& on_token) {
    uint64_t count = 0;
    status = 0;
    if (tok_type == 10) {
        unsigned long long carry = 1ull;
        for (uint64_t p0 = 0; p0 < len && count < tb; p0 += 64u) {
            const uint64_t pos = p0 + lane;
            const char c = pos < len ? doc[pos] : ' ';
            const unsigned long long sp = __ballot(c == ' ');
            const unsigned long long starts = ~sp & ((sp << 1) | carry);
            carry = sp >> 63;
            if ((starts >> lane) & 1ull) {
                const uint64_t ord = count + lanes_below(starts);
                if (ord < tb) {
                    const unsigned long long m = sp >> lane;
                    uint64_t end;
                    if (m) end = pos + (uint64_t)__builtin_ctzll(m);
                    else { end = p0 + 64u; while (end < len && doc[end] != ' ') ++end; }
                    on_token(ord, pos, end - pos);
                }
            }
            count += (uint64_t)__popcll(starts);
        }
    } else {
        for (uint64_t p0 = 0; p0 < len && count < tb; p0 += 64u) {
            const uint64_t pos = p0 + lane;
            const bool valid = pos < len;
            const uint8_t c = valid ? (uint8_t)doc[pos] : (uint8_t)0x80;
            const bool start = valid && !is_cont(c);
            const unsigned long long starts = __ballot(start);
            uint32_t viol = 0;
            if (start) {
                const uint64_t ord = count + lanes_below(starts);
                if (ord < tb) {                            // (positions past the max_length cut are not checked; nor does the host)
                    const uint64_t cs = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
                    const uint64_t n = cs < len - pos ? cs : len - pos;
                    bool inner = true;
                    for (uint64_t i = 1; i < n; ++i) inner &= is_cont((uint8_t)doc[pos + i]);
                    if (pos + cs < len && is_cont((uint8_t)doc[pos + cs])) viol = 1;      // the host's next character starts on a continuation byte
                    else if (!inner) viol = 2;                                          // the host skips a byte that starts a character here
                    on_token(ord, pos, n);
                }
            } else if (pos == 0 && valid) viol = 1;
            const unsigned long long vm = __ballot(viol != 0);
            if (vm && !status) status = (uint32_t)__shfl((int)viol, __builtin_ctzll(vm), 64);
            count += (uint64_t)__popcll(starts);
        }
    }
    return count;
}

}  // namespace tokw
}  // namespace xrl
