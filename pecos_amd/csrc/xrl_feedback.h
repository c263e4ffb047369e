// Pruning feedback: what the bound pruning of the PREVIOUS predicts of a handle achieved, per layer, so that a model on which the first
// stage settles almost nothing (scores that do not saturate, routing spread over the tree) stops paying for the staging -- the layer then
// scores every candidate in one pass (tile format: on tile-sorted items).  Results never depend on it.
#pragma once
#include "xrl_common.h"

namespace xrl {

constexpr int kFbLayers = 16;               // layers 0 .. kFbLayers-1 of a model take part
// Word layout of the pinned, device-visible array PruneFeedback::host (the kernels that write it: xrl_k1q_impl.h, xrl_k1.hip, xrl_k1t.hip):
//   [0, kFbCounterWords)             K1Q's sampled counters {queries seen, queries that needed the second pass} per layer, a copy of
//                                    PruneFeedback::dev made by the first wavefront of the next K1Q launch
//   [kFbCounterWords, kFbHostWords)  the last stage's item count of tile-format layers (written by its K1 launch)
constexpr int kFbCounterWords = 2 * kFbLayers, kFbHostWords = 3 * kFbLayers;
constexpr int fb_seen_word(int layer) { return 2 * layer; }
constexpr int fb_second_word(int layer) { return 2 * layer + 1; }
constexpr int fb_items_word(int layer) { return kFbCounterWords + layer; }
constexpr uint32_t kFbPending = 0xFFFFFFFFu;   // items word: no bound-pruned launch has reported since the word was armed

struct PruneFeedback {
    // kReprobe: an unstaged layer is staged again every so many predicts (the data may have changed).  K1Q: a decision needs kMinSamples sampled
    // queries; unstaged when more than kSecondShare of them needed the second pass.  Tile format: unstaged when the last stage held more
    // than kItemShare of the slots it was sized for.
    static constexpr uint32_t kReprobe = 32, kMinSamples = 256;
    static constexpr double kSecondShare = 0.7, kItemShare = 0.6;

    uint32_t* host = nullptr; DevBuf dev;           // pinned words (layout above); K1Q's counters (device atomics)
    uint32_t seen[kFbLayers] = {0}, second[kFbLayers] = {0};   // K1Q counters at the last decision
    uint64_t tile_slots[kFbLayers] = {0};                      // last-stage slots the item count of a tile-format layer refers to
    uint32_t unstaged_calls[kFbLayers] = {0};                  // predicts in a row a layer has run unstaged (re-probed every kReprobe)
    uint8_t unstaged[kFbLayers] = {0}, probing[kFbLayers] = {0};   // probing: an unstaged layer was staged ONCE (the probe) and its outcome has not arrived yet: it keeps running unstaged meanwhile

    ~PruneFeedback() { if (host) (void)hipHostFree(host); }
    uint32_t word(int w) const { return static_cast<volatile const uint32_t*>(host)[w]; }   // the device writes these while the host enqueues

    // Start of a predict of n_layers layers (xrl_predict.cpp): allocates the words on first use, folds what has arrived into the per-layer
    // state (`sample` false -- the stats pass -- leaves the state alone) and says how each layer runs THIS time.
    struct Plan { bool unstaged[kFbLayers] = {false}, probed[kFbLayers] = {false}; };
    Plan begin_predict(size_t n_layers, bool sample);
    // What the handle's warm-up predicts taught is discarded: every layer staged again, counters re-based, item words armed.
    void reset() {
        if (!host) return;
        for (int l = 0; l < kFbLayers; ++l) {
            unstaged[l] = 0; probing[l] = 0; unstaged_calls[l] = 0; tile_slots[l] = 0;
            seen[l] = host[fb_seen_word(l)]; second[l] = host[fb_second_word(l)]; host[fb_items_word(l)] = kFbPending;
        }
    }
    // Option "adaptive" was set: every layer staged again; counters, item words and the re-probe clock stay as they are.
    void restage() { for (auto& u : unstaged) u = 0; for (auto& u : probing) u = 0; }
};

}  // namespace xrl
