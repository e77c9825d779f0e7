// klt_sched.cpp — the trackers' two state machines (klt_sched.h) as pure functions of (state, values).
#include "klt_sched.h"

namespace ftk {

bool klt_sched_applies(const KltSchedInput &in) {
    // From kSchedMinFeatures on — or, when this variant's recent calls had a long feature (long_tail: the kernels report it,
    // klt_tail_class_step), already from kSchedMinLongTail: multi-wave features of a few thousand do NOT all fit the chip at once, and
    // a 50-iteration feature that starts in the second round ends the launch that much later (the reference's example pair, same
    // box, order from 4 096 / from 1 024: affine inverse 2 000 features 165.9 / 138.8 us, affine direct 3 000: 174.7 / 136.0, LSSD
    // fast 3 000: 143.2 / 113.2, Basic fast 3 000: 60.9 / 52.3; the synthetic scene's LSSD / affine variants -4 ... -15 %).  Calls
    // without a tail keep list order there: the order costs every feature one more dependent load (Basic variants +3 ... 4 %).
    const uint32_t sched_min = in.sched_min != kKltNotSet ? (uint32_t)in.sched_min  // (experiment override)
                                                          : (in.long_tail ? kSchedMinLongTail : kSchedMinFeatures);
    return in.sched != 0 && in.n_track >= sched_min && in.n <= kSchedMaxFeatures;
}

// Launch order.  A call's time is bulk + tail: features run a data-dependent number of Gauss-Newton iterations
// (config 3: mean 6.7, one feature 52), a launch in list order starts the long ones wherever they happen to sit,
// and the grid drains while they finish.  Trackers are called frame after frame on (nearly) the same feature list
// and a feature that needed many iterations tends to need many again, so the launch slots go through a permutation:
// longest first by an EARLIER call's iteration counts.  No launch of its own: call k's tracker launch carries one
// extra workgroup (block 0, klt_order.h klt_order_block) that sorts call k - 1's counts while the features of call k
// run, and call k + 1 uses the result — so from the third call with the same feature count on, with a predictor two
// calls old.  Which slot runs a feature changes nothing in its arithmetic.  Only for calls with more features than
// fit the chip at once; FTK_KLT_SCHED=0 keeps list order.
//
// Call k of a run of calls with one feature count (DESIGN.md 5.8 has the same table):
//   k      writes counts to   sorts (counts -> order)   installs
//   0      iters[0]           -                         Position order into order[0], or none
//   1      iters[1]           iters[0] -> order[0]      Position order into order[1], or none
//   2      iters[0]           iters[1] -> order[1]      order[0]: written by the sort of call 1 from the counts of call 0
//   k      iters[k & 1]       the other pair            order[k & 1]: written by the sort of call k - 1
KltSchedStep klt_sched_step(KltSchedState &s, const KltSchedInput &in) {
    KltSchedStep out = {};
    out.sort_from = -1;
    if (!klt_sched_applies(in)) {
        return out;
    }
    out.active = true;
    if ((size_t)in.n > s.capacity) {
        // position-keyed slot swaps: a claim word per launch slot, and (once) the two tables of iteration counts by position
        out.grow_to = ((size_t)in.n + 4095) / 4096 * 4096;
        s.capacity = out.grow_to;
        s.n = 0;
    }
    if (s.n != in.n) {
        s.n = in.n;
        s.calls = 0;
    }
    const uint32_t k = s.calls++;
    const bool grown = out.grow_to != 0;
    // Position-keyed swaps ride on every such call, whatever the list did since the last one.  Call numbers start at 4 (an
    // all-zero grid / claim word is never "recent") and tag 23 bits of a claim word: the claims are wiped before a tag could
    // repeat.
    // (never inside a stream capture: a replayed launch would carry this call's number again and read its own old claims)
    // EVERY such call (outside a capture) leaves its iteration counts in the position table — one or two atomics per feature —
    // so that the next one can order or trade by position whatever kernel either of them runs.
    out.recording = !in.capturing && (grown || (in.have_grid && in.have_claim));
    uint32_t last_recorded = 0;
    if (out.recording) {
        if (s.call < 4u) {
            s.call = 4u;
        }
        ++s.call;
        if (sched_claim_tag(s.call) < 4u) {
            out.wipe_claims_and_grid = true;
            s.call += 4u;
            s.recorded = 0;
        }
        out.sched_call = s.call;
        last_recorded = s.recorded;
        s.recorded = s.call;
    }
    // (no trades when the results overwrite the reference positions: both sides of a trade must read the same positions)
    // Multi-wave features only: there a feature is tens of microseconds long and iteration counts have heavy tails
    // (config 3: 192 / 207 -> 149 / 166 us with no / a stale launch order, +0.5 % with a fitting one); the one-wave kernels
    // run 10 000 - 25 000 cheap features, every late one of which would pay a table look-up for a 3 % gain at best
    // (config 4: +2.9 % with a fitting order, -3 % without; config 5: +1 %).
    out.trades = out.recording && in.waves_per_feature >= 2 && in.ref_untouched && in.n > kSchedTradeMin;
    out.iters_buf = (int)(k & 1u);
    if (k >= 1) {  // sort the previous call's counts beside this call's features
        out.sort_from = (int)((k - 1) & 1u);
        // The spatial (tile) order reads the reference positions in two passes while the feature workgroups of the same
        // launch write cur_uv_out: with one position buffer updated in place (ref == out, allowed by include/ftk.h) a
        // feature crossing a tile boundary in between would make the histogram and the scatter disagree — duplicates,
        // stale entries, a write past order[n - 1].  Such a call gets the iteration-count / identity order instead.
        out.sort_reads_ref_uv = in.ref_untouched;
    }
    if (k >= 2) {  // made during the previous call from the counts before it
        out.order = KltOrder::Index;
    } else if (out.recording && last_recorded != 0u && last_recorded + 1u == s.call && (grown || in.have_pred) && in.model != FTK_MODEL_BASIC && !out.trades) {
        // (LSSD and affine KLT: their iteration counts have tails — config 4 without history 206 -> 183 us, with luminance
        // 357 -> 315; Basic KLT's are flat on most scenes and the ~10 us of the two launches would buy nothing — config 5 shard
        // 181 -> 190; the multi-wave kernels trade slots by position inside the launch instead)
        // No index-keyed order (the feature count has just changed, or these are the first calls): order THIS call by what the
        // last call left at its features' positions — two small launches in front of the tracker's (klt_kernels.hip
        // klt_position_order_launch).  The buffer is the one an index-keyed order of this call would have used: nobody else
        // writes it during this call.
        out.order = KltOrder::Position;
    }
    out.order_buf = out.order != KltOrder::None ? (int)(k & 1u) : 0;
    return out;
}

void klt_sched_reset(KltSchedState &s) {
    s.calls = 0;
    s.n = 0;
}

// A variant's own word: {call number << 8 | iterations} of the longest feature of its most recent launch that has got that far.
// The host may be many launches ahead of the device (back-to-back calls), so a report counts while it is at most kTailFresh
// launches of the context old, and one long report holds for kTailHold launches of the variant.
int klt_tail_class_step(KltTailState &t, int model, int method, uint32_t seen_word) {
    KltTailState::Variant &v = t.variant[model][klt_method_class(method)];
    const uint32_t age = (t.call - tail_word_call(seen_word)) & kTailCallMask;
    if (seen_word != 0 && age <= kTailFresh && tail_word_iters(seen_word) >= kTailLongFrom) {
        v.long_until = v.launches + kTailHold;
    }
    return v.launches < v.long_until ? 1 : 0;
}

uint32_t klt_tail_next_call(KltTailState &t, int model, int method, bool *wipe_device_word) {
    t.call = (t.call + 1u) & kTailCallMask;
    *wipe_device_word = t.call == 0u;
    if (t.call == 0u) {
        t.call = 1u;  // (after 16 M launches the device word's running maximum starts over with the host's)
    }
    ++t.variant[model][klt_method_class(method)].launches;
    return t.call;
}

}  // namespace ftk
