// klt_sched.h — what the host and the kernels of the trackers share about launch order and tail class: the geometry of the position
// tables, the formats of the four words both sides read and write, and the two state machines of a context (which launch order a
// call gets, which tail class a variant is in) as pure step functions (klt_sched.cpp: no context, no environment, no HIP call;
// tests/test_klt_sched_cpu.py walks them without a device through host/build/klt_sched_cli).  Plain C++: klt_order.h includes
// this for the device side, ftk_klt.cpp for the host side.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/ftk.h"

namespace ftk {

constexpr int kKltNotSet = -1;  // an FTK_KLT_* override that is not in the environment

// inverse 0, direct 1, fast-like (fast / sse / neon) 2: the method axis of the wave policy table and of the tail words
constexpr int klt_method_class(int method) { return method == FTK_METHOD_INVERSE ? 0 : (method == FTK_METHOD_DIRECT ? 1 : 2); }

// The helpers are inlined before anything is optimised, like the kernels' own __forceinline__ helpers.
#define FTK_WORD_FN constexpr __attribute__((always_inline))

// ---- position tables and launch slots (klt_order.h "Position-keyed slot swaps") ----
constexpr int kSchedTableBits = 16;
constexpr int kSchedTableSize = 1 << kSchedTableBits;  // entries per table; two tables (written by this call / read from the last)
constexpr int kSchedHeadFirst = 256;   // the heads are the slots [kSchedHeadFirst, kSchedHeadFirst + kSchedHeadSlots): resident from the
constexpr int kSchedHeadSlots = 256;   // first microsecond, but NOT the very first ones — with a fitting launch order those hold the
constexpr int kSchedLateSlot = 1024;   // longest features, which must not start a scan's 2 - 3 us later
constexpr uint32_t kSchedLongCount = 12;   // a late slot is a candidate from this predicted count on ...
constexpr uint32_t kSchedSwapMargin = 8;   // ... and a head trades with it if that is this much above its own feature's prediction
constexpr uint32_t kSchedSelf = 0x1FFu;    // claim code "the slot runs its own feature"; 0 .. kSchedHeadSlots - 1: the head (by number) it trades with
constexpr uint32_t kTailReportFrom = 12;   // a feature reports its iteration count from here on (klt_order.h tail_report)
// trades need more features than this: a late slot beyond the heads' own
constexpr int32_t kSchedTradeMin = kSchedLateSlot + kSchedHeadFirst + kSchedHeadSlots;

// The grid buffer of a context, in words: the two tables, the two "no tail" flags, then the histogram + cursors of the
// position-keyed launch order (klt_position_order_launch).
constexpr size_t kSchedFlagsAt = (size_t)2 << kSchedTableBits;
constexpr size_t kSchedTableWords = kSchedFlagsAt + 2;
constexpr size_t kSchedOrderWords = 512;
constexpr size_t kSchedGridWords = kSchedTableWords + kSchedOrderWords;
FTK_WORD_FN uint32_t sched_table_at(uint32_t call) { return (call & 1u) << kSchedTableBits; }  // the table call `call` writes

// ---- the words ----
// grid word {call:24 | iters:8}: what call `call` left at a position
constexpr uint32_t kSchedGridCallMask = 0xFFFFFFu;
FTK_WORD_FN uint32_t sched_grid_tag(uint32_t call) { return call & kSchedGridCallMask; }
FTK_WORD_FN uint32_t sched_grid_pack(uint32_t call, uint32_t iters) { return (sched_grid_tag(call) << 8) | (iters < 255u ? iters : 255u); }
FTK_WORD_FN uint32_t sched_grid_call(uint32_t word) { return word >> 8; }
FTK_WORD_FN uint32_t sched_grid_iters(uint32_t word) { return word & 0xFFu; }
// claim word {call:23 | code:9}: who runs the feature of a late slot in call `call` (kSchedSelf, or a head by number)
constexpr uint32_t kSchedClaimCallMask = 0x7FFFFFu, kSchedClaimCodeMask = 0x1FFu;
FTK_WORD_FN uint32_t sched_claim_tag(uint32_t call) { return call & kSchedClaimCallMask; }
FTK_WORD_FN uint32_t sched_claim_pack(uint32_t call, uint32_t code) { return (sched_claim_tag(call) << 9) | code; }
FTK_WORD_FN uint32_t sched_claim_call(uint32_t word) { return word >> 9; }
FTK_WORD_FN uint32_t sched_claim_code(uint32_t word) { return word & kSchedClaimCodeMask; }
// flag word {call:31 | flat:1}: "the counts call `call` sorted had no tail"
FTK_WORD_FN uint32_t sched_flag_pack(uint32_t call, uint32_t flat) { return ((call & 0x7FFFFFFFu) << 1) | flat; }
FTK_WORD_FN uint32_t sched_flag_call(uint32_t word) { return word >> 1; }
FTK_WORD_FN uint32_t sched_flag_flat(uint32_t word) { return word & 1u; }
// tail word {call:24 | iters:8}: the longest feature of a variant's launch number `call` of the context
constexpr uint32_t kTailCallMask = 0xFFFFFFu;
FTK_WORD_FN uint32_t tail_word_pack(uint32_t call, uint32_t iters) { return (call << 8) | (iters < 255u ? iters : 255u); }
FTK_WORD_FN uint32_t tail_word_call(uint32_t word) { return word >> 8; }
FTK_WORD_FN uint32_t tail_word_iters(uint32_t word) { return word & 0xFFu; }

static_assert(kSchedSelf <= kSchedClaimCodeMask && (uint32_t)kSchedHeadSlots - 1u < kSchedSelf, "the claim code holds every head number and kSchedSelf");
static_assert(kSchedFlagsAt == 2 * (size_t)kSchedTableSize && kSchedFlagsAt + 2 <= kSchedGridWords, "two tables and two flags in front of the order workspace");
static_assert(kSchedTableWords == (2u << 16) + 2 && kSchedTradeMin == 1024 + 512, "the figures the kernels were measured with");
static_assert((kSchedClaimCallMask << 9 | kSchedClaimCodeMask) == 0xFFFFFFFFu && (kSchedGridCallMask << 8 | 0xFFu) == 0xFFFFFFFFu, "the fields fill their words");

// ---- launch order: which order a call gets, what it records, what it sorts for the next one ----
constexpr uint32_t kSchedMinFeatures = 4096;    // below this (nearly) every feature is resident from the start: nothing to order ...
constexpr uint32_t kSchedMinLongTail = 1024;    // ... unless the variant's calls have a long tail (klt_sched_step)
constexpr int32_t kSchedMaxFeatures = 1 << 18;  // the sort block walks the list alone; beyond this it could outlast the launch

// The counters of a context (ftk_context::sched).
struct KltSchedState {
    uint32_t recorded = 0;  // `call` of the last call that left its counts in the position table (0: none yet)
    uint32_t call = 0;      // calls that used the grid so far (tags its entries and the claims)
    size_t capacity = 0;    // features each buffer holds
    int32_t n = 0;          // feature count of the calls counted in `calls`
    uint32_t calls = 0;     // consecutive calls with that feature count so far
};

// Everything the decision depends on, as values.
struct KltSchedInput {
    int32_t n;
    uint32_t n_track;
    int model, waves_per_feature, long_tail;
    bool capturing;      // the stream is being captured into a graph
    bool ref_untouched;  // the results do not overwrite the reference positions
    int sched, sched_min;  // FTK_KLT_SCHED / FTK_KLT_SCHED_MIN, parsed, or kKltNotSet
    bool have_grid, have_claim, have_pred;  // the context holds these buffers already (after a growth it holds all of them)
};

enum class KltOrder { None, Index, Position };

// What the caller must do and install, as values.  Buffer numbers index the context's double-buffered iteration counts and orders.
struct KltSchedStep {
    bool active;                // klt_sched_applies; false: list order, nothing recorded, the state untouched
    size_t grow_to;             // != 0: (re)allocate every buffer for this many features first
    bool wipe_claims_and_grid;  // zero the claim words and the tables + flags first: a 23-bit tag is about to repeat
    int iters_buf;              // this call's counts go here
    int sort_from;              // -1, or: the sort block orders the counts of this buffer into the order buffer of the same number ...
    bool sort_reads_ref_uv;     // ... and may use the spatial (tile) order
    KltOrder order;             // Index: order_buf as an earlier launch's sort block left it; Position: made into order_buf in front of
    int order_buf;              // the launch, from the table call sched_call - 1 wrote
    bool recording;             // the call leaves its counts in the position table under sched_call
    uint32_t sched_call;
    bool trades;                // slot trades by position are on
};

// Does the call get a launch order at all?  From n, n_track, long_tail and the two switches alone: a caller asks this before it
// reads the rest of the input from the world (klt_sched_step asks it again).
bool klt_sched_applies(const KltSchedInput &in);
KltSchedStep klt_sched_step(KltSchedState &s, const KltSchedInput &in);
// The history starts over: the next call is the first of its ladder (a call that ran without the order, or did not run at all).
void klt_sched_reset(KltSchedState &s);

// ---- tail class: is a variant's next launch looked up in the long-tail half of the wave policy? ----
constexpr uint32_t kTailLongFrom = 24;  // iterations of a call's longest feature from which the call counts as tail-bound
constexpr uint32_t kTailHold = 8;       // launches of the variant for which one such report holds
constexpr uint32_t kTailFresh = 256;    // launches of the context a report may lag behind (the host enqueues far ahead of the device)

struct KltTailState {
    uint32_t call = 0;  // tracker launches of this context so far (tags the reports)
    struct Variant {
        uint32_t launches = 0;    // launches of this variant so far
        uint32_t long_until = 0;  // "this variant's calls have a long tail" while launches < long_until
    } variant[3][3];              // [model][klt_method_class]
};

// Tail class of the variant's next launch given its tail word as the host sees it now (0: nothing reported yet).
int klt_tail_class_step(KltTailState &t, int model, int method, uint32_t seen_word);
// The number of the variant's next launch; *wipe_device_word: the counter wrapped, the device words' running maxima start over.
uint32_t klt_tail_next_call(KltTailState &t, int model, int method, bool *wipe_device_word);

}  // namespace ftk
