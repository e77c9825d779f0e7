// klt_order.h — the device side of klt_sched.h: iteration counts remembered by position, the trade of launch slots between
// early and late workgroups, the tail report for the next call's wave policy, and the extra workgroup that sorts the next
// launch order (klt_order_block).  Used by the three tracker translation units.
#pragma once

#include "klt_scalar.h"
#include "klt_sched.h"

#include <math.h>

namespace ftk {

// ---------------------------------------------------------------------------------------------
// Position-keyed slot swaps.  The launch order (klt_order_block, below) is a permutation of LIST INDICES made during an earlier call: a caller whose
// feature list changes between frames (features re-detected, reshuffled) gets an arbitrary order, and a feature that needs dozens
// of iterations starts wherever it happens to sit — the launch then ends that much later (config 3: 146 us with a fitting order,
// 208 with a stale one).  Iteration counts are therefore ALSO remembered by POSITION: every tracked feature leaves
// (call number, count) in a hash table keyed by its level-0 position (atomicMax: the newest call wins, then the largest count;
// one table is written by this call while the other, last call's, is only read).  At the start of a launch the first kSchedHeadSlots slots — resident from the first microsecond — each look through
// their share of the LATE slots (>= kSchedLateSlot: the ones that may have to wait for a free CU), pick the one whose position
// predicts the most iterations, and, if that is kSchedSwapMargin more than their own feature's prediction, trade places with
// it: the head runs the long feature now, the late slot runs the head's feature when its turn comes.  A claim word per late
// slot, taken with a compare-and-swap by whichever of the two gets there first, guarantees that every feature is processed
// exactly once whatever the timing; nobody waits for anybody.  Which slot runs a feature changes nothing in its arithmetic.
// ---------------------------------------------------------------------------------------------
// (the slot classes, the table geometry and the formats of the words: klt_sched.h, shared with the host)

// positions are remembered at 4-pixel resolution (a feature that crosses such a boundary between two frames is simply not predicted)
__device__ __forceinline__ uint32_t sched_table_slot(float u, float v) {
    const uint32_t qx = (uint32_t)(int)fminf(fmaxf(u * 0.25f, 0.0f), 1048575.0f), qy = (uint32_t)(int)fminf(fmaxf(v * 0.25f, 0.0f), 1048575.0f);  // NaN -> 0
    return ((qx * 73856093u) ^ (qy * 19349663u)) & (uint32_t)(kSchedTableSize - 1);
}

// What the LAST call left at this position (the table this call only reads: every wave of a launch sees the same predictions)
__device__ __forceinline__ uint32_t sched_prediction(const KltParams &p, float u, float v) {
    // (sched_table_at(p.sched_call - 1u), spelled out: through the helper the compiler forms this address with other instructions)
    const uint32_t word = p.sched_grid[(((p.sched_call - 1u) & 1u) << kSchedTableBits) + sched_table_slot(u, v)];
    return sched_grid_call(word) == sched_grid_tag(p.sched_call - 1u) ? sched_grid_iters(word) : 0u;
}

// ... at the feature's reference position (a caller that tracks the same list again asks there) AND at the position it was tracked to
// (a caller that tracks frame after frame asks there: the next call's reference positions are this call's results)
__device__ __forceinline__ void sched_grid_record(const KltParams &p, float ref_u, float ref_v, float out_u, float out_v, uint32_t iters) {
    if (p.sched_grid != nullptr) {
        const uint32_t word = sched_grid_pack(p.sched_call, iters);
        uint32_t *table = p.sched_grid + sched_table_at(p.sched_call);
        const uint32_t at_ref = sched_table_slot(ref_u, ref_v), at_out = sched_table_slot(out_u, out_v);
        atomicMax(&table[at_ref], word);
        if (at_out != at_ref) {
            atomicMax(&table[at_out], word);
        }
    }
}

// The iteration count of a call's longest feature, for the NEXT call's wave policy (ftk_klt.cpp klt_tail_class): features that ran at
// least kTailReportFrom iterations raise a device word with atomicMax — an L2 load for most, an atomic for the few that raise it —
// and whoever raised it forwards the new value to a device-visible host word with one system-scope store.  A lower value may land
// after a higher one (two raisers racing over PCIe): the host treats the word as a hint.  One lane per feature calls this.
__device__ __forceinline__ void tail_report(const KltParams &p, uint32_t iters, uint32_t id) {
    if (p.tail_dev != nullptr && (iters >= kTailReportFrom || id == 0u)) {  // (feature 0 always: every launch refreshes the variant's word)
        const uint32_t word = tail_word_pack(p.tail_call, iters);
        if (word > __hip_atomic_load(p.tail_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            if (atomicMax(p.tail_dev, word) < word) {
                __hip_atomic_store(p.tail_host, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Called by ONE wave on behalf of a launch slot (every lane with the same arguments): the list slot whose feature this launch
// slot runs — `slot` itself, or the slot it traded places with.  `swapped_in` tells a head that it now runs a predicted-long feature.
__device__ __forceinline__ uint32_t sched_resolve_slot(const KltParams &p, uint32_t slot, bool &swapped_in) {
    swapped_in = false;
    const uint32_t n = (uint32_t)p.n, call = sched_claim_tag(p.sched_call);
    const int lane = (int)(threadIdx.x & 63);
    // The sort block of the LAST launch found no tail in the counts it sorted: nobody trades, and nobody pays for looking (one
    // word, the same for every slot of this launch: this launch's own sort block writes the other one).
    if (p.sched_flags[(p.sched_call - 1u) & 1u] == sched_flag_pack(p.sched_call - 1u, 1u)) {
        return slot;
    }
    if (slot >= (uint32_t)kSchedLateSlot) {
        // A late slot.  Heads only ever claim slots whose prediction reaches kSchedLongCount, and predictions come from a table
        // nobody writes during this launch: a slot below that knows, without asking, that it runs its own feature.
        const uint32_t f = p.order ? (uint32_t)p.order[slot] : slot;
        if (sched_prediction(p, p.ref_uv[2 * f], p.ref_uv[2 * f + 1]) < kSchedLongCount) {
            return slot;
        }
        uint32_t word = 0;
        if (lane == 0) {
            uint32_t seen = __hip_atomic_load(&p.sched_claim[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sched_claim_call(seen) != call) {
                const uint32_t mine = sched_claim_pack(call, kSchedSelf);
                const uint32_t prev = atomicCAS(&p.sched_claim[slot], seen, mine);
                seen = prev == seen ? mine : prev;  // lost the race: only a head of THIS call writes here
            }
            word = seen;
        }
        word = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
        const uint32_t code = sched_claim_code(word);
        return (sched_claim_call(word) == call && code != kSchedSelf) ? (uint32_t)kSchedHeadFirst + code : slot;
    }
    if (slot < (uint32_t)kSchedHeadFirst || slot >= (uint32_t)(kSchedHeadFirst + kSchedHeadSlots) || n <= (uint32_t)kSchedLateSlot) {
        return slot;
    }
    // a head: my share of the late slots, one per lane and pass
    const uint32_t head = slot - (uint32_t)kSchedHeadFirst;
    const uint32_t late = n - (uint32_t)kSchedLateSlot, share = (late + kSchedHeadSlots - 1) / kSchedHeadSlots;
    const uint32_t first = (uint32_t)kSchedLateSlot + head * share, last = min(first + share, n);
    const uint32_t own_feature = p.order ? (uint32_t)p.order[slot] : slot;
    const uint32_t own = sched_prediction(p, p.ref_uv[2 * own_feature], p.ref_uv[2 * own_feature + 1]);
    uint32_t best = 0;  // (prediction << 20) | slot: the most iterations, then the highest slot
    for (uint32_t s = first + (uint32_t)lane; s < last; s += 64u) {
        const uint32_t f = p.order ? (uint32_t)p.order[s] : s;
        best = max(best, (sched_prediction(p, p.ref_uv[2 * f], p.ref_uv[2 * f + 1]) << 20) | s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        best = max(best, (uint32_t)__shfl_xor((int)best, off));
    }
    const uint32_t pred = best >> 20, target = best & 0xFFFFFu;
    if (pred < kSchedLongCount || pred < own + kSchedSwapMargin || target < first) {
        return slot;
    }
    uint32_t won = 0;
    if (lane == 0) {
        const uint32_t seen = __hip_atomic_load(&p.sched_claim[target], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sched_claim_call(seen) != call) {
            won = atomicCAS(&p.sched_claim[target], seen, sched_claim_pack(call, head)) == seen ? 1u : 0u;
        }
    }
    won = (uint32_t)__builtin_amdgcn_readfirstlane((int)won);
    swapped_in = won != 0u;
    return won != 0u ? target : slot;
}

// ---------------------------------------------------------------------------------------------
// Launch order of a later call, computed by ONE extra workgroup of the tracker launch itself (block 0: it starts first and
// runs beside the feature workgroups, so the sort costs no launch and no time of its own): the feature indices sorted by the
// iteration counts of the PREVIOUS call, longest first — a counting sort over min(count, 255) with the workgroup's dynamic LDS
// as its bins.  When the counts have no tail (largest <= 1.5 x the mean of the tracked features) the same counting sort runs over
// image tiles instead (klt_order_block).  Any permutation yields the same tracking results; only the schedule differs.
// ---------------------------------------------------------------------------------------------

// Counting only (nothing returns, so nothing waits): ONE LDS atomic for all the lanes that share the lowest active lane's bin, one
// each for the rest.
__device__ __forceinline__ void wave_bin_count(int *bins, int bin, bool active) {
    const unsigned long long todo = wave_ballot(active);
    if (todo == 0ull) {
        return;
    }
    const int leader = __builtin_ctzll(todo);
    const int leader_bin = __builtin_amdgcn_readlane(bin, leader);
    const bool with_leader = active && bin == leader_bin;
    const unsigned long long same = wave_ballot(with_leader);
    if ((int)(threadIdx.x & 63) == leader) {
        (void)__hip_atomic_fetch_add(&bins[leader_bin], __popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (active && !with_leader) {
        (void)__hip_atomic_fetch_add(&bins[bin], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// A slot in its bin for every active lane, for U independent elements per lane.  Per element one round of "the lowest active
// lane's bin: ONE LDS atomic for all the lanes that share it" — iteration counts cluster, and a call whose features all took 5
// iterations would otherwise serialise thousands of atomics on one address — then one atomic per remaining lane (counts spread
// over many bins: little contention).  The U leader atomics are issued back to back, then the U atomics of the remaining lanes:
// two waits instead of 2 U.  Slots are unique (LDS atomics of a wave execute in order; other waves interleave atomically); which
// of two equal-bin features gets the earlier slot is not defined.
template <int U>
__device__ __forceinline__ void wave_bin_claim_batch(int *bins, const int (&bin)[U], const bool (&active)[U], int (&slot)[U]) {
    const int lane = (int)(threadIdx.x & 63);
    const unsigned long long below = (1ull << lane) - 1ull;
    int leader[U], leader_bin[U], base[U];
    unsigned long long same[U];
    bool with_leader[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long todo = wave_ballot(active[u]);
        leader[u] = todo != 0ull ? __builtin_ctzll(todo) : 0;
        leader_bin[u] = __builtin_amdgcn_readlane(bin[u], leader[u]);
        with_leader[u] = active[u] && bin[u] == leader_bin[u];
        same[u] = wave_ballot(with_leader[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        base[u] = 0;
        if (same[u] != 0ull && lane == leader[u]) {
            base[u] = atomicAdd(&bins[leader_bin[u]], __popcll(same[u]));
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        base[u] = __builtin_amdgcn_readlane(base[u], leader[u]);
        slot[u] = with_leader[u] ? base[u] + __popcll(same[u] & below) : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (active[u] && !with_leader[u]) {
            slot[u] = atomicAdd(&bins[bin[u]], 1);
        }
    }
}

constexpr int kOrderLdsBytes = (4 * 256 + 4) * 4;  // two histograms (iteration counts, image tiles) with their scans + a flag

// Rank in tile order -> launch slot.  Workgroups go to the eight XCDs round robin (workgroup w -> XCD w mod 8, each with its own
// L2), so runs of kOrderRunGroups consecutive workgroup ranks (one small image region) are dealt to ONE XCD, run after run round
// robin: neighbours in the image share an L2 and a moment in time, and every XCD still gets a mix of all regions (whole eighths
// of the image per XCD fetch least — 5.5 MB instead of 32.8 MB per 25 000-feature launch at 1080p — but run 6 % SLOWER than list
// order; runs of 4 / 16 / 32 / 64 / 128 / 256 workgroups: +2.5 / +1.3 / -0.9 / -1.6 / -1.6 / -1.3 % with 21.8 / 15.8 / - / 9.8 MB
// fetched).  Only whole blocks of 8 runs take part; the ranks behind them stay put.
constexpr int kOrderRunGroups = 64;

__device__ __forceinline__ int xcd_major_slot(int rank, int n, int group) {
    const int whole = n / group;  // workgroups with `group` features
    const int dealt = whole / (8 * kOrderRunGroups) * (8 * kOrderRunGroups);
    const int m = rank / group;  // workgroup rank
    if (m >= dealt) {
        return rank;
    }
    const int sub = rank - m * group;
    const int run = m / kOrderRunGroups, in_run = m - run * kOrderRunGroups;
    const int xcd = run & 7, j = (run >> 3) * kOrderRunGroups + in_run;  // the j-th workgroup of that XCD
    return (xcd + 8 * j) * group + sub;
}

// 16 x 16 tiles of the level-0 image, row by row: 256 bins.  (A run of the launch order — kOrderRunGroups workgroups — holds two
// or three tiles' features, so a squarer Morton walk over the tiles would buy nothing, and this key is three instructions.)
__device__ __forceinline__ int image_tile(float u, float v, float inv_tile_u, float inv_tile_v) {
    const int tx = (int)fminf(fmaxf(u * inv_tile_u, 0.0f), 15.0f), ty = (int)fminf(fmaxf(v * inv_tile_v, 0.0f), 15.0f);  // NaN -> 0
    return ty * 16 + tx;
}

// exclusive scan of the 256 bin counts into bin_start by one wave, four bins per lane
__device__ __forceinline__ void order_scan_bins(const int *bin_count, int *bin_start, int l) {
    const int c0 = bin_count[4 * l], c1 = bin_count[4 * l + 1], c2 = bin_count[4 * l + 2], c3 = bin_count[4 * l + 3];
    int run = c0 + c1 + c2 + c3;
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(run, off);
        if (l >= off) {
            run += up;
        }
    }
    const int before = run - (c0 + c1 + c2 + c3);
    bin_start[4 * l] = before;
    bin_start[4 * l + 1] = before + c0;
    bin_start[4 * l + 2] = before + c0 + c1;
    bin_start[4 * l + 3] = before + c0 + c1 + c2;
}

// The launch order of a later call (order[slot] = feature).  Iteration counts with a tail: longest first.  Without one (every
// feature takes about as long): in space — features of one image region next to each other AND on one XCD, so that the window
// loads of a level entry find their lines in that XCD's L2 instead of every L2 fetching the whole pyramid (`ref_uv`: this call's
// reference pixels at level 0, `cols` x `rows` that level; `group`: features per workgroup of the launch the order is for).
//
// ONE workgroup does this beside the feature workgroups of a launch, so it must not outlast them: two passes over the list, both
// histograms (256 iteration bins, 256 image tiles) counted in the first, and the global loads of kOrderBatch elements per thread
// in flight together (one load per trip had made each pass a chain of ~100 dependent L2 round trips: 137 us for 25 000 features
// and 1.16 ms for 200 000 — longer than the 200 000-feature launch itself).
constexpr int kOrderBatch = 8;

__device__ __forceinline__ void klt_order_block(const uint32_t *iters, int32_t *order, int n, int *lds, const float *ref_uv, int cols, int rows, int group,
                                                uint32_t *sched_flags, uint32_t sched_call) {
    int *bin_count = lds, *bin_start = lds + 256, *tile_count = lds + 512, *tile_start = lds + 768, *flat = lds + 1024;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const bool spatial = ref_uv != nullptr && cols >= 16 && rows >= 16;
    const float inv_tile_u = 16.0f / (float)(cols > 0 ? cols : 1), inv_tile_v = 16.0f / (float)(rows > 0 ? rows : 1);
    const float2 *uv2 = reinterpret_cast<const float2 *>(ref_uv);
    for (int k = tid; k < 256; k += nt) {
        bin_count[k] = 0;
        tile_count[k] = 0;
    }
    __syncthreads();
    for (int base = 0; base < n; base += nt * kOrderBatch) {
        uint32_t it[kOrderBatch];
        float2 uv[kOrderBatch];
#pragma unroll
        for (int u = 0; u < kOrderBatch; ++u) {
            // unconditional loads of a clamped index through 32-bit byte offsets from the uniform bases: two instructions of address
            const uint32_t i = (uint32_t)min(base + u * nt + tid, n - 1);
            it[u] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(iters) + i * 4u);
            uv[u] = spatial ? *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(uv2) + i * 8u) : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < kOrderBatch; ++u) {
            const bool active = base + u * nt + tid < n;
            wave_bin_count(bin_count, active ? 255 - (int)min(it[u], 255u) : 0, active);
            if (spatial && active) {
                // tile keys are spread over the bins: one plain LDS atomic per lane, nothing returned
                (void)__hip_atomic_fetch_add(&tile_count[image_tile(uv[u].x, uv[u].y, inv_tile_u, inv_tile_v)], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    if (tid < 64) {
        // exclusive scans of both histograms by one wave: four bins per lane; and the no-tail test on the iteration counts
        const int l = tid;
        const int c0 = bin_count[4 * l], c1 = bin_count[4 * l + 1], c2 = bin_count[4 * l + 2], c3 = bin_count[4 * l + 3];
        // bin k holds count 255 - k: weighted sum and largest count over the tracked features (count > 0: bins 0..254)
        long long weighted = (long long)c0 * (255 - 4 * l) + (long long)c1 * (254 - 4 * l) + (long long)c2 * (253 - 4 * l) + (long long)c3 * (252 - 4 * l);
        int tracked = c0 + c1 + c2 + c3 - (l == 63 ? c3 : 0);
        int largest = c0 ? 255 - 4 * l : (c1 ? 254 - 4 * l : (c2 ? 253 - 4 * l : (c3 ? 252 - 4 * l : 0)));
        for (int off = 32; off >= 1; off >>= 1) {
            weighted += __shfl_xor(weighted, off);
            tracked += __shfl_xor(tracked, off);
            largest = max(largest, __shfl_xor(largest, off));
        }
        order_scan_bins(bin_count, bin_start, l);
        order_scan_bins(tile_count, tile_start, l);
        if (l == 0) {
            *flat = (tracked == 0 || 2ll * largest * tracked <= 3ll * weighted) ? 1 : 0;  // largest <= 1.5 x mean
        }
    }
    __syncthreads();
    if (tid == 0 && sched_flags != nullptr) {
        sched_flags[sched_call & 1u] = sched_flag_pack(sched_call, 0u) | (*flat != 0 ? 1u : 0u);  // for the NEXT launch's slots (sched_resolve_slot)
    }
    const bool by_tile = *flat != 0 && spatial;
    if (*flat != 0 && !spatial) {
        for (int i = tid; i < n; i += nt) {
            order[i] = i;
        }
        return;
    }
    for (int base = 0; base < n; base += nt * kOrderBatch) {
        uint32_t it[kOrderBatch];
        float2 uv[kOrderBatch];
#pragma unroll
        for (int u = 0; u < kOrderBatch; ++u) {
            const uint32_t i = (uint32_t)min(base + u * nt + tid, n - 1);
            it[u] = by_tile ? 0u : *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(iters) + i * 4u);
            uv[u] = by_tile ? *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(uv2) + i * 8u) : make_float2(0.0f, 0.0f);
        }
        int bin[kOrderBatch], slot[kOrderBatch];
        bool active[kOrderBatch];
#pragma unroll
        for (int u = 0; u < kOrderBatch; ++u) {
            active[u] = base + u * nt + tid < n;
            bin[u] = !active[u] ? 0 : (by_tile ? image_tile(uv[u].x, uv[u].y, inv_tile_u, inv_tile_v) : 255 - (int)min(it[u], 255u));
        }
        if (by_tile) {
#pragma unroll
            for (int u = 0; u < kOrderBatch; ++u) {
                slot[u] = active[u] ? atomicAdd(&tile_start[bin[u]], 1) : 0;  // all in flight before the first is used
            }
        } else {
            wave_bin_claim_batch<kOrderBatch>(bin_start, bin, active, slot);
        }
#pragma unroll
        for (int u = 0; u < kOrderBatch; ++u) {
            if (active[u]) {
                order[by_tile ? xcd_major_slot(slot[u], n, group) : slot[u]] = base + u * nt + tid;
            }
        }
    }
}

}  // namespace ftk
