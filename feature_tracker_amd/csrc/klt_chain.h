// klt_chain.h — the sums of a Gauss-Newton step in the reference's order: one lane per sum over pipelined LDS reads
// (chain_lane, chain_groups, chain_chunk), a quad of lanes per sum through the DPP network ("quad chain"), and the butterfly
// of the throughput mode (tree_sums).  A translation unit may define FTK_CHAIN_ROUND (float4 per prefetch round) first.
// Used by the three tracker translation units and direct_kernels.hip.
#pragma once

#include "ftk_device.h"

namespace ftk {
namespace {

// Phase B: lane k < K of wave 0 adds terms[k][0..Ppad) strictly left to right and publishes the sum.
// The adds form one dependent chain (that IS the reference's order); the LDS reads are software
// pipelined one round (8 x ds_read_b128 = 32 terms) ahead in two ping-pong register sets, pinned
// in place with sched_barrier, so that the chain of v_add_f32 — not the ds_read latency — sets the
// pace.  The prefetch may run up to 16 float4 past the end of a row: it stays inside the
// workgroup's LDS carve (the arrays behind `terms` are larger than that) and is never consumed.
#ifndef FTK_CHAIN_ROUND
#define FTK_CHAIN_ROUND 8
#endif
constexpr int kChainRound = FTK_CHAIN_ROUND;

// The reads of a round are issued LAST-CONSUMED FIRST: LDS data returns in issue order, so the wait in front of the round's first
// add (its float4 was issued last) covers the whole round — one s_waitcnt per round instead of one per float4.  A lone wave issues
// one instruction of ANY kind per 4 cycles (scripts/microbench/dep_add_latency.hip: a dependent v_add_f32 costs 4, an s_nop or
// s_waitcnt in between 4 more), so the waits were a ninth of the chain loop's instructions.
__device__ __forceinline__ void chain_load(float4 (&q)[kChainRound], const float4 *t) {
#pragma unroll
    for (int d = 0; d < kChainRound; ++d) {
        const int e = kChainRound - 1 - d;
        q[e] = t[e];
    }
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ float chain_consume(float acc, const float4 (&q)[kChainRound], int count) {
#pragma unroll
    for (int d = 0; d < kChainRound; ++d) {
        if (d < count) {
            acc += q[d].x;
            acc += q[d].y;
            acc += q[d].z;
            acc += q[d].w;
        }
    }
    return acc;
}

__device__ __forceinline__ float chain_consume_all(float acc, const float4 (&q)[kChainRound]) {
#pragma unroll
    for (int d = 0; d < kChainRound; ++d) {
        acc += q[d].x;
        acc += q[d].y;
        acc += q[d].z;
        acc += q[d].w;
    }
    __builtin_amdgcn_sched_barrier(0);
    return acc;
}

__device__ __forceinline__ float chain_lane(const float *row, int Ppad, float acc = 0.0f) {
    const float4 *t = reinterpret_cast<const float4 *>(row);
    const int n4 = Ppad >> 2;
    float4 qa[kChainRound], qb[kChainRound];
    int i = 0;
    chain_load(qa, t);
    for (; i + 2 * kChainRound <= n4; i += 2 * kChainRound) {
        chain_load(qb, t + i + kChainRound);
        acc = chain_consume_all(acc, qa);
        chain_load(qa, t + i + 2 * kChainRound);
        acc = chain_consume_all(acc, qb);
    }
    chain_load(qb, t + i + kChainRound);
    const int rem = n4 - i;  // 0 .. 2*kChainRound-1 float4 left, the first kChainRound already in qa
    acc = chain_consume(acc, qa, rem);
    acc = chain_consume(acc, qb, rem - kChainRound);
    return acc;
}

// Throughput mode (ftk_set_reduction_mode): the sums of K term rows by ALL 64 lanes of one wave — lane l adds the terms
// l, l + 64, ... of a row, a butterfly adds the lanes; four rows at a time so that the shuffles of one cover the latency of the
// others.  A fixed order, not the reference's: the results are NOT bit-identical to the CPU path (reported, never asserted).
__device__ __forceinline__ void tree_sums(const float *terms, int K, int Ppad, float *sums, int lane) {
    for (int k0 = 0; k0 < K; k0 += 4) {
        float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = lane; i < Ppad; i += kWave) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                part[j] += (k0 + j < K) ? terms[(k0 + j) * Ppad + i] : 0.0f;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                part[j] += __shfl_xor(part[j], off, kWave);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + j < K) {
                    sums[k0 + j] = part[j];
                }
            }
        }
    }
}

// The same chain over a GROUPED layout: the terms of four consecutive pixels of one sum sit in one float4 and consecutive
// groups lie kStride4 float4 apart ([group][sum][4 pixels], written by the pixel lanes with immediate offsets).  Same adds in the
// same order as chain_lane.  `rounds` rounds of kChainRound groups: the caller pads the group count to a multiple of kChainRound
// with zero terms (x + 0 == x for every value a sum can hold), so no load is guarded and none runs past the last group — a
// stride's worth of overrun per prefetched group would leave the carve.
template <int kStride4>
__device__ __forceinline__ void chain_load_groups(float4 (&q)[kChainRound], const float4 *t) {
#pragma unroll
    for (int d = 0; d < kChainRound; ++d) {
        const int e = kChainRound - 1 - d;
        q[e] = t[e * kStride4];
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int kStride4>
__device__ __forceinline__ float chain_groups(const float4 *t, int rounds, float acc) {
    // Branch-free body (a conditional load of a loop-carried register set costs a copy of the set per trip): the prefetch two
    // rounds ahead always happens, from round 0 again once it would pass the end — in bounds, never consumed.
    float4 qa[kChainRound], qb[kChainRound];
    chain_load_groups<kStride4>(qa, t);
    int r = 0;
#pragma nounroll  // with a compile-time round count (13 x 13 instantiations) full unrolling takes the kernel from 81 to 128 VGPRs
    for (; r + 2 <= rounds; r += 2) {
        chain_load_groups<kStride4>(qb, t + (r + 1) * (kChainRound * kStride4));
        acc = chain_consume_all(acc, qa);
        const int ahead = (r + 2 < rounds) ? r + 2 : 0;  // wave-uniform: a scalar select
        chain_load_groups<kStride4>(qa, t + ahead * (kChainRound * kStride4));
        acc = chain_consume_all(acc, qb);
    }
    if (r < rounds) {
        acc = chain_consume_all(acc, qa);  // odd count: round r was loaded as `ahead`
    }
    return acc;
}

// 64 strictly ordered adds of one chunk row (lane k < kTerms of the consumer wave), 16 terms per batch in two
// ping-pong register sets.  The compiler hoists every ds_read of the unrolled chunk to its top if it may (64 VGPRs
// of terms live at once — the difference between 4 and 5-6 waves per SIMD for this kernel); sched_barrier does not
// stop that, a data dependency does: the address of batch k + 2 is tied to the accumulator after batch k, so its
// reads issue exactly when their registers are free, one batch (16 dependent adds) ahead of their use.
__device__ __forceinline__ int chain_tie(float acc) {
    int zero = 0;
    asm volatile("" : "+v"(zero) : "v"(acc));
    return zero;
}

#if FTK_CHAIN_ROUND == 4  // written for 4 batches of 16 terms (a 64-pixel chunk); translation units with another round do not use it
__device__ __forceinline__ float chain_chunk(float acc, const float *row) {
    const float4 *t = reinterpret_cast<const float4 *>(row);
    float4 qa[kChainRound], qb[kChainRound];
    chain_load(qa, t);
    chain_load(qb, t + kChainRound);
    acc = chain_consume_all(acc, qa);
    chain_load(qa, t + 2 * kChainRound + chain_tie(acc));
    acc = chain_consume_all(acc, qb);
    chain_load(qb, t + 3 * kChainRound + chain_tie(acc));
    acc = chain_consume_all(acc, qa);
    acc = chain_consume_all(acc, qb);
    return acc;
}

// The chunk a patch ENDS in: its lanes [left, 64) wrote exact zeros, and x + (+-0) == x for every value a sum can hold (the sums start
// at +0 and -0 never arises: +0 + (-0) == +0), so only the 16-term batches that hold a patch pixel are read and added — at 13 x 13
// (41 pixels in the third chunk) 48 adds and 12 reads instead of 64 and 16, in every chain pass of every iteration.  Same adds in the
// same order up to the last patch pixel: bit-identical.  `left` = patch pixels in this chunk (wave-uniform; >= 64 for a full chunk).
__device__ __forceinline__ float chain_chunk_left(float acc, const float *row, int left) {
    if (left > 3 * 4 * kChainRound) {
        return chain_chunk(acc, row);
    }
    const float4 *t = reinterpret_cast<const float4 *>(row);
    float4 qa[kChainRound], qb[kChainRound];
    chain_load(qa, t);
    if (left > 2 * 4 * kChainRound) {  // 33 .. 48 pixels: three batches
        chain_load(qb, t + kChainRound);
        acc = chain_consume_all(acc, qa);
        chain_load(qa, t + 2 * kChainRound + chain_tie(acc));
        acc = chain_consume_all(acc, qb);
        return chain_consume_all(acc, qa);
    }
    if (left > 4 * kChainRound) {  // 17 .. 32: two
        chain_load(qb, t + kChainRound);
        acc = chain_consume_all(acc, qa);
        return chain_consume_all(acc, qb);
    }
    return chain_consume_all(acc, qa);  // 1 .. 16: one
}
#endif


// ---------------------------------------------------------------------------------------------
// The exact-order chain through the DPP network ("quad chain", round 5).
//
// chain_chunk above gives every sum ONE lane, which reads 4 of its terms per ds_read_b128 and adds them: one read instruction per
// 4 terms — and a lone wave issues one instruction of ANY kind per 4 cycles and pays 9 - 14 for an LDS read, so a term costs 8.5 - 10.7
// cycles although the dependent add itself needs 4 (scripts/microbench/dpp_quad_chain.hip, V0).  Here every sum has a QUAD of lanes,
// all four holding the same running value: lane i of quad q reads the float4 at terms 16 j + 4 i of sum q, so ONE ds_read_b128 brings
// 16 consecutive terms of up to 16 sums into the wave, and sixteen `v_add_f32_dpp acc, T, acc quad_perm:[i,i,i,i]` add them in
// order — quad lane 0's x, y, z, w, then lane 1's, ... — the DPP network broadcasting lane i's register to its quad.  The same
// IEEE adds in the same order (the DPP operand is the TERM; the accumulator is the plain src1, forwarded from the add before:
// no wait state, 64 000 random sums of 448 terms bit-identical), 4.84 cycles per term from registers, 6.6 with a chunk's four reads
// issued up front (V2 / V4 of the microbenchmark) against 10.7.  The loads are ordinary C++ loads (the compiler places their waits);
// the adds are one asm block per 16 terms.  Every lane of the wave must be active (EXEC all ones: no VALU write of EXEC in front of
// a DPP instruction); quads beyond the last sum follow any valid row and their results are ignored.
// ---------------------------------------------------------------------------------------------
#define FTK_QADD(i, reg) "v_add_f32_dpp %0, " reg ", %0 quad_perm:[" #i "," #i "," #i "," #i "] row_mask:0xf bank_mask:0xf\n"
#define FTK_QADD4(i) FTK_QADD(i, "%1") FTK_QADD(i, "%2") FTK_QADD(i, "%3") FTK_QADD(i, "%4")
// acc += the quad's 16 terms in order.  `s_nop 1`: should the compiler have MOVED a term register with a VALU instruction right in
// front of this block, the two wait states a DPP operand needs after a VALU write are there (it cannot see the DPP in the asm).
__device__ __forceinline__ float chain_quad_step16(float acc, const float4 q) {
    asm volatile("s_nop 1\n" FTK_QADD4(0) FTK_QADD4(1) FTK_QADD4(2) FTK_QADD4(3) : "+v"(acc) : "v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w));
    return acc;
}

// 64 terms (four reads) in one block: one `s_nop` and one wait for the reads per 64 adds instead of per 16 — a lone wave issues an
// instruction of any kind every 4 - 5 cycles, so each instruction that is not an add costs as much as a term.
#define FTK_QADD4R(i, a, b, c, d) FTK_QADD(i, a) FTK_QADD(i, b) FTK_QADD(i, c) FTK_QADD(i, d)
#define FTK_QADD16R(a, b, c, d) FTK_QADD4R(0, a, b, c, d) FTK_QADD4R(1, a, b, c, d) FTK_QADD4R(2, a, b, c, d) FTK_QADD4R(3, a, b, c, d)
__device__ __forceinline__ float chain_quad_step64(float acc, const float4 q0, const float4 q1, const float4 q2, const float4 q3) {
    asm volatile("s_nop 1\n" FTK_QADD16R("%1", "%2", "%3", "%4") FTK_QADD16R("%5", "%6", "%7", "%8") FTK_QADD16R("%9", "%10", "%11", "%12")
                     FTK_QADD16R("%13", "%14", "%15", "%16")
                 : "+v"(acc)
                 : "v"(q0.x), "v"(q0.y), "v"(q0.z), "v"(q0.w), "v"(q1.x), "v"(q1.y), "v"(q1.z), "v"(q1.w), "v"(q2.x), "v"(q2.y), "v"(q2.z), "v"(q2.w),
                   "v"(q3.x), "v"(q3.y), "v"(q3.z), "v"(q3.w));
    return acc;
}

// One chunk row of up to 64 terms: `quad_row` = the row of THIS lane's quad's sum + 4 * (lane & 3) floats (16-byte aligned);
// `left` = terms that count (wave-uniform, >= 1; anything >= 64 is a full chunk); terms up to the next multiple of 16 are read and
// added, so they must be exact zeros (x + (+-0) == x for every value a sum can hold: the sums start at +0).  All four reads of the
// chunk are issued first; each 16-add block waits only for its own.
__device__ __forceinline__ float chain_quads_left(float acc, const float *quad_row, int left) {
    const float4 *t = reinterpret_cast<const float4 *>(quad_row);
    const float4 q0 = t[0];
    if (left > 48) {
        const float4 q1 = t[4], q2 = t[8], q3 = t[12];
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q0);  // (16-add blocks here: the reads were issued just now, and the first block can start on the
        acc = chain_quad_step16(acc, q1);  // first read; one 64-add block measured 1.6 - 2.3 % slower in the pipelined Basic kernel)
        acc = chain_quad_step16(acc, q2);
        return chain_quad_step16(acc, q3);
    }
    if (left > 32) {
        const float4 q1 = t[4], q2 = t[8];
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q0);
        acc = chain_quad_step16(acc, q1);
        return chain_quad_step16(acc, q2);
    }
    if (left > 16) {
        const float4 q1 = t[4];
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q0);
        return chain_quad_step16(acc, q1);
    }
    return chain_quad_step16(acc, q0);
}

// `count` FULL chunks (count >= 1, wave-uniform), `step4` float4 from one chunk's row to the next.  Four term registers as in
// chain_quads_left, but each is read again — for the NEXT chunk — as soon as its 16 adds are through, so a read has the other 48 adds
// to arrive: no LDS latency between chunks, no registers beyond chain_quads_left's (a second set of four cost the pipelined Basic
// kernel a wave per SIMD), one address per chunk.  (Behind the last chunk the reads repeat that chunk: valid memory, never used.)
__device__ __forceinline__ float chain_quads_chunks(float acc, const float4 *t, int count, int step4) {
    float4 q0 = t[0], q1 = t[4], q2 = t[8], q3 = t[12];
#pragma nounroll
    for (int w = 0; w < count; ++w) {
        t += w + 1 < count ? step4 : 0;
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q0);
        q0 = t[0];
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q1);
        q1 = t[4];
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q2);
        q2 = t[8];
        __builtin_amdgcn_sched_barrier(0);
        acc = chain_quad_step16(acc, q3);
        q3 = t[12];
    }
    return acc;
}

// `n16` 16-term steps (n16 >= 1, wave-uniform) from `t_lane` = this lane's first float4, consecutive steps `step4` float4 apart: two
// register pairs, the reads two steps ahead of the adds.
// kBlocks64 (the one-wave-per-feature kernels, where the chain wave is alone on its SIMD and every issued instruction counts: Basic /
// affine fast on the real pair -4 .. -5 %): 64-add blocks; otherwise (the multi-wave kernels: no consistent difference) 16-add blocks.
template <bool kBlocks64 = false>
__device__ __forceinline__ float chain_quads_strided(float acc, const float4 *t, int n16, int step4) {
    if constexpr (kBlocks64) {
        // blocks of four steps (64 adds in one asm block), the reads of the next block issued before the adds of this one; the up to
        // three steps behind the last block are read up front and kept in registers (no LDS latency at the end of the chain)
        const int rem = n16 & 3, tail = n16 - rem;
        const float4 r0 = t[(rem > 0 ? tail : 0) * step4], r1 = t[(rem > 1 ? tail + 1 : 0) * step4], r2 = t[(rem > 2 ? tail + 2 : 0) * step4];
        if (tail > 0) {
            float4 a0 = t[0], a1 = t[step4], a2 = t[2 * step4], a3 = t[3 * step4], b0, b1, b2, b3;
            int j = 0;
#pragma nounroll
            for (;;) {
                const bool more_b = j + 8 <= tail;
                if (more_b) {
                    b0 = t[(j + 4) * step4];
                    b1 = t[(j + 5) * step4];
                    b2 = t[(j + 6) * step4];
                    b3 = t[(j + 7) * step4];
                }
                __builtin_amdgcn_sched_barrier(0);
                acc = chain_quad_step64(acc, a0, a1, a2, a3);
                j += 4;
                if (!more_b) {
                    break;
                }
                const bool more_a = j + 8 <= tail;
                if (more_a) {
                    a0 = t[(j + 4) * step4];
                    a1 = t[(j + 5) * step4];
                    a2 = t[(j + 6) * step4];
                    a3 = t[(j + 7) * step4];
                }
                __builtin_amdgcn_sched_barrier(0);
                acc = chain_quad_step64(acc, b0, b1, b2, b3);
                j += 4;
                if (!more_a) {
                    break;
                }
            }
        }
        if (rem > 0) {
            acc = chain_quad_step16(acc, r0);
        }
        if (rem > 1) {
            acc = chain_quad_step16(acc, r1);
        }
        if (rem > 2) {
            acc = chain_quad_step16(acc, r2);
        }
        return acc;
    } else {
        float4 qa = t[0], qb = t[n16 > 1 ? step4 : 0], qc, qd;
        int j = 0;
#pragma nounroll
        for (; j + 4 <= n16; j += 4) {
            qc = t[(j + 2) * step4];
            qd = t[(j + 3) * step4];
            __builtin_amdgcn_sched_barrier(0);
            acc = chain_quad_step16(acc, qa);
            acc = chain_quad_step16(acc, qb);
            qa = t[(j + 4 < n16 ? j + 4 : 0) * step4];  // (wave-uniform selects; a read past the end is never made)
            qb = t[(j + 5 < n16 ? j + 5 : 0) * step4];
            __builtin_amdgcn_sched_barrier(0);
            acc = chain_quad_step16(acc, qc);
            acc = chain_quad_step16(acc, qd);
        }
        const int rem = n16 - j;  // 0 .. 3 steps left; qa / qb hold the first two
        if (rem > 2) {
            qc = t[(j + 2) * step4];
            __builtin_amdgcn_sched_barrier(0);
        }
        if (rem > 0) {
            acc = chain_quad_step16(acc, qa);
        }
        if (rem > 1) {
            acc = chain_quad_step16(acc, qb);
        }
        if (rem > 2) {
            acc = chain_quad_step16(acc, qc);
        }
        return acc;
    }
}

// A whole row [n16 * 16 terms] of one sum: `quad_row` = the row + 4 * (lane & 3) floats.
template <bool kBlocks64 = false>
__device__ __forceinline__ float chain_quads_row(float acc, const float *quad_row, int n16) {
    return chain_quads_strided<kBlocks64>(acc, reinterpret_cast<const float4 *>(quad_row), n16, 4);
}

constexpr int kChunkPixels = 64;              // pixels per chunk of the chunked sweep / chain loops = one wave round
constexpr int kChunkRow = kChunkPixels + 4;   // ring row pitch in floats: the chain lanes' 16-byte reads of different rows hit different banks

}  // namespace
}  // namespace ftk
