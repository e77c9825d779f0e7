// klt_ldlt.h — the Eigen-compatible LDLT solvers: the generic one in registers (ldlt_solve<N>), the written-out 3 x 3 of the
// LSSD trackers, the lane-parallel 6 x 6 of the affine trackers and the direct method, and where the affine chain lanes put
// their Hessian sums for it.  Used by klt_kernels.hip, klt_fast_kernels.hip and direct_kernels.hip.
#pragma once

#include "klt_scalar.h"

#include <math.h>

namespace ftk {
namespace {

// ---------------------------------------------------------------------------------------------
// Eigen-compatible LDLT solve, N in {2, 3, 6}, everything in registers (all loops unrolled,
// pivot swaps predicated on compile-time indices so nothing is dynamically indexed).
// Mirrors the published Eigen 3.3.7+ algorithm; see oracle/oracle_substrate.c for the statement.
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void ldlt_solve(float (&m)[N][N], const float (&b)[N], float (&x)[N]) {
    int tr[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        tr[k] = k;
    }
    bool degenerate = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (!degenerate) {
            int p = k;
            float biggest = fabsf(m[k][k]);
#pragma unroll
            for (int i = k + 1; i < N; ++i) {
                const float cand = fabsf(m[i][i]);
                if (cand > biggest) {
                    biggest = cand;
                    p = i;
                }
            }
            tr[k] = p;
#pragma unroll
            for (int q = k + 1; q < N; ++q) {
                if (p == q) {
#pragma unroll
                    for (int j = 0; j < k; ++j) {
                        swap_values(m[k][j], m[q][j]);
                    }
#pragma unroll
                    for (int i = q + 1; i < N; ++i) {
                        swap_values(m[i][k], m[i][q]);
                    }
                    swap_values(m[k][k], m[q][q]);
#pragma unroll
                    for (int i = k + 1; i < q; ++i) {
                        swap_values(m[i][k], m[q][i]);
                    }
                }
            }
            if (k > 0) {
                float temp[N];
#pragma unroll
                for (int j = 0; j < k; ++j) {
                    temp[j] = m[j][j] * m[k][j];
                }
                float dot = m[k][0] * temp[0];
#pragma unroll
                for (int j = 1; j < k; ++j) {
                    dot += m[k][j] * temp[j];
                }
                m[k][k] -= dot;
#pragma unroll
                for (int i = k + 1; i < N; ++i) {
                    float s = m[i][0] * temp[0];
#pragma unroll
                    for (int j = 1; j < k; ++j) {
                        s += m[i][j] * temp[j];
                    }
                    m[i][k] -= s;
                }
            }
            const float akk = m[k][k];
            const bool pivot_valid = fabsf(akk) > 0.0f;
            if (k == 0 && !pivot_valid) {
                tr[0] = 0;
                degenerate = true;
            } else if (pivot_valid) {
#pragma unroll
                for (int i = k + 1; i < N; ++i) {
                    m[i][k] /= akk;
                }
            }
        }
    }

    float y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        y[i] = b[i];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int q = k + 1; q < N; ++q) {
            if (tr[k] == q) {
                swap_values(y[k], y[q]);
            }
        }
    }
#pragma unroll
    for (int i = 1; i < N; ++i) {
        float s = m[i][0] * y[0];
#pragma unroll
        for (int j = 1; j < i; ++j) {
            s += m[i][j] * y[j];
        }
        y[i] -= s;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (fabsf(m[i][i]) > 1.17549435e-38f) {
            y[i] /= m[i][i];
        } else {
            y[i] = 0.0f;
        }
    }
#pragma unroll
    for (int i = N - 2; i >= 0; --i) {
        float s = m[i + 1][i] * y[i + 1];
#pragma unroll
        for (int j = i + 2; j < N; ++j) {
            s += m[j][i] * y[j];
        }
        y[i] -= s;
    }
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
#pragma unroll
        for (int q = k + 1; q < N; ++q) {
            if (tr[k] == q) {
                swap_values(y[k], y[q]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[i] = y[i];
    }
}

// ldlt_solve<3> written out for the symmetric 3x3 system of the LSSD trackers (lssd_klt.cpp:107, lssd_klt_fast.cpp:87): the
// same operations in the same order — Eigen's LDLT is left-looking, so the pivot search of step k sees ORIGINAL diagonal
// entries (moved by the swaps) and the two transpositions can be decided up front; only the lower triangle is ever read.
// ~40 % of the instructions of the generic unrolled form (no 3x3 array with predicated swaps of every element).
// Independent divisions of WAVE-UNIFORM values side by side: lane k divides numerator k (the lanes beyond the last repeat it),
// the quotients come back through v_readlane.  One correctly rounded division sequence (~10 instructions) instead of one per
// quotient, and each quotient is the same instruction sequence on the same operands as before — bit-identical.
__device__ __forceinline__ void lane_div2(int lane, float n0, float n1, float d, float &q0, float &q1) {
    const float q = (lane == 0 ? n0 : n1) / d;
    q0 = bcast_lane(q, 0);
    q1 = bcast_lane(q, 1);
}

// kLanes: the inputs are wave-uniform and all 64 lanes are executing (the one-wave trackers): independent divisions run on
// separate lanes (lane_div2 and its three-way form below); otherwise every lane divides for itself as before.
template <bool kLanes = false>
__device__ __forceinline__ void ldlt3_solve(float a00, float a10, float a20, float a11, float a21, float a22, const float (&b)[3], float (&x)[3],
                                            int lane = 0) {
    // step 0: pivot = first maximum of |a00|, |a11|, |a22|
    float m00 = a00, m10 = a10, m20 = a20, m11 = a11, m21 = a21, m22 = a22;
    const float d0 = fabsf(m00), d1 = fabsf(m11), d2 = fabsf(m22);
    int p0 = 0;
    float biggest = d0;
    if (d1 > biggest) {
        biggest = d1;
        p0 = 1;
    }
    if (d2 > biggest) {
        p0 = 2;
    }
    if (p0 == 1) {  // rows / columns 0 <-> 1 of the lower triangle: m[2][0] <-> m[2][1], the diagonals
        swap_values(m20, m21);
        swap_values(m00, m11);
    } else if (p0 == 2) {  // 0 <-> 2: the diagonals, m[1][0] <-> m[2][1]
        swap_values(m00, m22);
        swap_values(m10, m21);
    }
    const bool valid0 = fabsf(m00) > 0.0f;
    const bool degenerate = !valid0;  // a zero first pivot: Eigen stops, the transpositions become the identity
    int p1 = 1;
    if (!degenerate) {
        if (kLanes) {
            lane_div2(lane, m10, m20, m00, m10, m20);
        } else {
            m10 /= m00;
            m20 /= m00;
        }
        // step 1: pivot among the remaining diagonals
        if (fabsf(m22) > fabsf(m11)) {
            p1 = 2;
            swap_values(m10, m20);
            swap_values(m11, m22);
        }
        {
            const float temp0 = m00 * m10;
            const float dot = m10 * temp0;
            m11 -= dot;
            const float s = m20 * temp0;
            m21 -= s;
        }
        if (fabsf(m11) > 0.0f) {
            m21 /= m11;
        }
        // step 2
        {
            const float temp0 = m00 * m20, temp1 = m11 * m21;
            float dot = m20 * temp0;
            dot += m21 * temp1;
            m22 -= dot;
        }
    } else {
        p0 = 0;
    }
    // y = P b
    float y0 = b[0], y1 = b[1], y2 = b[2];
    if (p0 == 1) {
        swap_values(y0, y1);
    } else if (p0 == 2) {
        swap_values(y0, y2);
    }
    if (p1 == 2) {
        swap_values(y1, y2);
    }
    // L^-1
    y1 -= m10 * y0;
    {
        float s = m20 * y0;
        s += m21 * y1;
        y2 -= s;
    }
    // D^+
    if (kLanes) {
        const float num = lane == 0 ? y0 : (lane == 1 ? y1 : y2);
        const float den = lane == 0 ? m00 : (lane == 1 ? m11 : m22);
        const float q = (fabsf(den) > 1.17549435e-38f) ? num / den : 0.0f;
        y0 = bcast_lane(q, 0);
        y1 = bcast_lane(q, 1);
        y2 = bcast_lane(q, 2);
    } else {
        y0 = (fabsf(m00) > 1.17549435e-38f) ? y0 / m00 : 0.0f;
        y1 = (fabsf(m11) > 1.17549435e-38f) ? y1 / m11 : 0.0f;
        y2 = (fabsf(m22) > 1.17549435e-38f) ? y2 / m22 : 0.0f;
    }
    // L^-T
    y1 -= m21 * y2;
    {
        float s = m10 * y1;
        s += m20 * y2;
        y0 -= s;
    }
    // P^T
    if (p1 == 2) {
        swap_values(y1, y2);
    }
    if (p0 == 1) {
        swap_values(y0, y1);
    } else if (p0 == 2) {
        swap_values(y0, y2);
    }
    x[0] = y0;
    x[1] = y1;
    x[2] = y2;
}

// ---------------------------------------------------------------------------------------------
// The same 6x6 LDLT, rows spread over lanes (affine trackers, direct method).
//
// ldlt_solve<6> above is ~1 000 dependent instructions on one lane per Gauss-Newton iteration — the
// longest serial stretch of an affine iteration.  Two facts make it parallel without changing a
// single rounding:
//   * Eigen's in-place LDLT is LEFT-looking: step k touches column k only, so the diagonal entries
//     the pivot search looks at are still the ORIGINAL ones (moved by the swaps).  The whole pivot
//     order can therefore be replayed up front on the six diagonal magnitudes alone, with the same
//     strict '>' first-maximum rule and the same position swaps.
//   * with the permutation known, row i of B = P A P^T lives on lane i: column k of L is one
//     multiply-add sweep over all lanes at once (same products, same left-to-right sums per
//     element), the divisions of a column happen side by side, and the triangular solves
//     broadcast one y_j per step.
// a_lds: 36 floats, row-major, symmetric (bitwise).  All 64 lanes of ONE wave call; lanes 0..5 work.
// ---------------------------------------------------------------------------------------------
struct Ldlt6 {
    float l[6];    // lane i: L(i, j) for j < i (unit diagonal implied), of the permuted matrix
    float d_mine;  // lane i: D(i)
    int perm;      // lane i: original index of position i
};


// Element (i, j) of the symmetric matrix: a row-major 6 x 6 in LDS (the non-fast affine trackers' chain lanes store their 18
// distinct Hessian sums straight into it, klt_kernels.hip affine_dense_slots).
struct Ldlt6Dense {
    const float *a;
    __device__ __forceinline__ float operator()(int i, int j) const { return a[i * 6 + j]; }
};

template <typename Elem>
__device__ __forceinline__ Ldlt6 ldlt6_factor_of(const Elem &elem, int lane);

__device__ __forceinline__ Ldlt6 ldlt6_factor(const float *a_lds, int lane) { return ldlt6_factor_of(Ldlt6Dense{a_lds}, lane); }

// my_ad: |A(i, i)| on lane i < 6 (anything elsewhere); ad_all[j]: the same six magnitudes, wave-uniform.  Callers that hold the
// diagonal in registers (the non-fast affine trackers: the chain lanes' accumulators) pass it in and save two LDS round trips.
template <typename Elem>
__device__ __forceinline__ Ldlt6 ldlt6_factor_diag(float my_ad, const float (&ad_all)[6], const Elem &elem, int lane);

template <typename Elem>
__device__ __forceinline__ Ldlt6 ldlt6_factor_of(const Elem &elem, int lane) {
    const int me0 = lane < 6 ? lane : 5;
    const float my_ad = fabsf(elem(me0, me0));
    float ad_all[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        ad_all[j] = bcast_lane(my_ad, j);
    }
    return ldlt6_factor_diag(my_ad, ad_all, elem, lane);
}

template <typename Elem>
__device__ __forceinline__ Ldlt6 ldlt6_factor_diag(float my_ad, const float (&ad_all)[6], const Elem &elem, int lane) {
    // ---- pivot order, replayed on the diagonal ----
    // Distinct, non-NaN magnitudes (the normal case): selection with swaps is then simply the descending order,
    // and lane i finds its own position as the number of larger magnitudes — six broadcasts instead of a serial
    // selection sort.  Ties, NaN or an all-zero diagonal take the literal replay (first maximum, position swaps).
    int rank = 0, equal = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        rank += (ad_all[j] > my_ad) ? 1 : 0;
        equal += (ad_all[j] == my_ad) ? 1 : 0;
    }
    rank = lane < 6 ? rank : 99;  // lanes that hold no row never match a position
    equal = lane < 6 ? equal : 1;
    const bool irregular = wave_ballot(equal != 1) != 0ull;  // equal == 0: NaN; > 1: a tie
    int pos[6];
    bool degenerate = false;
    if (!irregular) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            pos[k] = __builtin_ctzll(wave_ballot(rank == k));  // exactly one lane holds each rank here: v_cmp + s_ff1
        }
        // the largest magnitude is positive here (six distinct non-negative numbers), so the first pivot is valid
    } else {
        float ad[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            ad[i] = ad_all[i];
            pos[i] = i;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            int p = k;
            float biggest = ad[k];
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                if (ad[i] > biggest) {
                    biggest = ad[i];
                    p = i;
                }
            }
            if (k == 0) {
                // the k == 0 pivot is its (unmodified) diagonal entry: |akk| > 0 fails for an all-zero / NaN diagonal,
                // and the reference then stops factorising (identity order from here on)
                degenerate = !(biggest > 0.0f);
            }
#pragma unroll
            for (int q = k + 1; q < 6; ++q) {
                if (p == q && !(degenerate && k > 0)) {
                    swap_values(ad[k], ad[q]);
                    swap_values(pos[k], pos[q]);
                }
            }
        }
    }
    // ---- row `lane` of the permuted matrix ----
    const int me = lane < 6 ? lane : 5;
    int pi = pos[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) {
        pi = (me == i) ? pos[i] : pi;
    }
    float bmat[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        bmat[j] = elem(pi, pos[j]);
    }
    Ldlt6 f;
    f.perm = pi;
    f.d_mine = 0.0f;
    float dl[6];  // lane i: D(j) * L(i, j) — the product is formed on every lane BEFORE the broadcast (one multiply by a uniform,
                  // off the critical path as soon as column j is known) instead of after it (uniform x uniform: a copy + a multiply)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float m_ik = bmat[k];
        if (k > 0) {
            // temp[j] = D(j) * L(k, j); s = sum_j L(i, j) * temp[j], j ascending — the reference's order
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < k; ++j) {
                const float temp_j = bcast_lane(dl[j], k);
                s = (j == 0) ? f.l[0] * temp_j : s + f.l[j] * temp_j;
            }
            m_ik = degenerate ? m_ik : m_ik - s;
        }
        const float akk = bcast_lane(m_ik, k);
        f.d_mine = (me == k) ? akk : f.d_mine;
        const bool pivot_valid = fabsf(akk) > 0.0f;
        f.l[k] = (pivot_valid && !degenerate) ? m_ik / akk : m_ik;  // meaningful on lanes > k
        dl[k] = akk * f.l[k];
    }
    return f;
}

__device__ __forceinline__ void ldlt6_solve(const Ldlt6 &f, const float *b_lds, float *x_lds, int lane) {
    const int me = lane < 6 ? lane : 5;
    float y = b_lds[f.perm];  // transpositions applied to the right-hand side
    // forward: y_i -= sum_{j<i} L(i, j) y_j, j ascending
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float yj = bcast_lane(y, j);  // final: lane j committed its sum at the end of step j - 1
        s = (j == 0) ? f.l[0] * yj : s + f.l[j] * yj;
        y = (me == j + 1) ? y - s : y;
    }
    // D^+: components with |d| <= FLT_MIN become 0
    y = (fabsf(f.d_mine) > 1.17549435e-38f) ? y / f.d_mine : 0.0f;
    // backward: y_i -= sum_{j>i} L(j, i) y_j, j ascending; the terms of column i live on lanes j > i
#pragma unroll
    for (int i = 4; i >= 0; --i) {
        const float term = f.l[i] * y;  // lane j: L(j, i) * y_j
        float t = bcast_lane(term, i + 1);
#pragma unroll
        for (int j = i + 2; j < 6; ++j) {
            t = t + bcast_lane(term, j);
        }
        y = (me == i) ? y - t : y;
    }
    if (lane < 6) {
        x_lds[f.perm] = y;  // transpositions undone
    }
}

// ---------------------------------------------------------------------------------------------
// Affine KLT (6x6).  Chain indices of the 18 distinct Hessian product sequences + 6 bias ones.
// H(1,2) = H(0,3), H(1,4) = H(0,5) are the same products; H(3,4) is yy*dxdy as in the reference
// (affine_klt.cpp:245, sic), i.e. the same sequence as H(2,3).
// ---------------------------------------------------------------------------------------------
enum {
    A_XX_DXDX, A_XX_DXDY, A_XY_DXDX, A_XY_DXDY, A_X_DXDX, A_X_DXDY, A_XX_DYDY, A_XY_DYDY, A_X_DYDY, A_YY_DXDX, A_YY_DXDY, A_Y_DXDX, A_Y_DXDY,
    A_YY_DYDY, A_Y_DYDY, A_DXDX, A_DXDY, A_DYDY, A_B0, A_B1, A_B2, A_B3, A_B4, A_B5, A_COUNT
};

// Where chain lane s < 18 stores its sum in the dense row-major 6 x 6 Hessian (H(1,2) = H(0,3), H(1,4) = H(0,5), H(3,4) = H(2,3): the
// aliases of affine_klt.cpp:264-270 and the (sic) of :245): up to four entries e = 6 i + j per sum, one byte each (sums with fewer
// entries repeat one).  Row i of chain indices: 0 1 2 3 4 5 | 1 6 3 7 5 8 | 2 3 9 10 11 12 | 3 7 10 13 10 14 | 4 5 11 10 15 16 | 5 8 12 14 16 17.
__device__ __forceinline__ uint32_t affine_dense_slots(int sum) {
    constexpr uint32_t kSlots[18] = {
        0x00000000u | 0u * 0x01010101u,                           //  0: H00
        1u | 6u << 8 | 1u << 16 | 6u << 24,                       //  1: H01 H10
        2u | 12u << 8 | 2u << 16 | 12u << 24,                     //  2: H02 H20
        3u | 18u << 8 | 8u << 16 | 13u << 24,                     //  3: H03 H30 H12 H21
        4u | 24u << 8 | 4u << 16 | 24u << 24,                     //  4: H04 H40
        5u | 30u << 8 | 10u << 16 | 25u << 24,                    //  5: H05 H50 H14 H41
        7u * 0x01010101u,                                         //  6: H11
        9u | 19u << 8 | 9u << 16 | 19u << 24,                     //  7: H13 H31
        11u | 31u << 8 | 11u << 16 | 31u << 24,                   //  8: H15 H51
        14u * 0x01010101u,                                        //  9: H22
        15u | 20u << 8 | 22u << 16 | 27u << 24,                   // 10: H23 H32 H34 H43
        16u | 26u << 8 | 16u << 16 | 26u << 24,                   // 11: H24 H42
        17u | 32u << 8 | 17u << 16 | 32u << 24,                   // 12: H25 H52
        21u * 0x01010101u,                                        // 13: H33
        23u | 33u << 8 | 23u << 16 | 33u << 24,                   // 14: H35 H53
        28u * 0x01010101u,                                        // 15: H44
        29u | 34u << 8 | 29u << 16 | 34u << 24,                   // 16: H45 H54
        35u * 0x01010101u,                                        // 17: H55
    };
    return kSlots[sum < 18 ? sum : 17];
}
// chain lanes that hold the diagonal H(j, j), j = 0..5
constexpr int kAffineDiagLane[6] = {A_XX_DXDX, A_XX_DYDY, A_YY_DXDX, A_YY_DYDY, A_DXDX, A_DYDY};

}  // namespace
}  // namespace ftk
