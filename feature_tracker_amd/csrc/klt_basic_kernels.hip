// klt_basic_kernels.hip — Basic KLT, inverse method (the headline configuration): pipelined kernel.
//
// Same contract as klt_track_kernel<FTK_MODEL_BASIC, FTK_METHOD_INVERSE> (klt_kernels.hip) — one
// workgroup per feature, ONE launch per TrackFeatures call, sums in the reference's row-major order,
// results bit-identical to the scalar CPU path (basic_klt.cpp:7-181) — with three structural changes
// that remove most of the instruction and latency cost of the generic kernel:
//
//  1. Reference-side LATTICE instead of five taps per pixel.  The five reference taps of pixel
//     (r, c) sit at (y_r, x_c), (y_r, x_c -+ 1), (y_r -+ 1, x_c) with y_r = float(r - h) + v,
//     x_c = float(c - h) + u (basic_klt.cpp:127-134).  Along one axis the tap coordinates take only a
//     few distinct float values: the len + 2 values {y_0 - 1, y_0 ... y_{len-1}, y_{len-1} + 1},
//     plus an "extra" node wherever fl(y_r - 1) != y_{r-1} or fl(y_r + 1) != y_{r+1} bitwise —
//     that happens only where the unit step crosses a binade boundary, so at most
//     2 * (log2(len + 2) + 3) times per axis.  Every tap of the patch is therefore the bilinear value
//     at a node pair (row node, column node), computed ONCE per level with exactly the per-tap
//     expressions (same fractions, same weights, same sum order): ~(len + 2)^2 bilinears instead of
//     5 * len^2.  Per patch row / column an index triple (centre, minus, plus) says which nodes
//     its taps use; gx, gy and i_ref are read back from the lattice each iteration.
//
//  2. Windows prefetched, as plain bytes.  At level entry the global loads of the current-image window
//     and of the NEXT level's reference window are issued into registers, the node tables and the
//     lattice of this level are built meanwhile, and only then are the loads consumed (LDS stores).
//     A window row is `pitch` bytes (a power of two, ftk_device.h klt_byte_pitch: 32 at 21x21), staged
//     in 8-byte units that go to LDS as they came from memory — unit -> (row, position) is a shift
//     and a mask, one unit per thread and window at 21x21 on two waves — and a tap reads the two
//     aligned dwords around its pixel in each of its two rows and shifts them into place (node_tap:
//     as many LDS reads as with pairs; four single-byte reads measured 6 % slower than pairs, and a
//     16-bit read at an odd address 22 %, docs/LAB_NOTES.md).  The generic and the one-wave kernels
//     keep 16-bit pixel pairs (klt_window.h Win), whose staging is four times the work.  The
//     reference window is one row / column larger than the generic kernel's so that a valid tap is
//     always covered (a coordinate sum may round up to the next integer), hence no global-memory
//     fallback sampler exists here.
//
//  3. Producer / consumer waves.  Wave 0 runs the five exact-order chains (one lane each) over
//     64-pixel chunks while the other wave(s) compute the next chunk's per-pixel products; chunks
//     travel through a two-slot LDS ring, one barrier per chunk.  The chain — 441 dependent adds
//     per iteration at 21x21, the latency floor of bit-identical sums — then overlaps the sampling
//     instead of following it.  With one wave per feature the same loop runs both roles in turn.
//
// Arithmetic contract as in klt_kernels.hip: IEEE fp32, no contraction, correctly rounded division.
#define FTK_CHAIN_ROUND 4  // 16 terms per round: the consumer wave holds 32 VGPRs of prefetched terms
#include "klt_chain.h"
#include "klt_ldlt.h"
#include "klt_order.h"
#include "klt_plan.h"
#include "klt_scalar.h"
#include "klt_stage.h"
#include "klt_window.h"

namespace ftk {
namespace {

constexpr int kChunk = 64;  // pixels per chunk = one producer wave round
// What a chunk is.  LINEAR: pixels [64 k, 64 k + 64) of the row-major patch — every lane divides its pixel number by the patch width in
// every chunk.  ROW chunks: kChunk / patch_cols WHOLE patch rows, the lanes behind them idle (exact zeros in the ring) — a lane's column
// and its row within the chunk are then the same in every chunk, on every level and in every iteration.  Row chunks are taken where
// they do not add a chunk (each one is a barrier and 64 chain adds): 21 x 21 has 7 chunks either way (3 rows = 63 pixels); 13 x 13
// would go from 3 to 4 and 11 x 11 from 2 to 3, so they stay linear, as does the run-time geometry (patch_rows = 0 here).
constexpr bool pb_row_chunks(int patch_rows, int patch_cols) {
    if (patch_rows < 1 || patch_cols < 1 || patch_cols > kChunk) {
        return false;
    }
    const int rows_per_chunk = kChunk / patch_cols;
    return (patch_rows + rows_per_chunk - 1) / rows_per_chunk == (patch_rows * patch_cols + kChunk - 1) / kChunk;
}
// The chunk geometry of an instantiation <HR, HC> (0 / 0: run-time geometry).
template <int HR, int HC>
struct PbChunks {
    static constexpr int kRows = HR > 0 && HC > 0 ? 2 * HR + 1 : 0, kCols = HR > 0 && HC > 0 ? 2 * HC + 1 : 0;
    static constexpr bool kByRows = pb_row_chunks(kRows, kCols);
    static constexpr int kRowsPerChunk = kByRows ? kChunk / kCols : 1;
    static constexpr int kCount = kByRows ? (kRows + kRowsPerChunk - 1) / kRowsPerChunk : 0;  // chunks per patch (row chunks only)
    static constexpr bool kLastRowsShort = kCount * kRowsPerChunk > kRows;                    // the last chunk has rows beyond the patch
};
static_assert(PbChunks<10, 10>::kByRows && PbChunks<10, 10>::kCount == 7 && !PbChunks<10, 10>::kLastRowsShort, "21 x 21: seven chunks of three rows");
static_assert(!PbChunks<6, 6>::kByRows && !PbChunks<5, 5>::kByRows && !PbChunks<0, 0>::kByRows, "13 x 13, 11 x 11 and the run-time geometry stay linear");
// Ring rows are kChunk + 4 floats apart: the consumer's lanes read 16 bytes each from DIFFERENT rows
// at the same column, and a row pitch of 256 B would put all of them on the same four banks.
// (round 5: the quad chain reads 16 bytes per lane, the four lanes of a quad 64 consecutive bytes of ONE row; a pitch of 80 floats puts
// the rows of the two quads of an 8-lane group on the two halves of the banks.  Its quads follow klt_chain.h chain_quads_left.)
constexpr int kRingRow = kChunk + 16;
constexpr int kTerms = 5;   // 0 H00, 1 H11, 2 H01, 3 -fx*ft, 4 -fy*ft (basic_klt.cpp:139-144)
// 8-byte window loads a thread holds in flight per window: what the instantiation's windows need on its fewest threads (one wave
// solo, two otherwise).  The run-time geometry (rows = 0) holds kRunTimeRefOctets / kRunTimeCurOctets, the slot counts of the pair
// staging this replaced: a unit carries twice the pixels of a quad and a pitch is less than twice the columns, so every window
// those covered is covered (up to 33 x 33 on two waves); a window with more units is staged after the lattice instead.
constexpr int kRunTimeRefOctets = 3, kRunTimeCurOctets = 4;
constexpr int pb_octets(int rows, int pitch, bool solo, int run_time) {
    return rows > 0 ? (rows * (pitch / 8) + (solo ? 64 : 128) - 1) / (solo ? 64 : 128) : run_time;
}

__host__ __device__ inline int pb_pad4(int x) { return (x + 3) & ~3; }
__host__ __device__ inline int pb_producers(int waves) { return waves > 1 ? waves - 1 : 1; }
// Ring slots: with separate producer and consumer waves the chunk being chained and the chunk being produced
// coexist (2 slots); a single wave produces and then chains each chunk itself (1 slot, 1.4 KB of LDS saved —
// LDS, not registers, is what caps the resident features per CU for the one-wave configuration).
__host__ __device__ inline int pb_ring_slots(int waves) { return waves > 1 ? 2 : 1; }

// LDS carve-up (float4 regions first so that every region keeps its natural alignment).
struct PbLds {
    float4 *rnodes, *cnodes;  // lattice nodes per axis: {window element offset, fraction, 1 - fraction, valid}
    uint4 *ridx, *cidx;       // per patch row / column: {centre node, minus node, plus node, all three valid}
    float4 *ctab;             // per producer wave: 2 float4 per patch row, then per patch column (see cur_tables)
    float *ring;              // [2][producers][kTerms][kRingRow]
    float *lattice;           // [n_r][n_c] reference bilinear values
    float *sol;               // 4 floats: published solution
    uint32_t *slots;          // 16: node counts (0, 1), valid-pixel counts by iteration parity (4 + 4 * parity + wave)
    // Byte windows (klt_stage.h "Byte windows"), rows pb_rwin_pitch / pb_cwin_pitch bytes apart, inside regions that are still sized
    // for 16-bit pixel pairs (pb_lds_bytes: 2 * pad4(rows * cols) bytes each; klt_byte_windows_ok holds the pitch to that room).
    uint8_t *ref_win;         // two reference windows (this level, next level), ref_win_stride BYTES apart
    int ref_win_stride;
    uint8_t *cur_win;
};

// Current-tap tables: one per producer wave; in the throughput mode (p.tree) every wave samples, so one per wave.
__host__ __device__ inline int pb_tables(const KltParams &p, int waves) { return p.tree ? waves : pb_producers(waves); }

__host__ __device__ inline size_t pb_lds_bytes(const KltParams &p, int waves) {
    const int np = pb_producers(waves);
    size_t bytes = 16 * (size_t)(p.pb_cap_r + p.pb_cap_c);
    bytes += 16 * (size_t)(p.patch_rows + p.patch_cols);
    bytes += 16 * (size_t)pb_tables(p, waves) * 2 * (p.patch_rows + p.patch_cols);
    bytes += 4 * (size_t)pb_ring_slots(waves) * np * kTerms * kRingRow;
    bytes += 4 * (size_t)pb_pad4(p.pb_cap_r * p.pb_cap_c);
    bytes += 4 * 4 + 4 * 16;
    bytes += 2 * (size_t)2 * pb_pad4(p.pb_rwin_rows * p.pb_rwin_cols);
    bytes += 2 * (size_t)pb_pad4(p.cwin_rows * p.cwin_cols);
    return (bytes + 15) & ~(size_t)15;
}

__device__ __forceinline__ PbLds pb_carve(float4 *base, const KltParams &p, int waves) {
    const int np = pb_producers(waves);
    PbLds c;
    c.rnodes = base;
    c.cnodes = c.rnodes + p.pb_cap_r;
    c.ridx = reinterpret_cast<uint4 *>(c.cnodes + p.pb_cap_c);
    c.cidx = c.ridx + p.patch_rows;
    c.ctab = reinterpret_cast<float4 *>(c.cidx + p.patch_cols);
    c.ring = reinterpret_cast<float *>(c.ctab + pb_tables(p, waves) * 2 * (p.patch_rows + p.patch_cols));
    c.lattice = c.ring + pb_ring_slots(waves) * np * kTerms * kRingRow;
    c.sol = c.lattice + pb_pad4(p.pb_cap_r * p.pb_cap_c);
    c.slots = reinterpret_cast<uint32_t *>(c.sol + 4);
    c.ref_win = reinterpret_cast<uint8_t *>(c.slots + 16);
    c.ref_win_stride = 2 * pb_pad4(p.pb_rwin_rows * p.pb_rwin_cols);
    c.cur_win = c.ref_win + 2 * c.ref_win_stride;
    return c;
}

// ---------------------------------------------------------------------------------------------
// Lattice nodes of one axis (executed by ONE wavefront; len <= 64).
//   x_t = float(t - h) + centre  — the coordinate of patch row / column t, as basic_klt.cpp:127-130
//   nodes: 0 = x_0 - 1, t + 1 = x_t, len + 1 = x_{len-1} + 1, then the extras.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 node_entry(float x, int limit, int lo, int extent, int pitch) {
    const Axis a = make_axis(x, limit);
    const int rel = (int)((unsigned)a.i0 - (unsigned)lo);
    const bool hit = (unsigned)rel < (unsigned)extent;
    // valid implies hit by construction of the windows; `hit` only keeps the LDS read in bounds
    return make_float4(__int_as_float(hit ? rel * pitch : 0), a.sub, a.inv, __int_as_float((a.valid && hit) ? 1 : 0));
}

struct AxisSpec {
    int len, h, limit, lo, extent, pitch, cap;
    float centre;
    float4 *nodes;
    uint4 *idx;
    uint32_t *n_out;
};

// One pass of one wavefront over up to two axes: lanes [0, A.len) work on axis A, lanes
// [A.len, A.len + B.len) on axis B (B.len == 0: A alone).  Requires A.len + B.len <= 64.
__device__ __forceinline__ void build_nodes_pass(int lane, const AxisSpec &A, const AxisSpec &B) {
    const bool is_b = lane >= A.len;
    const int len = is_b ? B.len : A.len;
    const int h = is_b ? B.h : A.h;
    const int limit = is_b ? B.limit : A.limit;
    const int lo = is_b ? B.lo : A.lo;
    const int extent = is_b ? B.extent : A.extent;
    const int pitch = is_b ? B.pitch : A.pitch;
    const int cap = is_b ? B.cap : A.cap;
    const float centre = is_b ? B.centre : A.centre;
    float4 *nodes = is_b ? B.nodes : A.nodes;
    uint4 *idx = is_b ? B.idx : A.idx;
    const int t = is_b ? lane - A.len : lane;
    const bool act = t < len;
    const unsigned long long mask_a = (A.len >= 64) ? ~0ull : ((1ull << A.len) - 1ull);
    const unsigned long long mask_ab = (A.len + B.len >= 64) ? ~0ull : ((1ull << (A.len + B.len)) - 1ull);
    const unsigned long long mine = is_b ? (mask_ab & ~mask_a) : mask_a;

    const float lim = (float)limit;
    const float x0 = (float)(t - h) + centre;
    const float xm = x0 - 1.0f;
    const float xp = x0 + 1.0f;
    const float xprev = (float)(t - 1 - h) + centre;
    const float xnext = (float)(t + 1 - h) + centre;
    const bool v0 = x0 >= 0.0f && x0 <= lim;
    const bool vm = xm >= 0.0f && xm <= lim;
    const bool vp = xp >= 0.0f && xp <= lim;
    const bool needm = act && t > 0 && vm && __float_as_uint(xm) != __float_as_uint(xprev);
    const bool needp = act && t < len - 1 && vp && __float_as_uint(xp) != __float_as_uint(xnext);
    const unsigned long long bm = wave_ballot(needm), bp = wave_ballot(needp);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int nm = (int)__popcll(bm & mine);
    int em = len + 2 + (int)__popcll(bm & mine & below);
    int ep = len + 2 + nm + (int)__popcll(bp & mine & below);
    int total = len + 2 + nm + (int)__popcll(bp & mine);
    // capacity guard (cap covers the provable maximum of extras; this only keeps LDS accesses in range)
    em = em < cap ? em : cap - 1;
    ep = ep < cap ? ep : cap - 1;
    total = total < cap ? total : cap;
    if (act) {
        nodes[t + 1] = node_entry(x0, limit, lo, extent, pitch);
        if (t == 0 || t == len - 1) {
            nodes[t == 0 ? 0 : len + 1] = node_entry(t == 0 ? xm : xp, limit, lo, extent, pitch);
        }
        const int im = (t == 0) ? 0 : (needm ? em : t);
        const int ip = (t == len - 1) ? len + 1 : (needp ? ep : t + 2);
        idx[t] = make_uint4((unsigned)(t + 1), (unsigned)im, (unsigned)ip, (v0 && vm && vp) ? 1u : 0u);
        if (t == 0) {
            *(is_b ? B.n_out : A.n_out) = (uint32_t)total;
        }
    }
    if (len == 1 && act) {
        nodes[2] = node_entry(xp, limit, lo, extent, pitch);  // a one-pixel axis: lane 0 owns both edge nodes
    }
    if ((bm | bp) != 0ull) {  // wave-uniform: most levels have no extra node
        if (needm) {
            nodes[em] = node_entry(xm, limit, lo, extent, pitch);
        }
        if (needp) {
            nodes[ep] = node_entry(xp, limit, lo, extent, pitch);
        }
    }
}

// A window of this kernel: bytes, `pitch` apart (a power of two >= cols + 1: element (r, c < cols) reads bytes c, c + 1 of rows r, r + 1).
struct PbWin {
    const uint8_t *data;
    int r_lo, c_lo;
    int rows, cols, pitch;  // wave-uniform
    float cover[4];         // as Win::cover (win_set_cover)
};

// Bilinear value of a node pair from an LDS window: tap_table() of the generic kernel.  No 16-bit read of the two neighbours: idx is
// odd half of the time, and single-byte reads double the LDS instructions of the kernel's most frequent read.
__device__ __forceinline__ float node_tap(const uint8_t *win, int pitch, const float4 &nr, const float4 &nc) {
    const int idx = __float_as_int(nr.x) + __float_as_int(nc.x);
    // two aligned dwords per row and an alignbyte: pixel idx, idx + 1 in bytes 0, 1 (the second dword is inside the row: pitch >= cols + 4)
    const uint32_t *const w = reinterpret_cast<const uint32_t *>(win) + (idx >> 2);
    const uint32_t top = __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)idx & 3u);
    const uint32_t bot = __builtin_amdgcn_alignbyte(w[(pitch >> 2) + 1], w[pitch >> 2], (uint32_t)idx & 3u);
    const unsigned tl = top & 0xFFu, tr = (top >> 8) & 0xFFu;
    const unsigned bl = bot & 0xFFu, br = (bot >> 8) & 0xFFu;
    const float w_tl = nr.z * nc.z;
    const float w_tr = nr.z * nc.y;
    const float w_bl = nr.y * nc.z;
    const float w_br = nr.y * nc.y;
    return w_tl * (float)tl + w_tr * (float)tr + w_bl * (float)bl + w_br * (float)br;
}

// Per-iteration tables of the current-image taps, private to one producer wave (so no barrier):
// entry t         = node_entry of the current coordinate of patch row / column t, w = valid AND the
//                   reference-side validity of that row / column
// entry total + t = lattice offsets {centre, minus, plus} of that row (pre-multiplied by n_c) / column
__device__ __forceinline__ void cur_tables(int lane, const KltParams &p, const PbLds &c, float4 *tab, const DevImage &cur, const PbWin &cw, float cur_u,
                                           float cur_v, int n_c) {
    const int total = p.patch_rows + p.patch_cols;
    for (int t = lane; t < total; t += kWave) {
        const bool is_row = t < p.patch_rows;
        const int d = is_row ? t : t - p.patch_rows;
        const float x = (float)(d - (is_row ? p.half_rows : p.half_cols)) + (is_row ? cur_v : cur_u);
        float4 e = node_entry(x, (is_row ? cur.rows : cur.cols) - 1, is_row ? cw.r_lo : cw.c_lo, is_row ? cw.rows - 1 : cw.cols,
                              is_row ? cw.pitch : 1);
        const uint4 id = is_row ? c.ridx[d] : c.cidx[d];
        e.w = __int_as_float(__float_as_int(e.w) & (int)id.w);
        const int mul = is_row ? n_c : 1;
        // two arrays, not interleaved pairs: the pixel lanes of a chunk read consecutive COLUMN entries with ds_read_b128, and
        // 32-byte strides put lanes i and i + 8 of a 16-lane group on the same banks (a 2-way conflict on every such read)
        tab[t] = e;
        tab[total + t] = make_float4(__int_as_float((int)id.x * mul), __int_as_float((int)id.y * mul), __int_as_float((int)id.z * mul), 0.0f);
    }
}

// Row chunks (PbChunks): what a lane keeps across chunks.  Its place, once per kernel; its column's two table entries, once per iteration
// (behind cur_tables): they are the same in every chunk, so a chunk reads only its row entries, at the lane's row + a wave-uniform offset.
struct PbLane {
    int row, col;  // row within the chunk, patch column; an idle lane sits on (0, 0), which is always in the tables
    bool in;       // the lane is a pixel of its chunk (lane < rows per chunk * patch_cols)
};
struct PbCols {
    float4 c0, c1;
};
template <class G>
__device__ __forceinline__ PbLane pb_lane(int lane) {
    PbLane l = {0, 0, false};
    if constexpr (G::kByRows) {
        constexpr uint32_t kMagic = (1048576 + G::kCols - 1) / G::kCols;  // lane < 64: exact (magic20)
        const int row = (int)(__umul24((uint32_t)lane, kMagic) >> 20);
        l.in = lane < G::kRowsPerChunk * G::kCols;
        l.row = l.in ? row : 0;
        l.col = l.in ? lane - row * G::kCols : 0;
    }
    return l;
}
template <class G>
__device__ __forceinline__ void pb_read_cols(const PbLane &l, const KltParams &p, const float4 *tab, PbCols &cols) {
    if constexpr (G::kByRows) {
        cols.c0 = tab[p.patch_rows + l.col];
        cols.c1 = tab[2 * p.patch_rows + p.patch_cols + l.col];
    }
}

// The five per-pixel products of one 64-pixel chunk (basic_klt.cpp:135-144); returns the lane's validity.
template <class G>
__device__ __forceinline__ bool chunk_products(int lane, int chunk, const KltParams &p, const PbLds &c, const float4 *tab, const PbWin &cw, const PbLane &l,
                                               const PbCols &cols, float (&prod)[kTerms]) {
    const int tab_total = p.patch_rows + p.patch_cols;
    bool in;
    float4 r0, r1, c0, c1;
    if constexpr (G::kByRows) {
        int prow = wadd(l.row, imul(chunk, G::kRowsPerChunk));  // (an unsigned sum and the 24-bit multiplier: a 32-bit LDS address, not a 64-bit multiply-add)
        in = l.in;
        if constexpr (G::kLastRowsShort) {  // (not at 21 x 21: 7 x 3 rows are the patch)
            in = in && prow < p.patch_rows;
            prow = in ? prow : 0;
        }
        r0 = tab[prow];
        r1 = tab[tab_total + prow];
        c0 = cols.c0;
        c1 = cols.c1;
    } else {
        const int pxi = chunk * kChunk + lane;
        in = pxi < p.P;
        const int pp = in ? pxi : 0;
        int prow, pcol;
        pixel_rc(p, pp, prow, pcol);
        r0 = tab[prow];
        r1 = tab[tab_total + prow];
        c0 = tab[p.patch_rows + pcol];
        c1 = tab[tab_total + p.patch_rows + pcol];
    }
    const float i_cur = node_tap(cw.data, cw.pitch, r0, c0);
    const float *lat = c.lattice;
    const int rc = __float_as_int(r1.x), rm = __float_as_int(r1.y), rp = __float_as_int(r1.z);
    const int cc = __float_as_int(c1.x), cm = __float_as_int(c1.y), cp = __float_as_int(c1.z);
    const float left = lat[rc + cm];
    const float right = lat[rc + cp];
    const float top = lat[rm + cc];
    const float bottom = lat[rp + cc];
    const float i_ref = lat[rc + cc];
    const bool ok = in && ((__float_as_int(r0.w) & __float_as_int(c0.w)) != 0);
    // an unused pixel contributes exact zeros (x + (+-0) == x)
    const float fx = ok ? right - left : 0.0f;
    const float fy = ok ? bottom - top : 0.0f;
    const float ft = ok ? i_cur - i_ref : 0.0f;
    prod[0] = fx * fx;
    prod[1] = fy * fy;
    prod[2] = fx * fy;
    prod[3] = -(fx * ft);
    prod[4] = -(fy * ft);
    return ok;
}

// ... -> ring slot (the exact mode: the consumer wave adds them in pixel order).
template <class G>
__device__ __forceinline__ bool produce_chunk(int lane, int chunk, const KltParams &p, const PbLds &c, const float4 *tab, const PbWin &cw, const PbLane &l,
                                              const PbCols &cols, float *slot) {
    float prod[kTerms];
    const bool ok = chunk_products<G>(lane, chunk, p, c, tab, cw, l, cols, prod);
#pragma unroll
    for (int k = 0; k < kTerms; ++k) {
        slot[k * kRingRow + lane] = prod[k];
    }
    return ok;
}

// Sum over the 64 lanes of a wave by a butterfly (the throughput mode's reduction: a fixed order, but not the reference's).
__device__ __forceinline__ void wave_sum5(float (&v)[kTerms]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kTerms; ++k) {
            v[k] += __shfl_xor(v[k], off, kWave);
        }
    }
}

// Exact ceil(2^20 / d) for 1 <= d <= 4096: q = (i * m) >> 20 equals i / d for i < 2^20 / d... (i * d < 2^20)
__device__ __forceinline__ uint32_t magic20(int d) {
    uint32_t m = (uint32_t)(1048576.0f / (float)d);
    while (m * (uint32_t)d < 1048576u) {
        ++m;
    }
    return m;
}

constexpr int kWavesPerEu = 4;

constexpr KltParams pb_geometry(int hr, int hc) {
    KltParams g = {};
    g.half_rows = hr;
    g.half_cols = hc;
    klt_fill_geometry(g);
    return g;
}

// The byte windows' staging rule (ftk_device.h klt_byte_window_inside) for a wave-uniform origin: four 32-bit scalar compares.
__device__ __forceinline__ bool pb_window_inside(const DevImage &im, int r_lo, int c_lo, int wrows, int pitch) {
    return klt_byte_window_inside(im.rows, im.cols, r_lo, c_lo, wrows, pitch);
}

// Workgroup barrier — or, for one-wave features packed several to a workgroup (solo), only a compiler fence: LDS operations of
// one wave execute in program order, and the other waves of the group work on other features.
__device__ __forceinline__ void pb_sync(bool solo) {
    if (solo) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// SOLO: one wave per feature, p.features_per_group features per workgroup (compile-time, so that the one-wave code carries none
// of the producer / consumer split).
// HR / HC: the half patch sizes as compile-time constants (the common ones are instantiated below), or 0 / 0 for "as passed":
// the whole patch / window / lattice geometry then folds into immediates (klt_fill_geometry) instead of being ~40 SGPR-resident
// kernel arguments, most of which the register allocator spills to vector lanes (106 SGPRs + 104 spills in the generic form).
// TREE: the throughput mode (ftk_set_reduction_mode, KltParams::tree) — every wave samples and keeps per-lane partial sums of the
// five products, a butterfly and a fixed-order sum over the waves replace the ring and the consumer's exact-order chain.  Same
// products, different summation order: NOT bit-identical to the reference; a separate instantiation so that the contract path's
// code is untouched by it.
template <bool SOLO, int HR, int HC, bool TREE>
__global__ void __attribute__((amdgpu_waves_per_eu(kWavesPerEu))) __launch_bounds__(256) klt_basic_inverse_pipelined_kernel(const KltParams p_arg) {
    // `p` carries everything but the level tables, which stay in the kernel argument (p_arg.ref / p_arg.cur): a local copy whose
    // arrays are indexed with a run-time level would be placed in scratch memory (measured: the kernel twice as slow).
    klt_touch_kernarg<sizeof(KltParams)>();  // every line of the argument block requested up front (klt_scalar.h)
    KltParams p = p_arg;
    if constexpr (HR > 0 && HC > 0) {
        p.half_rows = HR;
        p.half_cols = HC;
        klt_fill_geometry(p);  // the same function the host filled p_arg with: identical values, now compile-time
    }
    constexpr KltParams kGeo = pb_geometry(HR, HC);
    static_assert(HR == 0 || klt_byte_windows_ok(kGeo), "byte windows: power-of-two pitch inside the carved regions");
    constexpr int kCurOctets = pb_octets(HR > 0 ? kGeo.cwin_rows : 0, kGeo.pb_cwin_pitch, SOLO, kRunTimeCurOctets);
    constexpr int kRefOctets = pb_octets(HR > 0 ? kGeo.pb_rwin_rows : 0, kGeo.pb_rwin_pitch, SOLO, kRunTimeRefOctets);
    extern __shared__ float4 lds_raw[];
    Blk b;
    uint32_t id;
    float4 *lds_mine = lds_raw;
    // block 0 of a launch that carries the previous call's iteration counts sorts them into a later call's launch order
    // (klt_order.h) beside the feature workgroups; the feature blocks follow it
    uint32_t block = blockIdx.x;
    if (p.sort_iters) {
        if (block == 0) {
            klt_order_block(p.sort_iters, p.sort_order_out, p.n, reinterpret_cast<int *>(lds_raw), p.sort_ref_uv, p_arg.ref[0].cols, p_arg.ref[0].rows, SOLO ? max(p.features_per_group, 1) : 1,
                            p.sched_flags, p.sched_call);
            return;
        }
        block -= 1;
    }
    if (SOLO) {
        // One wave per feature, several features per workgroup: the waves of the group share nothing but the launch (each has
        // its own LDS carve and never meets the others at a barrier — pb_sync is a wave-local fence here).  The hardware admits
        // 16 workgroups per CU; packing lifts the cap of 16 ONE-wave features per CU (4 waves per SIMD) to what the
        // registers allow.
        b.tid = b.lane = threadIdx.x & (kWave - 1);
        b.nt = kWave;
        b.wave = 0;
        b.nwaves = 1;
        const uint32_t slot = threadIdx.x >> 6;
        id = block * (uint32_t)p.features_per_group + slot;
        lds_mine = lds_raw + (size_t)slot * (p.group_lds_stride >> 4);
    } else {
        b.tid = threadIdx.x;
        b.nt = blockDim.x;
        b.lane = b.tid & (kWave - 1);
        b.wave = b.tid >> 6;
        b.nwaves = b.nt >> 6;
        id = block;
    }
    constexpr bool solo = SOLO;
    if (id >= (uint32_t)p.n) {
        return;
    }
    const bool younger = 2u * id >= (uint32_t)p.n;  // launch slot in the later-dispatched half (set_level_priority)
    if (p.sched_claim != nullptr) {
        // a trade of places between an early slot and a late one whose POSITION predicts many iterations (klt_order.h
        // sched_resolve_slot; one wave decides for the workgroup)
        bool swapped_in = false;
        if (SOLO) {
            id = sched_resolve_slot(p, id, swapped_in);
        } else {
            uint32_t *const shared = reinterpret_cast<uint32_t *>(lds_raw);
            if (b.wave == 0) {
                const uint32_t r = sched_resolve_slot(p, id, swapped_in);
                if (b.lane == 0) {
                    shared[0] = r;
                }
            }
            __syncthreads();
            id = shared[0];
            __syncthreads();  // the word belongs to the carve below
        }
    }
    if (p.order) {
        id = (uint32_t)p.order[id];  // launch slot -> feature: longest first by the previous call's iteration counts
    }
    // the three per-feature inputs are requested together (one global round trip, not two one after the other)
    const float2 in_uv = reinterpret_cast<const float2 *>(p.cur_uv_in)[id];
    const float2 full_ref = reinterpret_cast<const float2 *>(p.ref_uv)[id];
    uint8_t status = p.status_in[id];
    const float in_u = in_uv.x, in_v = in_uv.y;
    // features beyond kMaxTrackPointsNumber and features that already failed are passed through (basic_klt.cpp:9,15)
    if (id >= p.n_track || status > FTK_TRACKED) {
        if (b.tid == 0) {
            p.cur_uv_out[2 * id] = in_u;
            p.cur_uv_out[2 * id + 1] = in_v;
            p.status_out[id] = status;
            if (p.iters) {
                p.iters[id] = 0;
            }
            if (p.sched_iters) {
                p.sched_iters[id] = 0;
            }
        }
        return;
    }
    const PbLds c = pb_carve(lds_mine, p, b.nwaves);
    const int np = pb_producers(b.nwaves);
    const bool producer = (b.nwaves == 1) || b.wave > 0;
    const bool consumer = b.wave == 0;
    const int pw = (b.nwaves == 1) ? 0 : b.wave - 1;  // producer index
    float4 *const my_tab = c.ctab + (TREE ? b.wave : pw) * 2 * (p.patch_rows + p.patch_cols);
    using G = PbChunks<HR, HC>;
    const PbLane my_px = pb_lane<G>(b.lane);
    const int n_chunks = G::kByRows ? G::kCount : (p.P + kChunk - 1) / kChunk;
    const int n_steps = (n_chunks + np - 1) / np;
    const int ring_mask = pb_ring_slots(b.nwaves) - 1;
    // (a last chunk of 49 .. 64 terms is a full one: its row is zero beyond P; so is every row chunk: its rows' terms, then zeros)
    const bool last_chunk_short = !G::kByRows && p.P - (n_chunks - 1) * kChunk <= 48;
    const float *const quad_rows = c.ring + min(b.lane >> 2, kTerms - 1) * kRingRow + 4 * (b.lane & 3);  // this lane's quad's sum, its 4 of every 16 terms

    // basic_klt.cpp:10,18-19 (pyramid) / :59-86 (single level)
    const float full_ref_u = full_ref.x, full_ref_v = full_ref.y;
    const float scale = p.single_level ? 1.0f : (float)(1 << (p.n_levels - 1));
    float ref_u = full_ref_u, ref_v = full_ref_v, cur_u = in_u, cur_v = in_v;
    if (!p.single_level) {
        // scale = 2^k: x * 2^-k is the correctly rounded x / 2^k, four multiplications instead of four ~11-instruction divisions in
        // every wave.  Taken only when the host has checked k <= 30 (p.scale_recip, klt_plan_call) and all four quotients are normal
        // numbers (|x| >= 2^(k - 126); a NaN fails the test) — the same answer in every lane of the wave; everything else divides.
        const uint32_t k = (uint32_t)(p.n_levels - 1);
        const float inv_scale = __uint_as_float((127u - k) << 23), least = __uint_as_float((1u + k) << 23);
        const bool normal = fabsf(full_ref_u) >= least && fabsf(full_ref_v) >= least && fabsf(in_u) >= least && fabsf(in_v) >= least;
        if (p.scale_recip && wave_ballot(!normal) == 0ull) {
            ref_u = full_ref_u * inv_scale;
            ref_v = full_ref_v * inv_scale;
            cur_u = in_u * inv_scale;
            cur_v = in_v * inv_scale;
        } else {
            ref_u = full_ref_u / scale;
            ref_v = full_ref_v / scale;
            cur_u = in_u / scale;
            cur_v = in_v / scale;
        }
    }

    const int rrows = p.pb_rwin_rows, rcols = p.pb_rwin_cols, rpitch = p.pb_rwin_pitch, cpitch = p.pb_cwin_pitch;
    const bool ref_fits = rrows * (rpitch >> 3) <= kRefOctets * b.nt, cur_fits = p.cwin_rows * (cpitch >> 3) <= kCurOctets * b.nt;

    int buf = 0;
    // origin of this level's reference window: computed once per level, as the NEXT level's origin while the level before it is entered
    int ref_r_lo, ref_c_lo;
    {
        // the coarsest level's reference window: nothing to overlap it with yet
        const DevImage ref = p_arg.ref[p.n_levels - 1];
        footprint_origin(p, ref_u, ref_v, ref_r_lo, ref_c_lo);
        stage_bytes_any(opaque_blk(b), ref, c.ref_win, ref_r_lo, ref_c_lo, rrows, rpitch);
    }
    uint32_t iters = 0;
    float out_u = in_u, out_v = in_v;
    // the column axis has patch_cols + 2 nodes on every level but those with an extra node: that divisor's magic once (a constant
    // in the compile-time geometries), not a float division and a correction loop per level in every thread
    const int base_n_c = p.patch_cols + 2;
    const uint32_t base_magic = (HC > 0) ? (uint32_t)((1048576 + base_n_c - 1) / base_n_c) : magic20(base_n_c);
    for (int level = p.n_levels - 1; level > -1; --level) {
        const DevImage ref = p_arg.ref[level];
        const DevImage cur = p_arg.cur[level];
        set_level_priority(level, younger);
        // ---- level entry: issue the window loads, build the node tables meanwhile ----
        PbWin rw, cw;
        rw.data = c.ref_win + buf * c.ref_win_stride;
        rw.rows = rrows;
        rw.cols = rcols;
        rw.pitch = rpitch;
        rw.r_lo = ref_r_lo;
        rw.c_lo = ref_c_lo;
        int need_r, need_c;
        footprint_origin(p, cur_u, cur_v, need_r, need_c);
        cw.data = c.cur_win;
        cw.r_lo = wadd(need_r, -p.cwin_margin);
        cw.c_lo = wadd(need_c, -p.cwin_margin);
        cw.rows = p.cwin_rows;
        cw.cols = p.cwin_cols;
        cw.pitch = cpitch;
        win_set_cover(p, cw);
        int nr_lo = 0, nc_lo = 0;
        if (level > 0) {
            footprint_origin(p, ref_u * 2.0f, ref_v * 2.0f, nr_lo, nc_lo);
        }
        const bool cur_async = cur_fits && pb_window_inside(cur, cw.r_lo, cw.c_lo, cw.rows, cpitch);
        const bool next_async = level > 0 && ref_fits && pb_window_inside(p_arg.ref[level > 0 ? level - 1 : 0], nr_lo, nc_lo, rrows, rpitch);
        // the window loads are issued FIRST (they depend on the footprints only) and fly while the node tables and
        // the lattice are built: at one wave per feature the level entry is a chain of dependent latencies
        RawOctets<kCurOctets> qc;
        RawOctets<kRefOctets> qn;
        if (cur_async) {
            issue_octets(qc, b, cur, cw.r_lo, cw.c_lo, cw.rows, cpitch);
        }
        if (next_async) {
            issue_octets(qn, b, p_arg.ref[level - 1], nr_lo, nc_lo, rrows, rpitch);
        }
        if (b.wave == 0) {
            // both axes' node tables in one pass of wave 0 (two passes when the patch has more than 64 rows + columns)
            AxisSpec ar = {p.patch_rows, p.half_rows, ref.rows - 1, rw.r_lo, rw.rows - 1, rw.pitch, p.pb_cap_r, ref_v, c.rnodes, c.ridx, &c.slots[0]};
            AxisSpec ac = {p.patch_cols, p.half_cols, ref.cols - 1, rw.c_lo, rw.cols, 1, p.pb_cap_c, ref_u, c.cnodes, c.cidx, &c.slots[1]};
            const int lane = opaque(b.lane);
            if (p.patch_rows + p.patch_cols <= kWave) {
                build_nodes_pass(lane, ar, ac);
            } else {
                AxisSpec none = ar;
                none.len = 0;
                build_nodes_pass(lane, ar, none);
                build_nodes_pass(lane, ac, none);
            }
        }
        pb_sync(solo);  // B1: node tables (and this level's reference window) visible
        // ---- lattice: one bilinear per node pair ----
        const int n_r = __builtin_amdgcn_readfirstlane((int)c.slots[0]), n_c = __builtin_amdgcn_readfirstlane((int)c.slots[1]);  // one value per feature
        {
            const int total = n_r * n_c;
            const uint32_t m = (n_c == base_n_c) ? base_magic : magic20(n_c);
            for (int idx = opaque(b.tid); idx < total; idx += b.nt) {
                const int r = (int)(__umul24((uint32_t)idx, m) >> 20);  // idx < 4096 and m <= 2^20: the 24-bit multiplier is exact here
                const int cc = idx - imul(r, n_c);
                c.lattice[idx] = node_tap(rw.data, rw.pitch, c.rnodes[r], c.cnodes[cc]);
            }
        }
        // ---- consume the prefetched loads ----
        if (cur_async) {
            store_octets(qc, b, c.cur_win, cw.rows, cpitch);
        } else {
            stage_bytes_any(opaque_blk(b), cur, c.cur_win, cw.r_lo, cw.c_lo, cw.rows, cpitch);
        }
        if (level > 0) {
            if (next_async) {
                store_octets(qn, b, c.ref_win + (buf ^ 1) * c.ref_win_stride, rrows, rpitch);
            } else {
                stage_bytes_any(opaque_blk(b), p_arg.ref[level - 1], c.ref_win + (buf ^ 1) * c.ref_win_stride, nr_lo, nc_lo, rrows, rpitch);
            }
        }
        pb_sync(solo);  // B2: lattice and windows visible

        // ---- Gauss-Newton iterations (TrackOneFeature, basic_klt.cpp:88-116) ----
        for (uint32_t iter = 0; iter < p.max_iteration; ++iter) {
            ++iters;
            if (iter > 0 && !win_covers(cw, cur_u, cur_v)) {  // four float compares in the usual case (klt_window.h win_set_cover)
                // restage the current window when the patch has left it (wave-uniform)
                footprint_origin(p, cur_u, cur_v, need_r, need_c);
                const long long nr = need_r, nc = need_c;
                const bool covered = nr >= (long long)cw.r_lo && nr + (2 * p.half_rows + 4) <= (long long)cw.r_lo + cw.rows &&
                                     nc >= (long long)cw.c_lo && nc + (2 * p.half_cols + 4) <= (long long)cw.c_lo + cw.cols + 1;
                if (!covered) {
                    cw.r_lo = wadd(need_r, -p.cwin_margin);
                    cw.c_lo = wadd(need_c, -p.cwin_margin);
                    win_set_cover(p, cw);
                    stage_bytes_any(opaque_blk(b), cur, c.cur_win, cw.r_lo, cw.c_lo, cw.rows, cpitch);
                    pb_sync(solo);
                }
            }
            uint32_t wave_valid = 0;
            float acc = 0.0f;
            PbCols my_cols = {};  // row chunks: this lane's column entries, the same for every chunk of the iteration
            if constexpr (TREE) {
                // throughput mode: no ring, no chain — every wave samples chunks wave, wave + W, ... into five per-lane partial sums
                float part[kTerms] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                cur_tables(b.lane, p, c, my_tab, cur, cw, cur_u, cur_v, n_c);
                __builtin_amdgcn_wave_barrier();
                pb_read_cols<G>(my_px, p, my_tab, my_cols);
                for (int chunk = b.wave; chunk < n_chunks; chunk += b.nwaves) {
                    float prod[kTerms];
                    const bool ok = chunk_products<G>(b.lane, chunk, p, c, my_tab, cw, my_px, my_cols, prod);
#pragma unroll
                    for (int k = 0; k < kTerms; ++k) {
                        part[k] += prod[k];
                    }
                    wave_valid += (uint32_t)__popcll(wave_ballot(ok));
                }
                wave_sum5(part);
                float *const wave_sums = c.ring;  // unused in this mode: [wave][kTerms]
                if (b.lane == 0) {
#pragma unroll
                    for (int k = 0; k < kTerms; ++k) {
                        wave_sums[b.wave * kTerms + k] = part[k];
                    }
                    c.slots[4 + 4 * (iter & 1u) + b.wave] = wave_valid;
                }
                pb_sync(solo);
                if (consumer) {
                    float tot[kTerms];
#pragma unroll
                    for (int k = 0; k < kTerms; ++k) {
                        tot[k] = wave_sums[k];
                        for (int w = 1; w < b.nwaves; ++w) {
                            tot[k] += wave_sums[w * kTerms + k];
                        }
                    }
                    float m[2][2], bb[2], sol[2];
                    m[0][0] = tot[0];
                    m[1][1] = tot[1];
                    m[0][1] = m[1][0] = tot[2];
                    bb[0] = tot[3];
                    bb[1] = tot[4];
                    ldlt_solve<2>(m, bb, sol);
                    if (b.lane == 0) {
                        c.sol[0] = sol[0];
                        c.sol[1] = sol[1];
                    }
                }
                pb_sync(solo);
            } else {
                if (producer) {
                    cur_tables(b.lane, p, c, my_tab, cur, cw, cur_u, cur_v, n_c);
                    __builtin_amdgcn_wave_barrier();  // same-wave LDS traffic is ordered; keep the compiler from reordering across
                    pb_read_cols<G>(my_px, p, my_tab, my_cols);
                }
                for (int s = 0; s < n_steps; ++s) {
                    if (producer) {
                        const int chunk = s * np + pw;
                        if (chunk < n_chunks) {
                            const bool ok = produce_chunk<G>(b.lane, chunk, p, c, my_tab, cw, my_px, my_cols, c.ring + ((s & ring_mask) * np + pw) * kTerms * kRingRow);
                            wave_valid += (uint32_t)__popcll(wave_ballot(ok));
                        }
                        if (s == n_steps - 1 && b.lane == 0) {
                            c.slots[4 + 4 * (iter & 1u) + b.wave] = wave_valid;
                        }
                    }
                    pb_sync(solo);
                    if (consumer) {
                        // the whole wave: quad k = lanes 4 k .. 4 k + 3 carries sum k (klt_chain.h, "quad chain"); the quads behind the
                        // fifth follow its rows and are ignored
                        // the step's chunks are all in the ring: the full ones in one go (the next chunk's reads under this one's adds),
                        // then the patch's last chunk if it has fewer than 49 terms
                        const int first = s * np, count = min(np, n_chunks - first);
                        const int full = count - ((first + count == n_chunks && last_chunk_short) ? 1 : 0);
                        const float *const row = quad_rows + ((s & ring_mask) * np) * (kTerms * kRingRow);
                        if (full > 0) {
                            acc = chain_quads_chunks(acc, reinterpret_cast<const float4 *>(row), full, kTerms * kRingRow / 4);
                        }
                        if (full < count) {
                            acc = chain_quads_left(acc, row + full * (kTerms * kRingRow), p.P - (n_chunks - 1) * kChunk);
                        }
                    }
                }
                if (consumer) {
                    float m[2][2], bb[2], sol[2];
                    const int acc_bits = __float_as_int(acc);
                    constexpr int kSumLanes = 4;  // sum k ends in lane 4 k (every lane of its quad)
                    m[0][0] = __int_as_float(__builtin_amdgcn_readlane(acc_bits, 0));
                    m[1][1] = __int_as_float(__builtin_amdgcn_readlane(acc_bits, 1 * kSumLanes));
                    m[0][1] = m[1][0] = __int_as_float(__builtin_amdgcn_readlane(acc_bits, 2 * kSumLanes));
                    bb[0] = __int_as_float(__builtin_amdgcn_readlane(acc_bits, 3 * kSumLanes));
                    bb[1] = __int_as_float(__builtin_amdgcn_readlane(acc_bits, 4 * kSumLanes));
                    ldlt_solve<2>(m, bb, sol);  // basic_klt.cpp:97
                    if (b.lane == 0) {
                        c.sol[0] = sol[0];
                        c.sol[1] = sol[1];
                    }
                }
                pb_sync(solo);  // B3: solution and valid counts visible
            }
            const float v0 = c.sol[0], v1 = c.sol[1];  // read together with the counts: one LDS round trip, not two
            uint32_t n_valid = 0;
            for (int w = ((b.nwaves == 1 || TREE) ? 0 : 1); w < b.nwaves; ++w) {
                n_valid += c.slots[4 + 4 * (iter & 1u) + w];
            }
            if (n_valid == 0) {
                break;  // basic_klt.cpp:94
            }
            if (isnan(v0) || isnan(v1)) {
                status = FTK_NUMERIC_ERROR;
                break;
            }
            cur_u += v0;
            cur_v += v1;
            if (uv_outside(cur_u, cur_v, cur)) {
                status = FTK_OUTSIDE;
                break;
            }
            if (v0 * v0 + v1 * v1 < p.converge) {
                status = FTK_TRACKED;
                break;
            }
        }

        if (level == 0) {
            out_u = cur_u;
            out_v = cur_v;
            break;
        }
        ref_u *= 2.0f;
        ref_v *= 2.0f;
        cur_u *= 2.0f;
        cur_v *= 2.0f;
        ref_r_lo = nr_lo;  // footprint_origin of the doubled position: what the level below would compute again
        ref_c_lo = nc_lo;
        buf ^= 1;
    }

    if (uv_outside(out_u, out_v, p_arg.cur[0])) {
        status = FTK_OUTSIDE;  // basic_klt.cpp:49-53
    }
    if (b.tid == 0) {
        p.cur_uv_out[2 * id] = out_u;
        p.cur_uv_out[2 * id + 1] = out_v;
        p.status_out[id] = status;
        if (p.iters) {
            p.iters[id] = iters;
        }
        tail_report(p, iters, id);  // the longest feature of the call, for the next call's wave policy
        sched_grid_record(p, full_ref_u, full_ref_v, out_u, out_v, iters);  // ... and by position
        if (p.sched_iters) {
            p.sched_iters[id] = iters;  // the next call's launch order (ftk_klt.cpp: longest first)
        }
    }
}


}  // namespace

namespace {
template <int HR, int HC>
KltKernel pick_kernel(bool solo, bool tree) {
    void (*entry)(const KltParams);
    if (tree) {
        entry = solo ? klt_basic_inverse_pipelined_kernel<true, HR, HC, true> : klt_basic_inverse_pipelined_kernel<false, HR, HC, true>;
    } else {
        entry = solo ? klt_basic_inverse_pipelined_kernel<true, HR, HC, false> : klt_basic_inverse_pipelined_kernel<false, HR, HC, false>;
    }
    return {entry, "pipelined", HR, solo, tree, false, false, PbChunks<HR, HC>::kByRows,
            pb_octets(HR > 0 ? pb_geometry(HR, HC).cwin_rows : 0, pb_geometry(HR, HC).pb_cwin_pitch, solo, kRunTimeCurOctets),
            pb_octets(HR > 0 ? pb_geometry(HR, HC).pb_rwin_rows : 0, pb_geometry(HR, HC).pb_rwin_pitch, solo, kRunTimeRefOctets)};
}
}  // namespace

size_t klt_pipelined_feature_lds_bytes(const KltParams &p) { return pb_lds_bytes(p, p.waves_per_feature); }

KltKernel klt_pipelined_pick(const KltParams &p) {
    const bool solo = p.waves_per_feature == 1;
    // compile-time geometry for the patch sizes of the BASELINE configurations and the reference's default (11x11, 13x13, 21x21);
    // the throughput mode (p.tree: reported, never the contract) has its own instantiations of the same set
    if (p.half_rows == p.half_cols) {
        KltParams check = p;
        klt_fill_geometry(check);  // the specialised kernels recompute exactly this: refuse them if the caller's geometry differs
        const bool same = check.pb_cap_r == p.pb_cap_r && check.pb_cap_c == p.pb_cap_c && check.cwin_rows == p.cwin_rows && check.cwin_cols == p.cwin_cols &&
                          check.pb_rwin_pitch == p.pb_rwin_pitch && check.pb_cwin_pitch == p.pb_cwin_pitch;
        if (same) {
            switch (p.half_rows) {
                case 5: return pick_kernel<5, 5>(solo, p.tree != 0);
                case 6: return pick_kernel<6, 6>(solo, p.tree != 0);
                case 10: return pick_kernel<10, 10>(solo, p.tree != 0);
                default: break;
            }
        }
    }
    return pick_kernel<0, 0>(solo, p.tree != 0);
}

// First-use cost out of the callers' timed regions (ftk_warmup): launching this empty kernel makes the runtime load this
// translation unit's code object onto the device, which otherwise happens inside the first real call.
__global__ void klt_basic_warm_kernel() {}
hipError_t klt_basic_warm(hipStream_t stream) {
    hipLaunchKernelGGL(klt_basic_warm_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

}  // namespace ftk
