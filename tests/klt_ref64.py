"""ref64: a float64 restatement of the reference's KLT family (Basic, Affine, LSSD x inverse, direct, fast).

TEST INFRASTRUCTURE ONLY.  Written from the reference's optical_flow_tracker sources, independently of oracle/*.c: it imports
nothing from oracle/ or tests/oracle_lib.py and shares none of its code.  Where the reference calls un-vendored code it follows
DESIGN.md §2's substrate table (GetPixelValue validity and bilinear, the truncating pyramid, static_cast<int32_t> out of range).

Precision rule: every sample coordinate is formed in float32 exactly as the reference forms it (e.g. `static_cast<float>(drow) +
uv.y()`, `affine * Vec2(dcol, drow)`, `R_cr * Vec2(col_i, row_i) + t_cr`), from the float32 rounding of the carried state, so
validity decisions are the reference's own.  Everything after that is float64: bilinear values, gradients, products, sums, the
solve (numpy.linalg.solve), the update and the state carried between iterations and levels.

Vectorised over features: every array is (n, patch).  Per feature the result carries, besides position / status / iterations,
the decision margins a test needs to exclude near-threshold features honestly:

* `m_converge`  smallest |(|v|^2 - kMaxConvergeStep)| / kMaxConvergeStep over the convergence tests taken;
* `m_large`     smallest |(|v|^2 - last |v|^2)| / last |v|^2 over the large-step tests taken (fast variants);
* `m_outside`   smallest px distance of a tested position to the outside bounds (0, cols-1, rows-1);
* `m_edge`      smallest px distance of a sample coordinate formed from a COMPUTED position to a validity edge (coordinates
                formed from the inputs alone are exact float32 values shared with any faithful implementation, so they carry no
                margin);
* `cond`        the largest condition number of a solved H, taken componentwise for the feature's new POSITION (Skeel's
                condition number against relative rounding of every summed term, in px, see _solve): how far rounding in a
                float32 implementation can move the position; `cond_raw` is the plain 2-norm condition number of H;
* `singular`    a solved H was singular (rank-deficient or all zero); such features are solved by pseudo-inverse and are not
                comparable (Eigen's zero-pivot rule decides them).

`Flags` switches each reference quirk off on its own, and carries the negative-control mutations the tests use to
show that they can fail.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR = range(5)  # feature_tracker.h TrackStatus

f32 = np.float32
_INT32_MIN = -2147483648


@dataclasses.dataclass(frozen=True)
class Flags:
    # Reference quirks, each on by default.
    no_half_gradient: bool = True            # central difference without 1/2 (basic_klt.cpp:135-137 and every variant)
    fast_status_reset: bool = True           # fast variants set kLargeResidual at each level (basic_klt_fast.cpp:29, affine_klt_fast.cpp:32, lssd_klt_fast.cpp:49)
    failed_level_continues: bool = True      # kOutside / kNumericError at a level does not stop finer levels (basic_klt.cpp:21-46)
    skip_incoming_failed: bool = True        # incoming status > kTracked is skipped (basic_klt.cpp:15)
    affine_h34_yy: bool = True               # H(3,4) += yy * dxdy (affine_klt.cpp:183,245; affine_klt_fast.cpp:132)
    affine_pyramid_identity: bool = True     # pyramid path starts from the identity, not predict_affine_ (affine_klt.cpp:21 vs :70)
    lssd_single_no_writeback: bool = True    # single-level LSSD never writes cur_pixel_uv (lssd_klt.cpp:72-89)
    lssd_mean_normalise: bool = True         # non-fast LSSD always divides by the patch means (lssd_klt.cpp:183-184,209-212)
    lssd_fast_luminance_mismatch: bool = True  # numerators / denominators of the fast luminance means (lssd_klt_fast.cpp:27-35,65-78)
    # Negative controls (mutations), each off by default.
    gradient_other_image: bool = False       # non-fast: gradient from the other image
    cur_lattice_row_shift: int = 0           # current-image patch rows shifted against the reference patch
    swap_sr_sc: bool = False                 # bilinear row / column fractions swapped
    validity_strict: bool = False            # GetPixelValue valid iff row < rows-1 (instead of <=)
    ex_patch_offset: int = 0                 # fast: extended reference patch lattice offset


QUIRKS = ("no_half_gradient", "fast_status_reset", "failed_level_continues", "skip_incoming_failed", "affine_h34_yy",
          "affine_pyramid_identity", "lssd_single_no_writeback", "lssd_mean_normalise", "lssd_fast_luminance_mismatch")
DEFAULT = Flags()


# ---- substrate -------------------------------------------------------------------------------------------

def create_pyramid(image, levels):
    """ImagePyramid::CreateImagePyramid: level i+1 = (a+b+c+d) >> 2 over 2x2 blocks, rows/2 x cols/2; level 0 is the image."""
    out = [np.ascontiguousarray(image, dtype=np.uint8)]
    for _ in range(1, levels):
        p = out[-1].astype(np.int32)
        r, c = p.shape[0] // 2, p.shape[1] // 2
        p = p[:2 * r, :2 * c]
        out.append(((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) >> 2).astype(np.uint8))
    return out


def _to_int32(x):
    """static_cast<int32_t>(float): truncation; NaN / out of range give INT32_MIN (x86-64 cvttss2si)."""
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x) & (x > -2147483649.0) & (x < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), _INT32_MIN).astype(np.int64)


def _wrap32(x):
    return ((np.asarray(x, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


class _Image:
    def __init__(self, img):
        img = np.asarray(img, np.uint8)
        self.rows, self.cols = img.shape
        self.flat = img.astype(np.float64).ravel()

    def bilinear(self, r0, c0, sr, sc, fl):
        """Value at base index (r0, c0) (int arrays, already inside) with fractions (sr, sc): weights (1-sr)(1-sc), (1-sr)sc,
        sr(1-sc), sr sc; the +1 neighbours clamped (their weight is 0 there)."""
        if fl.swap_sr_sc:
            sr, sc = sc, sr
        i00 = r0 * self.cols + c0
        i01 = i00 + (c0 + 1 < self.cols)
        down = np.where(r0 + 1 < self.rows, self.cols, 0)
        f = self.flat
        wr, wc = 1.0 - sr, 1.0 - sc
        return ((wr * wc * f.take(i00) + wr * sc * f.take(i01)) + sr * wc * f.take(i00 + down)) + sr * sc * f.take(i01 + down)

    def get(self, r, c, fl, edge=True):
        """GrayImage::GetPixelValue(row, col) at float32 coordinates: (value, valid, distance to the validity edge or None)."""
        r = np.asarray(r, np.float64)
        c = np.asarray(c, np.float64)
        R, C = self.rows - 1, self.cols - 1
        with np.errstate(invalid="ignore"):
            r_in, c_in = (r >= 0) & (r <= R), (c >= 0) & (c <= C)
            if fl.validity_strict:
                valid = (r >= 0) & (r < R) & (c >= 0) & (c < C)
            else:
                valid = r_in & c_in
        rr = np.where(valid, r, 0.0)
        cc = np.where(valid, c, 0.0)
        fr, fc = np.floor(rr), np.floor(cc)
        val = self.bilinear(fr.astype(np.int64), fc.astype(np.int64), rr - fr, cc - fc, fl)
        val[~valid] = 0.0
        if not edge:
            return val, valid, None
        with np.errstate(invalid="ignore"):
            # a coordinate's edge matters only while the other coordinate is in range
            e = np.minimum(np.where(c_in, np.minimum(np.abs(r), np.abs(r - R)), np.inf),
                           np.where(r_in, np.minimum(np.abs(c), np.abs(c - C)), np.inf))
        return val, valid, np.where(np.isnan(e), np.inf, e)

    def get_nocheck(self, r, c, fl):
        """GetPixelValueNoCheck(float, float): the same formula, base index clamped into the image."""
        r = np.asarray(r, np.float64)
        c = np.asarray(c, np.float64)
        fin = np.isfinite(r) & np.isfinite(c)
        rr, cc = np.where(fin, r, 0.0), np.where(fin, c, 0.0)
        fr = np.clip(np.floor(rr), -1e9, 1e9)
        fc = np.clip(np.floor(cc), -1e9, 1e9)
        r0 = np.clip(fr, 0, self.rows - 1).astype(np.int64)
        c0 = np.clip(fc, 0, self.cols - 1).astype(np.int64)
        return self.bilinear(r0, c0, rr - fr, cc - fc, fl)


def _lattice_edge(pos, k, n):
    """Integer-lattice validity (0 <= floor(pos) + k <= n - 2) flips where pos + k crosses 0 or n - 1."""
    x = pos[:, None] + k[None, :]
    return np.minimum(np.abs(x), np.abs(x - (n - 1))).min(axis=1)


# ---- per-feature result ---------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Result:
    ok: bool
    uv: np.ndarray          # (n, 2) float64
    status: np.ndarray      # (n,) uint8
    iters: np.ndarray       # (n,) uint32, summed over levels
    m_converge: np.ndarray
    m_large: np.ndarray
    m_outside: np.ndarray
    m_edge: np.ndarray
    cond: np.ndarray
    cond_raw: np.ndarray
    singular: np.ndarray
    min_valid: np.ndarray   # fewest valid pixels of any solved system
    capped: np.ndarray      # some level ran out of iterations without a stopping decision: the position is not a fixed point

    def comparable(self, cond_max=1e4):
        return (~self.singular) & (self.cond <= cond_max) & (self.min_valid >= 1)

    def away(self, rel=1e-3, px=1e-3, edge_px=1e-3):
        """Features whose every decision lies outside the band: relative `rel` of each threshold, `px` from the outside bounds,
        `edge_px` from validity edges."""
        return (self.m_converge > rel) & (self.m_large > rel) & (self.m_outside > px) & (self.m_edge > edge_px)


class _State:
    def __init__(self, n, cur_uv, status):
        self.uv = np.asarray(cur_uv, np.float64).copy()
        self.status = np.asarray(status, np.uint8).copy()
        self.iters = np.zeros(n, np.uint32)
        self.A = np.tile(np.eye(2), (n, 1, 1))
        self.R = np.tile(np.eye(2), (n, 1, 1))
        self.t = np.zeros((n, 2))
        inf = np.full(n, np.inf)
        self.m_converge, self.m_large, self.m_outside, self.m_edge = inf.copy(), inf.copy(), inf.copy(), inf.copy()
        self.cond = np.zeros(n)
        self.cond_raw = np.zeros(n)
        self.singular = np.zeros(n, bool)
        self.min_valid = np.full(n, np.iinfo(np.int64).max)
        self.capped = np.zeros(n, bool)

    def result(self, ok):
        return Result(ok, self.uv, self.status, self.iters, self.m_converge, self.m_large, self.m_outside, self.m_edge, self.cond,
                      self.cond_raw, self.singular, self.min_valid, self.capped)


@dataclasses.dataclass(frozen=True)
class Options:  # optical_flow.h:20-28
    kMaxTrackPointsNumber: int = 500
    kMaxIteration: int = 15
    kMaxToleranceLargeStep: int = 3
    kPatchRowHalfSize: int = 6
    kPatchColHalfSize: int = 6
    kMaxConvergeStep: float = 4e-2


def _normal(J, r, w):
    """H = sum J^T J, b = -sum J^T r over the valid pixels w, and the same sums of |term| (for the conditioning report)."""
    k = len(J)
    m = J[0].shape[0]
    H, Ha = np.zeros((m, k, k)), np.zeros((m, k, k))
    for i in range(k):
        for j in range(i, k):
            t = np.where(w, J[i] * J[j], 0.0)
            H[:, i, j] = H[:, j, i] = t.sum(axis=1)
            Ha[:, i, j] = Ha[:, j, i] = np.abs(t).sum(axis=1)
    t = [np.where(w, J[i] * r, 0.0) for i in range(k)]
    return H, -np.stack([a.sum(axis=1) for a in t], -1), Ha, np.stack([np.abs(a).sum(axis=1) for a in t], -1)


def _eye_map(m, k):
    return lambda x, sel: np.tile(np.eye(k), (len(x), 1, 1))


def _solve(st, ids, H, b, M, Ha, ba):
    """numpy.linalg.solve in float64; singular systems (rank-deficient, all zero) by pseudo-inverse and flagged.

    Conditioning (`cond`): Skeel's componentwise condition number of the new POSITION against relative perturbations of every
    term of every sum, in px: || |M H^-1| (Ha |x| + ba) ||_inf / 1 px, where Ha, ba are the sums of |term| and M(x) is the
    Jacobian of the position update at the solution.  To first order a float32 implementation that rounds its sums moves the
    position by about eps32 (6e-8) x a small multiple x cond px: cond <= 1e4 bounds that spread near 1e-3 px."""
    m, k = b.shape
    fin = np.isfinite(H).all(axis=(1, 2)) & np.isfinite(b).all(axis=1)
    x = np.full((m, k), np.nan)
    if fin.any():
        Hf, bf = H[fin], b[fin]
        sv = np.linalg.svd(Hf, compute_uv=False)
        with np.errstate(divide="ignore", invalid="ignore"):
            raw = np.where(sv[:, 0] > 0, sv[:, 0] / sv[:, -1], np.inf)
        sing = ~(raw < 1e13)
        xs = np.empty_like(bf)
        cs = np.full(len(bf), np.inf)
        ok = ~sing
        if ok.any():
            Hi = np.linalg.inv(Hf[ok])
            xs[ok] = np.linalg.solve(Hf[ok], bf[ok][..., None])[..., 0]
            sel = np.nonzero(fin)[0][ok]
            Mf = M(xs[ok], sel)
            S = np.abs(Mf @ Hi)
            pert = np.einsum("nij,nj->ni", Ha[fin][ok], np.abs(xs[ok])) + ba[fin][ok]
            cs[ok] = np.einsum("nij,nj->ni", S, pert).max(axis=1)
        if sing.any():
            xs[sing] = (np.linalg.pinv(Hf[sing]) @ bf[sing][..., None])[..., 0]
        x[fin] = xs
        g = ids[fin]
        st.cond[g] = np.maximum(st.cond[g], cs)
        st.cond_raw[g] = np.maximum(st.cond_raw[g], raw)
        st.singular[g] |= sing
    return x


def _note(arr, ids, vals):
    np.minimum.at(arr, ids, vals)


def _offsets(o):
    hr, hc = o.kPatchRowHalfSize, o.kPatchColHalfSize
    drow, dcol = np.meshgrid(np.arange(-hr, hr + 1), np.arange(-hc, hc + 1), indexing="ij")
    return drow.ravel(), dcol.ravel()


# ---- the reference's extended patch (optical_flow.cpp:49-102) and fast pre-computation ---------------------------------------

def _ex_patch(img, ref32, o, fl):
    """ExtractExtendPatchInReferenceImage on the integer lattice floor(ref) - ex/2 + k with ref's own bilinear fractions; valid iff
    0 <= row <= rows-2 and 0 <= col <= cols-2.  Returns values (m, EXR*EXC), valid, valid count."""
    exr, exc = 2 * o.kPatchRowHalfSize + 3, 2 * o.kPatchColHalfSize + 3
    fy, fx = np.floor(ref32[:, 1]), np.floor(ref32[:, 0])
    sr = ref32[:, 1].astype(np.float64) - fy
    sc = ref32[:, 0].astype(np.float64) - fx
    r0 = _wrap32(_to_int32(fy) - exr // 2 + fl.ex_patch_offset)
    c0 = _wrap32(_to_int32(fx) - exc // 2 + fl.ex_patch_offset)
    rows = _wrap32(r0[:, None] + np.arange(exr)[None, :])
    cols = _wrap32(c0[:, None] + np.arange(exc)[None, :])
    R = np.repeat(rows, exc, axis=1)
    C = np.tile(cols, (1, exr))
    valid = (R >= 0) & (R <= img.rows - 2) & (C >= 0) & (C <= img.cols - 2)
    val = img.bilinear(np.where(valid, R, 0), np.where(valid, C, 0), np.where(valid, sr[:, None], 0.0), np.where(valid, sc[:, None], 0.0), fl)
    return np.where(valid, val, 0.0), valid, valid.sum(axis=1)


def _ex_gradient(ex, exv, o):
    """PrecomputeJacobian*: central differences at the patch's pixels (ex index (row+1, col+1)); 0 unless all four neighbours are
    valid (basic_klt_fast.cpp:64-99)."""
    exr, exc = 2 * o.kPatchRowHalfSize + 3, 2 * o.kPatchColHalfSize + 3
    pr, pc = exr - 2, exc - 2
    e = ex.reshape(-1, exr, exc)
    v = exv.reshape(-1, exr, exc)
    ok = v[:, 1:-1, :-2] & v[:, 1:-1, 2:] & v[:, :-2, 1:-1] & v[:, 2:, 1:-1]
    dx = np.where(ok, e[:, 1:-1, 2:] - e[:, 1:-1, :-2], 0.0).reshape(-1, pr * pc)
    dy = np.where(ok, e[:, 2:, 1:-1] - e[:, :-2, 1:-1], 0.0).reshape(-1, pr * pc)
    center = v[:, 1:-1, 1:-1].reshape(-1, pr * pc)
    return dx, dy, e[:, 1:-1, 1:-1].reshape(-1, pr * pc), center


# ---- one level of one variant ----------------------------------------------------------------------------------------------

class _Level:
    def __init__(self, model, method, o, fl, refI, curI, exact_first, luminance, half_grad):
        self.model, self.method, self.o, self.fl = model, method, o, fl
        self.refI, self.curI = refI, curI
        self.exact_first = exact_first  # sample coordinates of iteration 0 come from the inputs alone
        self.luminance = luminance
        self.g = 1.0 if half_grad else 0.5
        self.drow, self.dcol = _offsets(o)
        self.thr = float(f32(o.kMaxConvergeStep))
        self._ref_cache = {}  # reference-image samples: the same in every iteration of the level

    # sample coordinates, float32 -------------------------------------------------------------------------------------------
    def _ref_coords(self, ref32):
        return f32(self.drow)[None, :] + ref32[:, 1:2], f32(self.dcol)[None, :] + ref32[:, 0:1]

    def _cur_coords_translation(self, cur32):
        drow = f32(self.drow + self.fl.cur_lattice_row_shift)
        return drow[None, :] + cur32[:, 1:2], f32(self.dcol)[None, :] + cur32[:, 0:1]

    def _cur_coords_affine(self, A32, cur32):  # affine * Vec2(dcol, drow) + cur (affine_klt.cpp:145-147)
        dc = f32(self.dcol)[None, :]
        dr = f32(self.drow + self.fl.cur_lattice_row_shift)[None, :]
        x = A32[:, 0, 0:1] * dc + A32[:, 0, 1:2] * dr
        y = A32[:, 1, 0:1] * dc + A32[:, 1, 1:2] * dr
        return y + cur32[:, 1:2], x + cur32[:, 0:1]

    def _cur_coords_se2(self, R32, t32, ri, ci):  # R_cr * Vec2(col_i, row_i) + t_cr (lssd_klt.cpp:146-148)
        ri = ri + f32(self.fl.cur_lattice_row_shift)
        x = (R32[:, 0, 0:1] * ci + R32[:, 0, 1:2] * ri) + t32[:, 0:1]
        y = (R32[:, 1, 0:1] * ci + R32[:, 1, 1:2] * ri) + t32[:, 1:2]
        return y, x

    def _ref_get(self, key, ids, r, c):
        """refI.get at coordinates formed from the reference position alone, computed once per level: the first iteration
        samples every feature of the level, later ones a subset of them in the same (ascending) order."""
        hit = self._ref_cache.get(key)
        if hit is None:
            val, v, _ = self.refI.get(r, c, self.fl, False)
            self._ref_cache[key] = (ids.copy(), val, v)
            return val, v
        ids0, val, v = hit
        rows = np.minimum(np.searchsorted(ids0, ids), len(ids0) - 1)
        assert (ids0[rows] == ids).all()
        return val[rows], v[rows]

    def _grad6(self, ids, gimg, gr, gc, r4, c4, r5, c5, note):
        """The six GetPixelValue calls of every non-fast variant: left, right, top, bottom on the gradient image, then ref and cur."""
        one = f32(1.0)
        # ref-side samples never move; only the current-image side is formed from a computed position
        ge = bool(note) and gimg is self.curI
        if gimg is self.refI:
            (t0, v0), (t1, v1) = self._ref_get(0, ids, gr, gc - one), self._ref_get(1, ids, gr, gc + one)
            (t2, v2), (t3, v3) = self._ref_get(2, ids, gr - one, gc), self._ref_get(3, ids, gr + one, gc)
        else:
            t0, v0, e0 = gimg.get(gr, gc - one, self.fl, ge)
            t1, v1, e1 = gimg.get(gr, gc + one, self.fl, ge)
            t2, v2, e2 = gimg.get(gr - one, gc, self.fl, ge)
            t3, v3, e3 = gimg.get(gr + one, gc, self.fl, ge)
        t4, v4 = self._ref_get(4, ids, r4, c4)
        t5, v5, e5 = self.curI.get(r5, c5, self.fl, bool(note))
        valid = v0 & v1 & v2 & v3 & v4 & v5
        if note:
            es = [e5] + ([e0, e1, e2, e3] if ge else [])
            note(np.min(np.stack(es).min(axis=0), axis=1))
        return (t1 - t0) * self.g, (t3 - t2) * self.g, t4, t5, valid

    def _gradient_image(self, rr, rc, cr, cc):
        use_cur = (self.method == "direct") != self.fl.gradient_other_image
        return (self.curI, cr, cc) if use_cur else (self.refI, rr, rc)

    # normal equations ---------------------------------------------------------------------------------------------------------
    def build(self, st, ids, ref32, it, pre):
        note = None
        if not (it == 0 and self.exact_first):
            def note(e):
                _note(st.m_edge, ids, e)
        if self.method == "fast":
            return getattr(self, "_build_fast_" + self.model)(st, ids, ref32, pre, note)
        return getattr(self, "_build_" + self.model)(st, ids, ref32, note)

    def _build_basic(self, st, ids, ref32, note):  # basic_klt.cpp:118-181
        ri, ci = self._ref_coords(ref32)
        rj, cj = self._cur_coords_translation(st.uv[ids].astype(f32))
        gimg, gr, gc = self._gradient_image(ri, ci, rj, cj)
        fx, fy, t4, t5, valid = self._grad6(ids, gimg, gr, gc, ri, ci, rj, cj, note)
        ft = t5 - t4
        H, b, Ha, ba = _normal([fx, fy], ft, valid)
        return H, b, valid.sum(axis=1), _eye_map(len(ids), 2), Ha, ba

    def _affine_H(self, x, y, dx, dy, w):
        """The 21 sums of affine_klt.cpp:167-187 (and |term| sums, for the conditioning report)."""
        xx, yy, xy = x * x, y * y, x * y
        dxdx, dydy, dxdy = dx * dx, dy * dy, dx * dy
        s = lambda a: np.where(w, a, 0.0).sum(axis=1)
        sa = lambda a: np.where(w, np.abs(a), 0.0).sum(axis=1)
        H = np.zeros((x.shape[0], 6, 6))
        Ha = np.zeros_like(H)
        terms = {(0, 0): xx * dxdx, (0, 1): xx * dxdy, (0, 2): xy * dxdx, (0, 3): xy * dxdy, (0, 4): x * dxdx, (0, 5): x * dxdy,
                 (1, 1): xx * dydy, (1, 2): xy * dxdy, (1, 3): xy * dydy, (1, 4): x * dxdy, (1, 5): x * dydy,
                 (2, 2): yy * dxdx, (2, 3): yy * dxdy, (2, 4): y * dxdx, (2, 5): y * dxdy,
                 (3, 3): yy * dydy, (3, 4): (yy if self.fl.affine_h34_yy else y) * dxdy, (3, 5): y * dydy,
                 (4, 4): dxdx, (4, 5): dxdy, (5, 5): dydy}
        for (i, j), a in terms.items():
            H[:, i, j] = H[:, j, i] = s(a)
            Ha[:, i, j] = Ha[:, j, i] = sa(a)
        return H, Ha

    @staticmethod
    def _affine_map(cur):  # v = z.head<2>() * x + z.segment<2>(2) * y + z.tail<2>() (affine_klt.cpp:104)
        M = np.zeros((cur.shape[0], 2, 6))
        M[:, 0, 0] = M[:, 1, 1] = cur[:, 0]
        M[:, 0, 2] = M[:, 1, 3] = cur[:, 1]
        M[:, 0, 4] = M[:, 1, 5] = 1.0
        return lambda x, sel: M[sel]

    @staticmethod
    def _affine_b(dt, x, y, dx, dy, w):
        terms = [dt * x * dx, dt * x * dy, dt * y * dx, dt * y * dy, dt * dx, dt * dy]
        b = -np.stack([np.where(w, a, 0.0).sum(axis=1) for a in terms], -1)
        ba = np.stack([np.where(w, np.abs(a), 0.0).sum(axis=1) for a in terms], -1)
        return b, ba

    def _build_affine(self, st, ids, ref32, note):  # affine_klt.cpp:131-273
        ri, ci = self._ref_coords(ref32)
        rj, cj = self._cur_coords_affine(st.A[ids].astype(f32), st.uv[ids].astype(f32))
        gimg, gr, gc = self._gradient_image(ri, ci, rj, cj)
        dx, dy, t4, t5, valid = self._grad6(ids, gimg, gr, gc, ri, ci, rj, cj, note)
        dt = t5 - t4
        x, y = cj.astype(np.float64), rj.astype(np.float64)
        H, Ha = self._affine_H(x, y, dx, dy, valid)
        b, ba = self._affine_b(dt, x, y, dx, dy, valid)
        return H, b, valid.sum(axis=1), self._affine_map(st.uv[ids]), Ha, ba

    @staticmethod
    def _se2_map(R, ref):
        """The Jacobian, at the solution x, of the position R' ref + t' after R' = R [1 -w; w 1] / |col 0|, t' = t + (v1, v2)
        (lssd_klt.cpp:114-117); d/dw by a central difference (the step in w is not small on features that diverge)."""
        def rotated(w):
            A = np.zeros((len(w), 2, 2))
            A[:, 0, 0] = A[:, 1, 1] = 1.0
            A[:, 0, 1], A[:, 1, 0] = -w, w
            Rn = R_sel @ A
            Rn /= np.linalg.norm(Rn[:, :, 0], axis=1)[:, None, None]
            return np.einsum("nij,nj->ni", Rn, ref_sel)

        def M(x, sel):
            nonlocal R_sel, ref_sel
            R_sel, ref_sel = R[sel], ref[sel]
            w = x[:, 0]
            h = 1e-6 * np.maximum(1.0, np.abs(w))
            out = np.zeros((len(w), 2, 3))
            out[:, :, 0] = (rotated(w + h) - rotated(w - h)) / (2 * h)[:, None]
            out[:, 0, 1] = out[:, 1, 2] = 1.0
            return out
        R_sel = ref_sel = None
        return M

    def _se2_normal(self, R, ri, ci, jx, jy, res, w):
        """jacobian = [jp . R(-row_i, col_i), jp]; H += J^T J, b -= J^T r (lssd_klt.cpp:209-215)."""
        ri, ci = ri.astype(np.float64), ci.astype(np.float64)
        gx = R[:, 0, 0:1] * -ri + R[:, 0, 1:2] * ci
        gy = R[:, 1, 0:1] * -ri + R[:, 1, 1:2] * ci
        return _normal([jx * gx + jy * gy, jx, jy], res, w)

    def _build_lssd(self, st, ids, ref32, note):  # lssd_klt.cpp:127-250
        R = st.R[ids]
        ri, ci = self._ref_coords(ref32)
        rj, cj = self._cur_coords_se2(R.astype(f32), st.t[ids].astype(f32), ri, ci)
        gimg, gr, gc = self._gradient_image(ri, ci, rj, cj)
        jx, jy, t4, t5, valid = self._grad6(ids, gimg, gr, gc, ri, ci, rj, cj, note)
        n = valid.sum(axis=1)
        if self.fl.lssd_mean_normalise:
            with np.errstate(divide="ignore", invalid="ignore"):
                ref_avg = np.where(valid, t4, 0.0).sum(axis=1) / n
                cur_avg = np.where(valid, t5, 0.0).sum(axis=1) / n
        else:
            ref_avg = cur_avg = np.ones(len(ids))
        norm = cur_avg if self.method == "direct" else ref_avg
        with np.errstate(divide="ignore", invalid="ignore"):
            jx, jy = jx / norm[:, None], jy / norm[:, None]
            res = t5 / cur_avg[:, None] - t4 / ref_avg[:, None]
        H, b, Ha, ba = self._se2_normal(R, ri, ci, jx, jy, res, valid)
        return H, b, n, self._se2_map(R, ref32.astype(np.float64)), Ha, ba

    # fast: per-level pre-computation and per-iteration bias ------------------------------------------------------------------
    def prepare_fast(self, st, ids, ref32):
        ex, exv, nvalid = _ex_patch(self.refI, ref32, self.o, self.fl)
        dx, dy, ref_px, ref_ok = _ex_gradient(ex, exv, self.o)
        pre = dict(dx=dx * self.g, dy=dy * self.g, ref=ref_px, ref_ok=ref_ok)
        if self.model == "basic":
            pre["H"], _, pre["Ha"], _ = _normal([pre["dx"], pre["dy"]], np.zeros_like(dx), np.ones(dx.shape, bool))
        elif self.model == "affine":  # affine_klt_fast.cpp:71-138, x from the level's starting cur position
            cur32 = st.uv[ids].astype(f32)
            pr, pc = 2 * self.o.kPatchRowHalfSize + 1, 2 * self.o.kPatchColHalfSize + 1
            rr, cc = np.meshgrid(np.arange(pr) - self.o.kPatchRowHalfSize, np.arange(pc) - self.o.kPatchColHalfSize, indexing="ij")
            x = (f32(cc.ravel())[None, :] + cur32[:, 0:1]).astype(np.float64)
            y = (f32(rr.ravel())[None, :] + cur32[:, 1:2]).astype(np.float64)
            H, Ha = self._affine_H(x, y, pre["dx"], pre["dy"], _ex_gradient_valid(exv, self.o))
            for X in (H, Ha):
                X[:, 1, 2] = X[:, 2, 1] = X[:, 0, 3]
                X[:, 1, 4] = X[:, 4, 1] = X[:, 0, 5]
                if self.fl.affine_h34_yy:
                    X[:, 3, 4] = X[:, 4, 3] = X[:, 2, 3]
            pre["H"], pre["Ha"] = H, Ha
        elif self.luminance:  # lssd_klt_fast.cpp:27-46
            if self.fl.lssd_fast_luminance_mismatch:
                avg = ref_px.sum(axis=1) / nvalid
            else:
                avg = np.where(ref_ok, ref_px, 0.0).sum(axis=1) / np.maximum(ref_ok.sum(axis=1), 1)
            for k in ("dx", "dy", "ref"):
                pre[k] = pre[k] / avg[:, None]
        return nvalid, pre

    def _build_fast_basic(self, st, ids, ref32, pre, note):  # basic_klt_fast.cpp:101-195
        o, img = self.o, self.curI
        cur = st.uv[ids]
        cur32 = cur.astype(f32)
        fy, fx = np.floor(cur32[:, 1]), np.floor(cur32[:, 0])
        sr, sc = cur[:, 1] - fy, cur[:, 0] - fx
        hr, hc = o.kPatchRowHalfSize, o.kPatchColHalfSize
        kr = np.arange(-hr, hr + 1) + self.fl.cur_lattice_row_shift
        kc = np.arange(-hc, hc + 1)
        rows = _wrap32(_to_int32(fy)[:, None] + kr[None, :])
        cols = _wrap32(_to_int32(fx)[:, None] + kc[None, :])
        R = np.repeat(rows, len(kc), axis=1)
        C = np.tile(cols, (1, len(kr)))
        valid = (R >= 0) & (R <= img.rows - 2) & (C >= 0) & (C <= img.cols - 2) & pre["ref_ok"]
        if note:
            note(np.minimum(_lattice_edge(cur[:, 1], kr, img.rows), _lattice_edge(cur[:, 0], kc, img.cols)))
        val = img.bilinear(np.where(valid, R, 0), np.where(valid, C, 0), sr[:, None], sc[:, None], self.fl)
        dt = val - pre["ref"]
        _, b, _, ba = _normal([pre["dx"], pre["dy"]], dt, valid)
        return pre["H"], b, valid.sum(axis=1), _eye_map(len(ids), 2), pre["Ha"], ba

    def _build_fast_affine(self, st, ids, ref32, pre, note):  # affine_klt_fast.cpp:140-188
        rj, cj = self._cur_coords_affine(st.A[ids].astype(f32), st.uv[ids].astype(f32))
        val, v, e = self.curI.get(rj, cj, self.fl, bool(note))
        if note:
            note(e.min(axis=1))
        valid = v & pre["ref_ok"]
        dt = val - pre["ref"]
        x, y = cj.astype(np.float64), rj.astype(np.float64)
        b, ba = self._affine_b(dt, x, y, pre["dx"], pre["dy"], valid)
        return pre["H"], b, valid.sum(axis=1), self._affine_map(st.uv[ids]), pre["Ha"], ba

    def _build_fast_lssd(self, st, ids, ref32, pre, note):  # lssd_klt_fast.cpp:56-85, 145-229
        o, img = self.o, self.curI
        R, t = st.R[ids], st.t[ids]
        R32, t32 = R.astype(f32), t.astype(f32)
        # ExtractPatchInCurrentImage: the "inside" test on a window of +-patch size around R ref + t
        cx = (R32[:, 0, 0] * ref32[:, 0] + R32[:, 0, 1] * ref32[:, 1]) + t32[:, 0]
        cy = (R32[:, 1, 0] * ref32[:, 0] + R32[:, 1, 1] * ref32[:, 1]) + t32[:, 1]
        pr, pc = 2 * o.kPatchRowHalfSize + 1, 2 * o.kPatchColHalfSize + 1
        r0 = _wrap32(_to_int32(cy) - pr)
        c0 = _wrap32(_to_int32(cx) - pc)
        inside = (r0 >= 0) & (_wrap32(r0 + 2 * pr) <= img.rows - 2) & (c0 >= 0) & (_wrap32(c0 + 2 * pc) <= img.cols - 2)
        ri, ci = self._ref_coords(ref32)
        rj, cj = self._cur_coords_se2(R32, t32, ri, ci)
        val, v, e = img.get(rj, cj, self.fl, bool(note))
        if note:
            note(e.min(axis=1))
        cur_ok = v | inside[:, None]
        cur = np.where(v, val, np.where(inside[:, None], img.get_nocheck(rj, cj, self.fl), 0.0))
        n_cur = cur_ok.sum(axis=1)
        if self.luminance:
            with np.errstate(divide="ignore", invalid="ignore"):
                if self.fl.lssd_fast_luminance_mismatch:
                    num = cur.reshape(-1, pr, pc)[:, 1:-1, 1:-1].reshape(len(ids), -1).sum(axis=1)
                    avg = num / n_cur
                else:
                    avg = np.where(cur_ok, cur, 0.0).sum(axis=1) / np.maximum(n_cur, 1)
                cur = cur / avg[:, None]
        valid = pre["ref_ok"] & cur_ok
        res = cur - pre["ref"]
        H, b, Ha, ba = self._se2_normal(R, ri, ci, pre["dx"], pre["dy"], res, valid)
        # a patch without a valid current pixel stops before the normal equations (lssd_klt_fast.cpp:62)
        n = np.where(n_cur == 0, 0, valid.sum(axis=1))
        return H, b, n, self._se2_map(R, ref32.astype(np.float64)), Ha, ba

    # the iteration ------------------------------------------------------------------------------------------------------------
    def run(self, st, ids, ref32):
        o, fl = self.o, self.fl
        fast = self.method == "fast"
        pre = None
        if fast:
            nvalid, pre = self.prepare_fast(st, ids, ref32)
            none = nvalid == 0
            st.status[ids[none]] = OUTSIDE
            keep = ~none
            ids, ref32 = ids[keep], ref32[keep]
            pre = {k: v[keep] for k, v in pre.items()}
            if fl.fast_status_reset:
                st.status[ids] = LARGE_RESIDUAL
            last = np.full(len(ids), np.inf)
            large = np.zeros(len(ids), np.int64)
        for it in range(o.kMaxIteration):
            if len(ids) == 0:
                break
            st.iters[ids] += 1
            with np.errstate(invalid="ignore", over="ignore"):
                H, b, n, M, Ha, ba = self.build(st, ids, ref32, it, pre)
            go = n > 0
            ids, ref32, H, b, n, Ha, ba = ids[go], ref32[go], H[go], b[go], n[go], Ha[go], ba[go]
            M = functools.partial(lambda M0, rows, x, sel: M0(x, rows[sel]), M, np.nonzero(go)[0])
            if fast:
                pre = {k: v[go] for k, v in pre.items()}
                last, large = last[go], large[go]
            if len(ids) == 0:
                break
            np.minimum.at(st.min_valid, ids, n)
            x = _solve(st, ids, H, b, M, Ha, ba)
            if self.model == "basic":
                v = x
                nan = np.isnan(v).any(axis=1)
            elif self.model == "affine":
                cur = st.uv[ids]
                v = x[:, 0:2] * cur[:, 0:1] + x[:, 2:4] * cur[:, 1:2] + x[:, 4:6]
                nan = np.isnan(x).any(axis=1) if fast else np.isnan(v).any(axis=1)
            else:
                v = x
                nan = np.isnan(v).any(axis=1)
            st.status[ids[nan]] = NUMERIC_ERROR
            ok = ~nan
            ids, ref32, x, v = ids[ok], ref32[ok], x[ok], v[ok]
            if fast:
                pre = {k: a[ok] for k, a in pre.items()}
                last, large = last[ok], large[ok]
            if self.model == "lssd":
                dR = np.zeros((len(ids), 2, 2))
                dR[:, 0, 0] = dR[:, 1, 1] = 1.0
                dR[:, 0, 1], dR[:, 1, 0] = -x[:, 0], x[:, 0]
                R = st.R[ids] @ dR
                st.R[ids] = R / np.linalg.norm(R[:, :, 0], axis=1)[:, None, None]
                st.t[ids] += x[:, 1:3]
            else:
                st.uv[ids] += v
                if self.model == "affine":
                    st.A[ids, :, 0] += x[:, 0:2]
                    st.A[ids, :, 1] += x[:, 2:4]
            stop = np.zeros(len(ids), bool)
            if not fast and self.model != "lssd":  # basic_klt.cpp:107-110
                u = st.uv[ids]
                out = (u[:, 0] < 0) | (u[:, 0] > self.curI.cols - 1) | (u[:, 1] < 0) | (u[:, 1] > self.curI.rows - 1)
                _note(st.m_outside, ids, _outside_margin(u, self.curI))
                st.status[ids[out]] = OUTSIDE
                stop |= out
            sq = (v * v).sum(axis=1)
            if fast:  # basic_klt_fast.cpp:48-60
                act = ~stop
                with np.errstate(invalid="ignore"):
                    rel = np.where(np.isfinite(last), np.abs(sq - last) / np.where(last > 0, last, np.inf), np.inf)
                _note(st.m_large, ids[act], rel[act])
                smaller = sq < last
                last = np.where(smaller, sq, last)
                large = np.where(smaller, 0, large + 1)
                stop |= (~smaller) & (large >= o.kMaxToleranceLargeStep)
            act = ~stop
            _note(st.m_converge, ids[act], np.abs(sq[act] - self.thr) / self.thr)
            conv = act & (sq < self.thr)
            st.status[ids[conv]] = TRACKED
            stop |= conv
            keep = ~stop
            ids, ref32 = ids[keep], ref32[keep]
            if fast:
                pre = {k: a[keep] for k, a in pre.items()}
                last, large = last[keep], large[keep]
        else:
            st.capped[ids] = True


def _ex_gradient_valid(exv, o):
    exr, exc = 2 * o.kPatchRowHalfSize + 3, 2 * o.kPatchColHalfSize + 3
    v = exv.reshape(-1, exr, exc)
    return (v[:, 1:-1, :-2] & v[:, 1:-1, 2:] & v[:, :-2, 1:-1] & v[:, 2:, 1:-1]).reshape(v.shape[0], -1)


def _outside_margin(u, img):
    return np.minimum(np.minimum(np.abs(u[:, 0]), np.abs(u[:, 0] - (img.cols - 1))), np.minimum(np.abs(u[:, 1]), np.abs(u[:, 1] - (img.rows - 1))))


# ---- the two TrackFeatures overloads (optical_flow.cpp:6-47, *_klt.cpp TrackMultipleLevel / TrackSingleLevel) ----------------

def _prepare(ref_uv, cur_uv, status):
    ref = np.asarray(ref_uv, np.float32).reshape(-1, 2)
    n = ref.shape[0]
    cur = ref if cur_uv is None or np.asarray(cur_uv).reshape(-1, 2).shape[0] != n else np.asarray(cur_uv, np.float32).reshape(-1, 2)
    st = np.zeros(n, np.uint8) if status is None or np.asarray(status).size != n else np.asarray(status, np.uint8)
    return ref, cur.astype(np.float64), st, n


def _options(half, half_cols, max_points, max_iteration, max_large_step, converge):
    return Options(max_points, max_iteration, max_large_step, half, half if half_cols is None else half_cols, converge)


def _todo(state, n, o, fl):
    ids = np.arange(min(n, o.kMaxTrackPointsNumber))
    if fl.skip_incoming_failed:
        ids = ids[state.status[ids] <= TRACKED]
    return ids


def track_pyramid(model, method, ref_levels, cur_levels, ref_uv, cur_uv=None, status=None, *, half=6, half_cols=None, max_points=500,
                  max_iteration=15, max_large_step=3, converge=4e-2, prior=None, luminance=False, flags=DEFAULT):
    """TrackFeatures(ref_pyramid, cur_pyramid, ...): returns a Result."""
    ref, cur, status, n = _prepare(ref_uv, cur_uv, status)
    st = _State(n, cur, status)
    if n == 0 or len(ref_levels) != len(cur_levels):
        return st.result(False)
    o = _options(half, half_cols, max_points, max_iteration, max_large_step, converge)
    L = len(ref_levels)
    refs = [_Image(i) for i in ref_levels]
    curs = [_Image(i) for i in cur_levels]
    ids = _todo(st, n, o, flags)
    scale = f32(1 << (L - 1))
    sref = ref[ids] / scale  # exact: a power of two
    P = np.eye(2) if prior is None else np.asarray(prior, np.float32).astype(np.float64).reshape(2, 2)
    if model == "affine" and not flags.affine_pyramid_identity:
        st.A[ids] = P
    if model == "lssd":  # lssd_klt.cpp:22-23
        st.R[ids] = P
        st.t[ids] = cur[ids] / float(scale) - sref.astype(np.float64) @ P.T
    else:
        st.uv[ids] = cur[ids] / float(scale)
    live = ids
    for lvl in range(L - 1, -1, -1):
        level = _Level(model, method, o, flags, refs[lvl], curs[lvl], lvl == L - 1 and (model != "lssd" or prior is None),
                       luminance, flags.no_half_gradient)
        if flags.failed_level_continues:
            run = np.ones(len(live), bool)
        else:
            run = np.isin(st.status[live], (NOT_TRACKED, TRACKED, LARGE_RESIDUAL)) | (lvl == L - 1)
        level.run(st, live[run], (sref * f32(2 ** (L - 1 - lvl)))[run].astype(f32))
        if lvl:
            if model == "lssd":
                st.t[live] *= 2.0
            else:
                st.uv[live] *= 2.0
    if model == "lssd":  # lssd_klt.cpp:43
        st.uv[ids] = np.einsum("nij,nj->ni", st.R[ids], ref[ids].astype(np.float64)) + st.t[ids]
    _final_outside(st, ids, curs[0])
    return st.result(True)


def track_single(model, method, ref_image, cur_image, ref_uv, cur_uv=None, status=None, *, half=6, half_cols=None, max_points=500,
                 max_iteration=15, max_large_step=3, converge=4e-2, prior=None, luminance=False, flags=DEFAULT):
    """TrackFeatures(ref_image, cur_image, ...): returns a Result."""
    ref, cur, status, n = _prepare(ref_uv, cur_uv, status)
    st = _State(n, cur, status)
    if n == 0:
        return st.result(False)
    o = _options(half, half_cols, max_points, max_iteration, max_large_step, converge)
    refI, curI = _Image(ref_image), _Image(cur_image)
    ids = _todo(st, n, o, flags)
    P = np.eye(2) if prior is None else np.asarray(prior, np.float32).astype(np.float64).reshape(2, 2)
    if model == "affine":
        st.A[ids] = P  # affine_klt.cpp:70
    if model == "lssd":  # lssd_klt.cpp:72-73
        st.R[ids] = P
        st.t[ids] = cur[ids] - ref[ids].astype(np.float64) @ P.T
    level = _Level(model, method, o, flags, refI, curI, model != "lssd" or prior is None, luminance, flags.no_half_gradient)
    level.run(st, ids, ref[ids])
    if model == "lssd" and not flags.lssd_single_no_writeback:
        st.uv[ids] = np.einsum("nij,nj->ni", st.R[ids], ref[ids].astype(np.float64)) + st.t[ids]
    _final_outside(st, ids, curI)
    return st.result(True)


def _final_outside(st, ids, img):
    u = st.uv[ids]
    with np.errstate(invalid="ignore"):
        out = (u[:, 0] < 0) | (u[:, 0] > img.cols - 1) | (u[:, 1] < 0) | (u[:, 1] > img.rows - 1)
    _note(st.m_outside, ids, np.where(np.isnan(_outside_margin(u, img)), np.inf, _outside_margin(u, img)))
    st.status[ids[out]] = OUTSIDE
