"""ref64 for DenseOpticalFlow (Farneback): a float64 restatement of the reference's dense_optical_flow.cpp / .h in whole-image
numpy operations.

TEST INFRASTRUCTURE ONLY.  Written from the reference's source (file:line below, all of dense_optical_flow.cpp unless a header is
named) and DESIGN.md section 2's substrate row for the un-vendored Utility::Interpolate (clamp-to-edge bilinear), independently of
tests/dense_flow_ref.c and of the kernels: it imports numpy and the standard library only and shares no line with
tests/dense_flow_ref.py or with the package.

Domain: finite inputs.  Everything is float64; the float32 expression order, the total-order median key, the x86 float-to-int cast
and the NaN conventions belong to the bit-exact contract that tests/test_dense_flow_gpu.py holds and are NOT restated here.  The
options' float thresholds are rounded to float32 once (they are `float` members, .h:18-19), so the decisions are taken against the
reference's numbers.

Stages (each usable on its own, which the staged checks of tests/test_dense_ref64_cpu.py need):
  gaussian(half, k)                        weights and (k2, k4, k22)                       :87-134
  moments(image, half, w)                  the six planes S0, Sr, Sc, Src, Srr, Scc        :136-189 (member order of .h:57-62)
  coefficients(S6, k)                      a00, a01, a11, b0, b1                           :247-303 / :305-332
  interpolate(M, r, c)                     Utility::Interpolate on one or several planes
  step(Sref, Scur, k, F, opt)              one capped Gauss-Newton update from the field F :194-238
  gauss_newton(Sref, Scur, k, F, opt, j)   the field BEFORE the median after j iterations  :200-242 (each pixel stops on its own)
  median3x3(P)                             SmoothFlow                                      :334-371
  upsample(F, shape)                       Interpolate(flow, r*0.5, c*0.5) * 2             :62-77
  track_image / track_pyramid              the two Track overloads                         :7-33 / :35-85

`Flags` carries the mutants: each switch introduces ONE plausible misreading of the source, so that a test can show that its
criterion fails on it.

`perturb=(seed, rel)` adds rel * U(-1, 1) * sum|term| to every moment value (sum|term| is the pixel's own sum of absolute terms):
a model of another, equally valid float32 accumulation of the moments.  The tests use it to find, from ref64 alone, the pixels whose
trajectory is not stable under rounding.
"""
from __future__ import annotations

import dataclasses

import numpy as np

f32 = np.float32
EPS = float(f32(1e-6))  # the 1e-6f of :287-302


@dataclasses.dataclass(frozen=True)
class Flags:
    """Mutants, each off by default."""
    a_avg_no_half: bool = False            # A_avg = A1 + A2 (:215)
    lambda_constant: float = 0.1           # another constant than 0.1 in lambda = 0.1 trace + 1 (:225)
    lambda_on_off_diagonal: bool = False   # H = MtM + lambda everywhere, not lambda I (:226)
    cap_per_component: bool = False        # each component clipped to +-kMaxDeltaFlowStep (:230-234)
    converge_before_update: bool = False   # the break taken before the update (:236-241)
    converge_on_norm: bool = False         # norm() < kMaxConvergeStep instead of squaredNorm() (:241)
    no_break: bool = False                 # pixels do not stop on their own: all run kMaxIteration steps (:241)
    upsample_half_pixel: bool = False      # samples at (r + 0.5) / 2 - 0.5 instead of r * 0.5 (:71-72)
    upsample_no_double: bool = False       # without * 2.0f (:74-75)
    median_rank: int = 4                   # nth_element position (:360-363)
    swap_d_e: bool = False                 # (D - E) under term1 and (D + E) under term2 (:287-291)
    zero_pad_moments: bool = False         # zero padding instead of the replicate clamp (:160-170)
    b_diff_reversed: bool = False          # b2 - b1 (:216)
    sample_ref_moments: bool = False       # the warped sample taken from image 0's moments (:212)
    interpolate_rounds: bool = False       # the warped sample at the nearest pixel, no bilinear (:307-312)
    median_zero_border: bool = False       # SmoothFlow's window zero-filled outside the image (:353-354)


DEFAULT = Flags()


@dataclasses.dataclass(frozen=True)
class Options:  # dense_optical_flow.h:15-20
    kMaxIteration: int = 10
    kHalfPatchSize: int = 2
    kMaxConvergeStep: float = 1e-6
    kMaxDeltaFlowStep: float = 1.0


# ---- InitializeGaussianKernel (:87-134) ---------------------------------------------------------------------------------------------

def gaussian(half: int, k=None):
    """(ok, weights (2h+1, 2h+1), (k2, k4, k22)).  half 0: weights [[1]] and k is the caller's (the object's previous values, :95-98;
    zeros for a fresh object, .h:51-53)."""
    k = (0.0, 0.0, 0.0) if k is None else tuple(float(x) for x in k)
    if half < 0:  # :88
        return False, None, k
    if half == 0:
        return True, np.ones((1, 1)), k
    d = np.arange(-half, half + 1, dtype=np.float64)
    dr, dc = d[:, None], d[None, :]
    w = np.exp(-0.5 * (dr * dr + dc * dc))  # sigma = 1 (:101)
    w /= w.sum()
    return True, w, (float((w * dr ** 2).sum()), float((w * dr ** 4).sum()), float((w * dr ** 2 * dc ** 2).sum()))


# ---- ComputeGaussianWeightedSecondMomentMatrix (:136-189) ---------------------------------------------------------------------------

def moments(image, half: int, w, flags: Flags = DEFAULT, with_abs: bool = False):
    """(6, rows, cols): S0, Sr, Sc, Src, Srr, Scc; with_abs also returns the per-pixel sums of |term|."""
    img = np.asarray(image, np.float64)
    rows, cols = img.shape
    pad = np.pad(img, half, mode="constant" if flags.zero_pad_moments else "edge") if half > 0 else img
    S = np.zeros((6, rows, cols))
    Sabs = np.zeros((6, rows, cols))
    for i, dr in enumerate(range(-half, half + 1)):
        for j, dc in enumerate(range(-half, half + 1)):
            t = pad[i:i + rows, j:j + cols] * w[i, j]
            f = (1.0, dr, dc, dr * dc, dr * dr, dc * dc)
            for n in range(6):
                S[n] += f[n] * t
                Sabs[n] += abs(f[n]) * np.abs(t)
    return (S, Sabs) if with_abs else S


def perturbed(S, Sabs, seed: int, rel: float):
    rs = np.random.RandomState(seed)
    return S + rel * rs.uniform(-1.0, 1.0, S.shape) * Sabs


# ---- ConstructConstrainFunctionForPixel (:247-303, :305-332) ------------------------------------------------------------------------

def coefficients(S6, k, flags: Flags = DEFAULT):
    """(a00, a01, a11, b0, b1) from six moments (arrays of any common shape, first axis the six)."""
    S0, Sr, Sc, Src, Srr, Scc = S6
    k2, k4, k22 = k
    D = k4 - k2 * k2
    E = k22 - k2 * k2
    inv_p = 1.0 / (D + E + EPS)
    inv_m = 1.0 / (D - E + EPS)
    if flags.swap_d_e:
        inv_p, inv_m = inv_m, inv_p
    term1 = (Srr + Scc - 2.0 * k2 * S0) * inv_p
    term2 = (Srr - Scc) * inv_m
    a = 0.5 * (term1 + term2)
    b_coeff = 0.5 * (term1 - term2)
    c_coeff = Src / (k22 + EPS)
    return a, 0.5 * c_coeff, b_coeff, Sr / (k2 + EPS), Sc / (k2 + EPS)


def interpolate(M, r, c, nearest: bool = False):
    """Utility::Interpolate: clamp-to-edge bilinear of the plane(s) M (..., rows, cols) at the float coordinates r, c (same shape)."""
    M = np.asarray(M, np.float64)
    rows, cols = M.shape[-2:]
    r = np.asarray(r, np.float64)
    c = np.asarray(c, np.float64)
    if nearest:
        r, c = np.floor(r + 0.5), np.floor(c + 0.5)
    fr, fc = np.floor(r), np.floor(c)
    sr, sc = r - fr, c - fc
    r0 = np.clip(fr, 0, rows - 1).astype(np.int64)
    r1 = np.clip(fr + 1.0, 0, rows - 1).astype(np.int64)
    c0 = np.clip(fc, 0, cols - 1).astype(np.int64)
    c1 = np.clip(fc + 1.0, 0, cols - 1).astype(np.int64)
    return (M[..., r0, c0] * ((1.0 - sr) * (1.0 - sc)) + M[..., r0, c1] * ((1.0 - sr) * sc)
            + M[..., r1, c0] * (sr * (1.0 - sc)) + M[..., r1, c1] * (sr * sc))


# ---- ComputeFlowByPixel (:191-245) --------------------------------------------------------------------------------------------------

def step(Sref, Scur, k, F, opt: Options, flags: Flags = DEFAULT, pixels=None):
    """The capped update (2, ...) of one iteration from the field F (2, rows, cols) (:202-234); `pixels` (a boolean mask) restricts
    it to some pixels, whose values come back as (2, n)."""
    rows, cols = Sref.shape[-2:]
    rr, cc = np.mgrid[0:rows, 0:cols]
    if pixels is None:
        pixels = np.ones((rows, cols), bool)
    rr, cc = rr[pixels], cc[pixels]
    a1, h1, d1, p1, q1 = coefficients(Sref[:, rr, cc], k, flags)  # the int overload: the pixel's own moments (:197)
    src = Sref if flags.sample_ref_moments else Scur
    S2 = interpolate(src, rr + F[0][pixels], cc + F[1][pixels], flags.interpolate_rounds)  # the MOMENTS are interpolated (:307-312)
    a2, h2, d2, p2, q2 = coefficients(S2, k, flags)
    g = 1.0 if flags.a_avg_no_half else 0.5
    m00, m01, m11 = 2.0 * g * (a1 + a2), 2.0 * g * (h1 + h2), 2.0 * g * (d1 + d2)  # M = 2 A_avg, symmetric (:215-220)
    e0, e1 = (p2 - p1, q2 - q1) if flags.b_diff_reversed else (p1 - p2, q1 - q2)
    n00 = m00 * m00 + m01 * m01  # MtM (:221)
    n01 = m00 * m01 + m01 * m11
    n11 = m01 * m01 + m11 * m11
    t0 = m00 * e0 + m01 * e1     # Mtb (:222)
    t1 = m01 * e0 + m11 * e1
    lam = flags.lambda_constant * (n00 + n11) + 1.0  # :225
    h00, h11 = n00 + lam, n11 + lam
    h01 = n01 + lam if flags.lambda_on_off_diagonal else n01
    det = h00 * h11 - h01 * h01
    dr = (h11 * t0 - h01 * t1) / det  # H^-1 Mtb (:227)
    dc = (h00 * t1 - h01 * t0) / det
    cap = float(f32(opt.kMaxDeltaFlowStep))
    if flags.cap_per_component:
        return np.stack([np.clip(dr, -cap, cap), np.clip(dc, -cap, cap)])
    norm = np.hypot(dr, dc)
    scale = np.where(norm > cap, cap / np.where(norm > cap, norm, 1.0), 1.0)  # :230-234
    return np.stack([dr * scale, dc * scale])


def gauss_newton(Sref, Scur, k, F, opt: Options, flags: Flags = DEFAULT, iterations=None):
    """The field before the median after `iterations` (default kMaxIteration) iterations from F, every pixel stopping on its own
    (:200-242).  Returns (field, active): active marks the pixels that have not taken their break."""
    F = np.array(F, np.float64, copy=True)
    thr = float(f32(opt.kMaxConvergeStep))
    active = np.ones(F.shape[1:], bool)
    n = int(opt.kMaxIteration) if iterations is None else min(int(iterations), int(opt.kMaxIteration))
    for _ in range(max(n, 0)):
        if not active.any():
            break
        d = step(Sref, Scur, k, F, opt, flags, active)
        sq = d[0] * d[0] + d[1] * d[1]
        small = (np.sqrt(sq) < thr) if flags.converge_on_norm else (sq < thr)  # :241
        if flags.no_break:
            small = np.zeros_like(small)
        if flags.converge_before_update:
            d = np.where(small, 0.0, d)
        F[0][active] += d[0]  # the update comes before the break (:237-241)
        F[1][active] += d[1]
        idx = np.nonzero(active)
        active[idx[0][small], idx[1][small]] = False
    return F, active


# ---- SmoothFlow (:334-371) ----------------------------------------------------------------------------------------------------------

def median3x3(P, flags: Flags = DEFAULT):
    """The 5th smallest of the clamp-to-edge 3 x 3 window, by value (numpy's sort)."""
    P = np.asarray(P, np.float64)
    rows, cols = P.shape
    pad = np.pad(P, 1, mode="constant" if flags.median_zero_border else "edge")
    win = np.stack([pad[i:i + rows, j:j + cols] for i in range(3) for j in range(3)])
    return np.sort(win, axis=0)[flags.median_rank]


# ---- Track(image, image, flow) (:7-33) ----------------------------------------------------------------------------------------------

def track_image(ref, cur, flow=(None, None), opt: Options = Options(), k=None, flags: Flags = DEFAULT, perturb=None, iterations=None,
                smooth: bool = True):
    """(ok, [flow_r, flow_c], k).  A plane of ref's shape is the initial guess, any other (None included) is reset to zero, each on its
    own (:18-23); ref and cur may differ in size.  iterations / smooth=False give the field before the median after j iterations."""
    ref = np.asarray(ref)
    cur = np.asarray(cur)
    ok, w, k = gaussian(int(opt.kHalfPatchSize), k)
    if not ok:
        return False, list(flow), k
    half = int(opt.kHalfPatchSize)
    planes = []
    for n, (img, seed_off) in enumerate(((ref, 0), (cur, 1))):
        S, Sabs = moments(img, half, w, flags, with_abs=True)
        if perturb is not None:
            S = perturbed(S, Sabs, 2 * perturb[0] + seed_off, perturb[1])
        planes.append(S)
    F = np.zeros((2,) + ref.shape)
    for n in range(2):
        if flow[n] is not None and np.shape(flow[n]) == ref.shape:
            F[n] = np.asarray(flow[n], np.float64)
    F, _ = gauss_newton(planes[0], planes[1], k, F, opt, flags, iterations)
    if smooth:
        F = np.stack([median3x3(F[0], flags), median3x3(F[1], flags)])
    return True, [F[0], F[1]], k


# ---- Track(pyramid, pyramid, flow) (:35-85) -----------------------------------------------------------------------------------------

def upsample(F, shape, flags: Flags = DEFAULT):
    """up(r, c) = Interpolate(F, r * 0.5, c * 0.5) * 2 on the next level's shape (:62-77); F is (2, rows, cols) or one plane."""
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    if flags.upsample_half_pixel:
        fr, fc = (rr + 0.5) * 0.5 - 0.5, (cc + 0.5) * 0.5 - 0.5
    else:
        fr, fc = rr * 0.5, cc * 0.5
    return interpolate(F, fr, fc) * (1.0 if flags.upsample_no_double else 2.0)


def track_pyramid(ref_levels, cur_levels, opt: Options = Options(), k=None, flags: Flags = DEFAULT, perturb=None):
    """(ok, [flow_r, flow_c], k) at level 0's size; the top level starts from zero.  The per-level result is ignored (:53): a negative
    half patch gives ok with the zero flow carried down."""
    if len(ref_levels) != len(cur_levels) or len(ref_levels) == 0:  # :37-39
        return False, [None, None], k
    top = len(ref_levels) - 1
    F = np.zeros((2,) + np.shape(ref_levels[top]))
    for lvl in range(top, -1, -1):
        p = None if perturb is None else (perturb[0] * 16 + lvl, perturb[1])
        ok, out, k2 = track_image(ref_levels[lvl], cur_levels[lvl], (F[0], F[1]), opt, k, flags, p)
        if ok:
            F, k = np.stack(out), k2
        if lvl == 0:
            break
        F = upsample(F, np.shape(ref_levels[lvl - 1]), flags)
    return True, [F[0], F[1]], k
