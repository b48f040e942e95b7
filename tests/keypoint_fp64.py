"""fp64 reference of the keypoint decode, written from the definition (TEST INFRASTRUCTURE ONLY; numpy only, no code shared with
tests/keypoint_ref.py): bicubic resize with the cubic convolution kernel at A = -0.75, half-pixel centres, taps clamped to the map, any side S, float64
throughout, followed by the first arg-max in row-major order; and the quantities of the fp32 error bound e.

THE DEFINITION.  W(x) = (A + 2)|x|^3 - (A + 3)|x|^2 + 1 for |x| <= 1, A|x|^3 - 5A|x|^2 + 8A|x| - 4A for 1 < |x| < 2, 0 beyond.  Output index d of n_out
over n_in samples the source at f = (d + 0.5) n_in / n_out - 0.5; with s = floor(f) the four taps s-1 .. s+2 carry W(f - tap) and are clamped to 0 .. n_in-1.
The resize is separable, so it is written as two dense matrices: out = Ry m Rx^T, Ry [hc, S], Rx [wc, S].

THE BOUND e (u = 2^-24, the unit roundoff of fp32; the kernel and the restatement perform the operations named here, each rounded once).
 (a) Products and sums.  A row value is ((wx0 m0 + wx1 m1) + wx2 m2) + wx3 m3: four products and three sums, so every term carries at most four roundings;
     the vertical pass adds four more.  |error| <= gamma_8 * sum|wy||wx||m| with gamma_8 = 8u / (1 - 8u): the `absum` term, |Ry| |m| |Rx|^T.
 (b) The sampling point.  f = fl(fl((d + 0.5) * fl(n_in / n_out)) - 0.5): d + 0.5 is exact, the quotient, the product and the difference each round once, so
     with g(d) = (d + 0.5) n_in / n_out = f + 0.5, |df| <= u (2 g + |f|) <= 3u g(d) -- at most 3u S, that is 1.5 * 2^-23 S.  t = f - s is exact for
     f >= 0 (s <= f < s + 1, and s is a multiple of f's last place) and rounds once, by at most u, for -0.5 < f < 0.  So |dt| <= u (3 g(d) + 1).  The
     interpolant is C1 in f (W' is continuous: W'(1) = A from both sides, W'(2) = 0), so f stepping over an integer changes nothing to first order, and
     a weight moves by at most |dt| |W'(f - tap)|: the `dsum` term, (D_y |Ry'|) |m| |Rx|^T + |Ry| |m| (D_x |Rx'|)^T with D = diag(u (3 g(d) + 1)).
 (c) The weight polynomials, evaluated in fp32 from the fp32 t (absolute errors; the intermediate magnitudes are for t in [0, 1], x = t + 1 in [1, 2]):
     w1 = ((1.25 t - 2.25) t) t + 1: 1.25u, +2.25u, *t +2.25u, *t +2.25u, +1: u  -> 9u.
     w2 = the same in fl(1 - t), whose rounding u/2 passes through |W'| <= 1.35 on [0, 1]                                        -> 9.7u.
     w0 = ((A x - 5A) x + 8A) x - 4A with x = fl(t + 1), rounding u, through |W'| <= 0.75 on [1, 2]: 0.75u;  A x: 1.5u;  + 3.75 (result <= 3): 4.5u;
          * x (<= 2, result <= 4.5): 13.5u;  - 6 (result in [-3, -1.5]): 16.5u;  * x (result about -3): 36.1u;  + 3: 37u                  -> 37u.
     w3 = ((1 - w0) - w1) - w2: the three errors above and three roundings of values <= 1.1                                     -> 59u.
     The `wsum` term: (Cy |m| |Rx|^T + |Ry| |m| Cx^T) u, C holding 37, 9, 9.7, 59 at the four clamped taps.
 e = (1 + 2^-10) (gamma_8 absum + dsum + u wsum); the factor covers the second-order terms (errors of the weights inside (a), W'' inside (b)), which are
 below 100u relative.  Nothing here is fitted: tests/test_keypoint_fp64_cpu.py prints the largest err / e of the restatement and shows that four altered
 restatements break the bound.
"""
import functools

import numpy as np

A = -0.75
U = 2.0 ** -24
GAMMA8 = 8 * U / (1 - 8 * U)
W_ERR = (37.0, 9.0, 9.7, 59.0)


def cubic_kernel(x):
    """W(x) of the cubic convolution, float64, any shape"""
    x = np.abs(np.asarray(x, np.float64))
    inner = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    outer = ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.where(x <= 1.0, inner, np.where(x < 2.0, outer, 0.0))


def cubic_kernel_slope(x):
    """|W'(x)|"""
    x = np.abs(np.asarray(x, np.float64))
    inner = (3.0 * (A + 2.0) * x - 2.0 * (A + 3.0)) * x
    outer = (3.0 * A * x - 10.0 * A) * x + 8.0 * A
    return np.abs(np.where(x <= 1.0, inner, np.where(x < 2.0, outer, 0.0)))


@functools.lru_cache(maxsize=64)
def matrices(n_out, n_in):
    """-> R, |R'| * u (3 g + 1), C: [n_out, n_in] float64 each -- the resize matrix of one axis, its slope term and its weight-error term of the bound"""
    d = np.arange(n_out, dtype=np.float64)
    g = (d + 0.5) * (float(n_in) / float(n_out))
    f = g - 0.5
    s = np.floor(f)
    R, D, C = (np.zeros((n_out, n_in), np.float64) for _ in range(3))
    rows = np.arange(n_out)
    for j in range(4):
        tap = s + (j - 1)
        col = np.clip(tap, 0, n_in - 1).astype(np.int64)
        np.add.at(R, (rows, col), cubic_kernel(f - tap))
        np.add.at(D, (rows, col), cubic_kernel_slope(f - tap) * U * (3.0 * g + 1.0))
        np.add.at(C, (rows, col), W_ERR[j])
    return R, D, C


def resize(m, hc, wc):
    """m [S, S] -> [hc, wc] float64"""
    m = np.asarray(m, np.float64)
    assert m.ndim == 2 and m.shape[0] == m.shape[1]
    Ry, Rx = matrices(hc, m.shape[0])[0], matrices(wc, m.shape[1])[0]
    return Ry @ m @ Rx.T


def resize_with_bound(m, hc, wc):
    """-> (out [hc, wc] float64, e [hc, wc] float64, parts {absum, dsum, wsum})"""
    m = np.asarray(m, np.float64)
    S = m.shape[0]
    Ry, Dy, Cy = matrices(hc, S)
    Rx, Dx, Cx = matrices(wc, S)
    # |w| per tap: clamped taps that fall on one source pixel are summed as absolute values (np.abs(Ry) would let them cancel at a border row)
    am, aRy, aRx = np.abs(m), _abs_matrix(hc, S), _abs_matrix(wc, S)
    right = am @ aRx.T
    absum = aRy @ right
    dsum = Dy @ right + aRy @ (am @ Dx.T)
    wsum = Cy @ right + aRy @ (am @ Cx.T)
    e = (1.0 + 2.0 ** -10) * (GAMMA8 * absum + dsum + U * wsum)
    return Ry @ m @ Rx.T, e, dict(absum=absum, dsum=dsum, wsum=wsum)


@functools.lru_cache(maxsize=64)
def _abs_matrix(n_out, n_in):
    d = np.arange(n_out, dtype=np.float64)
    f = (d + 0.5) * (float(n_in) / float(n_out)) - 0.5
    s = np.floor(f)
    out = np.zeros((n_out, n_in), np.float64)
    for j in range(4):
        tap = s + (j - 1)
        np.add.at(out, (np.arange(n_out), np.clip(tap, 0, n_in - 1).astype(np.int64)), np.abs(cubic_kernel(f - tap)))
    return out


def against_bound(m, hc, wc, score, pos):
    """One map's answer (score, row-major position) against fp64 -> (|score - max| / max(e[p*], e[pos]), (max - r[pos]) / (e[p*] + e[pos])), p* the fp64
    arg-max.  Both must be <= 1 for an fp32 evaluation v with |v - r| <= e that picks its own maximum: v[pos] >= v[p*] >= r[p*] - e[p*] and
    v[pos] <= r[pos] + e[pos] <= r[p*] + e[pos]; so the score lies within max(e[p*], e[pos]) <= e of the maximum and r[pos] within e[p*] + e[pos] <= 2e."""
    r, e, _ = resize_with_bound(m, hc, wc)
    r, e = r.reshape(-1), e.reshape(-1)
    p = int(np.argmax(r))
    return abs(float(score) - r[p]) / max(e[p], e[pos]), (r[p] - r[pos]) / (e[p] + e[pos])


def sides(box):
    """box [4] (fp32 values) -> (w, h as float32, wc, hc): w = max(x2 - x1, 1) in fp32 as the operator forms it, wc = ceil(w), cut at 16384"""
    b = np.asarray(box, np.float32)
    w, h = max(b[2] - b[0], np.float32(1.0)), max(b[3] - b[1], np.float32(1.0))
    return np.float32(w), np.float32(h), min(int(np.ceil(w)), 16384), min(int(np.ceil(h)), 16384)


def keypoint(box, pos):
    """The keypoint of row-major position `pos`: (x1 + (x_int + 0.5) w / wc, y1 + (y_int + 0.5) h / hc, 1), the fp32 formula of DESIGN.md 14"""
    F = np.float32
    b = np.asarray(box, F)
    w, h, wc, hc = sides(b)
    xi, yi = pos % wc, pos // wc
    return np.array([(F(xi) + F(0.5)) * (w / F(wc)) + b[0], (F(yi) + F(0.5)) * (h / F(hc)) + b[1], 1.0], F)


def position_of(box, kpt):
    """The inverse of keypoint(): the row-major position whose keypoint has exactly these bits (the formula is strictly increasing in x_int and y_int)"""
    F = np.float32
    b = np.asarray(box, F)
    w, h, wc, hc = sides(b)
    xs = (np.arange(wc, dtype=F) + F(0.5)) * (w / F(wc)) + b[0]
    ys = (np.arange(hc, dtype=F) + F(0.5)) * (h / F(hc)) + b[1]
    xi, yi = np.nonzero(xs == F(kpt[0]))[0], np.nonzero(ys == F(kpt[1]))[0]
    assert len(xi) == 1 and len(yi) == 1, (box, kpt, xi, yi)
    return int(yi[0]) * wc + int(xi[0])


def decode_one(maps, box):
    """maps [S, S, K], box [4] -> (kpt [K, 3] float32, score [K] float64, pos [K], n_max [K]: how many positions hold the maximum)"""
    maps = np.asarray(maps)
    _, _, wc, hc = sides(box)
    K = maps.shape[2]
    kpt, score, pos, nmax = np.zeros((K, 3), np.float32), np.zeros(K, np.float64), np.zeros(K, np.int64), np.zeros(K, np.int64)
    for k in range(K):
        r = resize(maps[:, :, k], hc, wc).reshape(-1)
        p = int(np.argmax(r))
        kpt[k], score[k], pos[k], nmax[k] = keypoint(box, p), r[p], p, int((r == r[p]).sum())
    return kpt, score, pos, nmax
