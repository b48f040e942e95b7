"""GroupNorm references (TEST INFRASTRUCTURE ONLY): (a) `gn_fp64`, the formula in float64; (b) `gn_kernel_order`, a numpy restatement of
csrc/groupnorm.hip in the kernel's documented fp32 / fp64 summation order, regime by regime -- the GPU tests compare bits against it; `gn_naive_fp32`,
the plain fp32 E[x^2] - mu^2 the kernel must NOT be; and `gn_bound`, the error bound of (b) against (a), derived below.

x is [N, H, W, C] (N images or RoI slabs), statistics over (H, W, C / groups) per image and group, biased variance, clamped at 0 before + eps.

ERROR BOUND of the kernel's scheme (first order in u = 2^-24; fp64 steps contribute u^2-sized terms and are dropped).
Notation per (image, group): K the pivot x[pixel 0][first channel of the group], d = x - K, md = mean(d), mu = K + md, s = sqrt(var + eps),
k = the longest fp32 chain of one thread (32 pixels for large planes, ceil(HW / rows) <= 13 for slabs).
  1. d~ = fl(x - K):                        |d~ - d| <= u |d|.
  2. S1: every fp32 chain adds at most k terms, so each term takes part in at most k roundings; with 1.:  |S1~ - S1| <= (k + 1) u sum|d|.
     The chains' results are combined in fp64 (exact at this order).  m = fl32(S1~ / count):
         |m - md| <= u A,   A = (k + 1) mean|d| + |md|.
  3. S2: d~^2 carries 2u (from d~) + u (the product), the chain k u:   |S2~ - S2| <= (k + 3) u sum d^2.
     var~ = S2~/count - md~^2 (fp64):   |var~ - var| <= u V,   V = (k + 3) mean(d^2) + 2 |md| (k + 1) mean|d|.
     rstd~ = fl32(1 / sqrt(var~ + eps)):  relative error rho = u (V / (2 s^2) + 1).
  4. apply, t~ = fl(d~ - m) against t = x - mu:   |t~ - t| <= u (|d| + A + |t|);
     z = t rstd gamma: two products (2u) and rho;  y0 = z + beta: u |y0|;  the residual add: u |y0 + res|  (ReLU is exact and a contraction).
         |y~ - y| <= u [ |gamma| / s (|x - K| + A + |x - mu|)  +  |gamma| |x - mu| / s (V / (2 s^2) + 3)  +  |y0|  +  |y0 + res| ]
The second term is the "unit roundoff x depth x |gamma| |x - mu| / sigma" of the variance (V / (2 s^2) is (k + 3) / 2 when the pivot sits at the mean
and grows with ((K - mu) / sigma)^2 when it does not); the first is the error of the mean itself, which no fp32 scheme avoids; the rest is the beta /
residual rounding.  The bound is taken times 1.05 for the dropped second-order terms, plus one float32 denormal.  It is derived from the scheme, not
fitted: a naive fp32 E[x^2] - mu^2 misses it by orders of magnitude on offset data (tests/test_groupnorm_cpu.py checks that).
"""
import numpy as np

U = 2.0 ** -24
SLAB_HW = 196        # csrc/groupnorm.hip GN_SLAB_HW
CHUNK_ITERS = 32     # GN_CHUNK_ITERS
THREADS = 256
TILE_C = 64


def is_slab(H, W):
    return H * W <= SLAB_HW


def geometry(C):
    tw = min(C, TILE_C)
    ncol = tw // 4
    return tw, ncol, THREADS // ncol


def gn_fp64(x, groups, gamma, beta, eps=1e-5, residual=None, relu=False):
    """(a) float64, straight from the formula.  -> float64 [N, H, W, C]"""
    x64 = np.asarray(x, np.float64)
    N, H, W, C = x64.shape
    g = x64.reshape(N, H * W, groups, C // groups)
    mu = g.mean(axis=(1, 3), keepdims=True)
    var = np.maximum(((g - mu) ** 2).mean(axis=(1, 3), keepdims=True), 0.0)
    y = ((g - mu) / np.sqrt(var + float(np.float32(eps)))).reshape(N, H, W, C) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return np.maximum(y, 0.0) if relu else y


def _stats_kernel_order(d, groups, slab):
    """d [N, HW, C] float32 (shifted data) -> (S1, S2) float64 [N, groups] in the kernel's order (steps 1-5 of csrc/groupnorm.hip)."""
    N, HW, C = d.shape
    cpg = C // groups
    _, _, rows = geometry(C)
    iters = -(-HW // rows) if slab else CHUNK_ITERS
    P = rows * iters
    nch = 1 if slab else -(-HW // P)
    dd = np.zeros((N, nch * P, C), np.float32)   # padding adds +0 to a chain: the same bits as the kernel's skipped pixels
    dd[:, :HW] = d
    dd = dd.reshape(N, nch, iters, rows, C)
    s1 = np.zeros((N, nch, rows, C), np.float32)
    s2 = np.zeros((N, nch, rows, C), np.float32)
    for k in range(iters):                        # 1. fp32 chain of thread (r, q) over its pixels p0 + r + k * rows
        v = dd[:, :, k]
        s1 = s1 + v
        s2 = s2 + v * v
    c1 = np.zeros((N, nch, C), np.float64)
    c2 = np.zeros((N, nch, C), np.float64)
    for r in range(rows):                         # 2. fp64 chain over the rows, per channel
        c1 = c1 + s1[:, :, r].astype(np.float64)
        c2 = c2 + s2[:, :, r].astype(np.float64)
    c1 = c1.reshape(N, nch, groups, cpg)
    c2 = c2.reshape(N, nch, groups, cpg)
    g1 = np.zeros((N, nch, groups), np.float64)
    g2 = np.zeros((N, nch, groups), np.float64)
    for c in range(cpg):                          # 3. fp64 chain over the group's channels
        g1 = g1 + c1[..., c]
        g2 = g2 + c2[..., c]
    if slab:
        return g1[:, 0], g2[:, 0]
    out = []
    for part in (g1, g2):
        it = -(-nch // 64)
        p = np.zeros((N, it * 64, groups), np.float64)
        p[:, :nch] = part
        p = p.reshape(N, it, 64, groups)
        lane = np.zeros((N, 64, groups), np.float64)
        for i in range(it):                       # 4. lane l chains chunks l, l + 64, ...
            lane = lane + p[:, i]
        off = 32
        while off >= 1:                           # 5. tree over the 64 lanes
            lane = lane[:, :off] + lane[:, off:2 * off]
            off //= 2
        out.append(lane[:, 0])
    return out[0], out[1]


def gn_moments_kernel_order(x, groups, eps=1e-5):
    """The statistics half of (b): -> (d [N, HW, C] fp32 shifted data, m [N, groups] fp32, rstd [N, groups] fp32).  gn_kernel_order takes the result as
    `moments`, so a test that applies several epilogues to one input pays for the summation once."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, C = x.shape
    HW, cpg = H * W, C // groups
    assert C % 4 == 0 and C % groups == 0 and C % min(C, TILE_C) == 0 and min(C, TILE_C) % cpg == 0, (C, groups)
    xr = x.reshape(N, HW, C)
    grp = np.arange(C) // cpg
    with np.errstate(all="ignore"):
        K = xr[:, 0, grp * cpg]                               # [N, C]: the group's pivot, per channel
        d = xr - K[:, None, :]
        S1, S2 = _stats_kernel_order(d, groups, is_slab(H, W))
        cnt = np.float64(HW * cpg)
        md = S1 / cnt
        var = S2 / cnt - md * md
        var = np.where(var > 0.0, var, 0.0)
        m = md.astype(np.float32)
        rstd = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)
    return d, m, rstd


def gn_kernel_order(x, groups, gamma, beta, eps=1e-5, residual=None, relu=False, moments=None):
    """(b) csrc/groupnorm.hip restated: shifted data, the documented summation order, fp64 moments, fp32 apply.  -> float32 [N, H, W, C]"""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, C = x.shape
    if N == 0:
        return x.copy()
    HW = H * W
    grp = np.arange(C) // (C // groups)
    d, m, rstd = gn_moments_kernel_order(x, groups, eps) if moments is None else moments
    with np.errstate(all="ignore"):
        y = (d - m[:, None, grp]) * rstd[:, None, grp] * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)
        if residual is not None:
            y = y + np.ascontiguousarray(residual, np.float32).reshape(N, HW, C)
        if relu:
            y = np.where(y > 0.0, y, np.float32(0.0))
    assert y.dtype == np.float32
    return y.reshape(N, H, W, C)


def affine(rng, C):
    """gamma in [0.5, 1.5], beta ~ 0.1 N(0, 1): what a trained norm looks like."""
    return rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)


def check_bits(ffi, x, groups, seed=0, eps=1e-5, gamma_beta=None):
    """The kernel through ffi.group_norm against the restatement, bit for bit: plain, ReLU, residual, residual + ReLU, each out of place and in place."""
    rng = np.random.default_rng(seed)
    ga, be = affine(rng, x.shape[-1]) if gamma_beta is None else gamma_beta
    res = rng.standard_normal(x.shape).astype(np.float32)
    mom = gn_moments_kernel_order(x, groups, eps)
    for kw in (dict(), dict(residual=res, relu=True), dict(relu=True), dict(residual=res)):
        want = gn_kernel_order(x, groups, ga, be, eps, kw.get("residual"), kw.get("relu", False), moments=mom)
        for inplace in (False, True):
            got = ffi.group_norm(x, groups, ga, be, eps, inplace=inplace, **kw)
            assert got.shape == x.shape and np.array_equal(got, want), (x.shape, groups, eps, sorted(kw), inplace)


def gn_naive_fp32(x, groups, gamma, beta, eps=1e-5):
    """What the kernel must not be: one-pass fp32 E[x^2] - mu^2 (pairwise sums, so the sums themselves are as good as fp32 gets)."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, C = x.shape
    g = x.reshape(N, H * W, groups, C // groups)
    cnt = np.float32(H * W * (C // groups))
    mu = g.sum(axis=(1, 3), keepdims=True, dtype=np.float32) / cnt
    ex2 = (g * g).sum(axis=(1, 3), keepdims=True, dtype=np.float32) / cnt
    var = np.maximum(ex2 - mu * mu, np.float32(0.0))
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    return ((g - mu) * rstd).reshape(N, H, W, C) * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)


def gn_bound(x, groups, gamma, beta, eps=1e-5, residual=None):
    """Elementwise bound on |kernel - fp64| (module docstring).  -> float64 [N, H, W, C]"""
    x64 = np.asarray(x, np.float64)
    N, H, W, C = x64.shape
    HW, cpg = H * W, C // groups
    _, _, rows = geometry(C)
    k = -(-HW // rows) if is_slab(H, W) else CHUNK_ITERS
    g = x64.reshape(N, HW, groups, cpg)
    K = g[:, :1, :, :1]
    d = g - K
    md = d.mean(axis=(1, 3), keepdims=True)
    mabs = np.abs(d).mean(axis=(1, 3), keepdims=True)
    m2 = (d * d).mean(axis=(1, 3), keepdims=True)
    var = np.maximum(m2 - md * md, 0.0)
    s = np.sqrt(var + float(np.float32(eps)))
    A = (k + 1) * mabs + np.abs(md)
    V = (k + 3) * m2 + 2 * np.abs(md) * (k + 1) * mabs
    t = d - md
    ga = np.abs(np.asarray(gamma, np.float64)).reshape(groups, cpg)
    y0 = gn_fp64(x, groups, gamma, beta, eps).reshape(N, HW, groups, cpg)
    yr = y0 if residual is None else y0 + np.asarray(residual, np.float64).reshape(N, HW, groups, cpg)
    b = ga / s * (np.abs(d) + A + np.abs(t)) + ga * np.abs(t) / s * (V / (2 * s * s) + 3) + np.abs(y0) + np.abs(yr)
    return (1.05 * U * b + 2.0 ** -149).reshape(N, H, W, C)
