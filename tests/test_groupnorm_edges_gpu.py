"""GroupNorm kernels (csrc/groupnorm.hip) away from the model's geometries: tiles narrower than 64 channels (idle threads), every layout of groups inside
a tile and inside a thread's float4, the chunk counts around the finalize's 64 lanes, eps, a signed / zero gamma, a non-finite or outlying pivot, and the
launcher's refusals.  Everything through _ffi.group_norm; every comparison BIT FOR BIT against tests/groupnorm_ref.gn_kernel_order (plain, ReLU, residual,
residual + ReLU, each out of place and in place), which tests/test_groupnorm_cpu.py holds inside the derived bound of float64 at these same inputs
(tests/groupnorm_cases.py)."""
import numpy as np
import pytest

import groupnorm_cases as GC
import groupnorm_ref as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", GC.NARROW, ids=str)
def test_narrow_tiles(ffi, case):
    """C < 64: TW = C, ncol = C / 4, rows = 256 / ncol rounded down; the threads with r >= rows take no part in loads, partials or stores."""
    _, ncol, rows = G.geometry(case[3])
    assert case[3] < 64 and (rows * ncol < 256 or ncol == 1)
    G.check_bits(ffi, GC.normal(case), case[4], seed=1)


@pytest.mark.parametrize("case", GC.LAYOUTS, ids=str)
def test_group_layouts_inside_a_tile(ffi, case):
    G.check_bits(ffi, GC.normal(case), case[4], seed=2)


@pytest.mark.parametrize("case", GC.CHUNKS, ids=lambda c: "W%d" % c[2])
def test_chunk_boundaries(ffi, case):
    """1 | 2, 2 | 3, 64 | 65 and 128 | 129 chunks of 512 pixels: the last chunk's tail, and the finalize's lanes chaining a second and a third partial."""
    assert not G.is_slab(case[1], case[2])
    G.check_bits(ffi, GC.normal(case), case[4], seed=3)


@pytest.mark.parametrize("eps", GC.EPS)
@pytest.mark.parametrize("case", GC.EPS_SHAPES, ids=str)
def test_eps_is_used(ffi, case, eps):
    x = GC.normal(case)
    G.check_bits(ffi, x, case[4], seed=4, eps=eps)
    if eps == 1e-3:   # a kernel that dropped the argument would give 1e-5's bits
        ga, be = G.affine(np.random.default_rng(4), case[3])
        assert not np.array_equal(ffi.group_norm(x, case[4], ga, be, 1e-3), ffi.group_norm(x, case[4], ga, be, 1e-5))


@pytest.mark.parametrize("case", GC.EPS_SHAPES, ids=str)
def test_signed_and_zero_gamma(ffi, case):
    ga, be = GC.signed_affine(case[3])
    assert (ga < 0).any() and (ga == 0).sum() >= case[3] // 5
    G.check_bits(ffi, GC.normal(case), case[4], seed=5, gamma_beta=(ga, be))


@pytest.mark.parametrize("shape", [(3, 14, 14, 256), (2, 25, 42, 256)])
def test_nonfinite_pivot_stays_in_its_group(ffi, shape):
    """The pivot K = x[n, 0, 0, first channel of the group] reaches every thread of the group on its own route (a scalar load in the slab kernel, the
    statistics buffer in the plane regime): a NaN / inf there makes exactly (image 1, group 5) non-finite and leaves every other bit alone."""
    rng = np.random.default_rng(6)
    ga, be = G.affine(rng, 256)
    x = rng.standard_normal(shape).astype(np.float32)
    clean = ffi.group_norm(x, 32, ga, be)
    assert np.array_equal(clean, G.gn_kernel_order(x, 32, ga, be))
    hit = np.zeros(shape, bool)
    hit[1, :, :, 40:48] = True
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 0, 0, 8 * 5] = bad
        for inplace in (False, True):
            got = ffi.group_norm(y, 32, ga, be, inplace=inplace)
            assert np.array_equal(got[~hit], clean[~hit]), (bad, inplace)
            assert not np.isfinite(got[hit]).any(), (bad, inplace)


@pytest.mark.parametrize("shape", [(2, 7, 7, 256), (1, 25, 42, 256)])
def test_outlier_pivot(ffi, shape):
    """Pivots at 30 sigma: mean(d) is 30 sigma instead of O(sigma), which is where the shifted-data scheme is weakest and its bound loosest (the variance
    term grows with ((K - mu) / sigma)^2).  Bit-exact against the restatement, inside the bound against float64; the figures are in DESIGN.md 11."""
    x = GC.outlier_pivot(shape)
    G.check_bits(ffi, x, 32, seed=7)
    ga, be = G.affine(np.random.default_rng(7), 256)
    err = np.abs(ffi.group_norm(x, 32, ga, be).astype(np.float64) - G.gn_fp64(x, 32, ga, be))
    bound = G.gn_bound(x, 32, ga, be)
    print("outlier pivot %s: max err %.3e, max err / bound %.4f" % (shape, float(err.max()), float((err / bound).max())))
    assert np.all(err <= bound), float((err / bound).max())


# ------------------------------------------------------------------------------------------------------------------- launcher
def _buffers(ffi, shape, pad=0):
    """x, gamma, beta, residual, poisoned out: each `pad` bytes longer than the shape needs, so a pointer moved by `pad` stays inside its allocation."""
    n = int(np.prod(shape))
    Cc = shape[-1]
    rng = np.random.default_rng(8)
    mk = lambda k: ffi.DeviceBuffer.from_numpy(rng.standard_normal(k + pad // 4).astype(np.float32))
    return mk(n), mk(Cc), mk(Cc), mk(n), ffi.DeviceBuffer((n + pad // 4,)).poison()


def _untouched(buf):
    return bool((buf.numpy().view(np.uint8) == 0xFF).all())


@pytest.mark.parametrize("shape", [(2, 7, 7, 64), (1, 15, 15, 64)])
@pytest.mark.parametrize("which", ["x", "out", "gamma", "residual"])
def test_unaligned_pointer_is_refused(ffi, shape, which):
    dx, dg, db, dr, do = _buffers(ffi, shape, pad=16)
    N, H, W, Cc = shape
    with pytest.raises(ffi.IsegmiError, match="16-byte aligned"):
        ffi.group_norm_device(dx, N, H, W, Cc, 32, dg, db, d_residual=dr, d_out=do, offsets={which: 4})
    assert _untouched(do)
    ffi.group_norm_device(dx, N, H, W, Cc, 32, dg, db, d_residual=dr, d_out=do, offsets={which: 16})   # the same call, aligned: accepted
    ffi.sync()
    assert np.isfinite(do.numpy()[4 if which == "out" else 0:][: N * H * W * Cc]).all()


def test_workspace_is_checked(ffi):
    shape = (1, 15, 15, 64)
    N, H, W, Cc = shape
    need = ffi.lib().isegmi_op_group_norm_workspace_bytes(N, H, W, Cc, 32)
    assert need == 1 * 1 * 32 * 16 + 32 * 16
    dx, dg, db, dr, do = _buffers(ffi, shape)
    ws = ffi.DeviceBuffer((need,), np.uint8)
    with pytest.raises(ffi.IsegmiError, match="workspace"):
        ffi.group_norm_device(dx, N, H, W, Cc, 32, dg, db, d_out=do, d_ws=ws, ws_bytes=need - 1)     # one byte short
    assert _untouched(do)
    with pytest.raises(ffi.IsegmiError, match="workspace"):
        ffi.group_norm_device(dx, N, H, W, Cc, 32, dg, db, d_out=do, alloc_ws=False)                   # none at all
    assert _untouched(do)
    assert ffi.lib().isegmi_op_group_norm_workspace_bytes(N, 14, 14, Cc, 32) == 0                      # a slab needs none
    ffi.group_norm_device(dx, N, 14, 14, Cc, 32, dg, db, d_out=do, alloc_ws=False)
    ffi.group_norm_device(dx, N, H, W, Cc, 32, dg, db, d_out=do, d_ws=ws)                              # exactly enough
    ffi.sync()
    assert np.isfinite(do.numpy()).all()


@pytest.mark.parametrize("shape,groups,msg", [((1, 4, 4, 6), 1, "multiple of 4"), ((1, 4, 4, 128), 1, "whole groups"), ((1, 15, 15, 128), 1, "whole groups")])
def test_bad_channel_counts_are_refused(ffi, shape, groups, msg):
    """C = 6 has no float4 rows; one group of 128 channels is wider than the 64-channel tile (slab and plane)."""
    dx, dg, db, dr, do = _buffers(ffi, shape)
    N, H, W, Cc = shape
    with pytest.raises(ffi.IsegmiError, match=msg):
        ffi.group_norm_device(dx, N, H, W, Cc, groups, dg, db, d_out=do)
    assert _untouched(do)


def test_empty_batch_of_planes_launches_nothing(ffi):
    """N = 0 with a plane shape: OK, no workspace asked for, nothing written (the buffers are sized for one image, so a launch would show)."""
    shape = (1, 15, 15, 64)
    dx, dg, db, dr, do = _buffers(ffi, shape)
    assert ffi.lib().isegmi_op_group_norm_workspace_bytes(0, 15, 15, 64, 32) == 0
    ffi.group_norm_device(dx, 0, 15, 15, 64, 32, dg, db, d_residual=dr, relu=True, d_out=do, alloc_ws=False)
    ffi.sync()
    assert _untouched(do)
    ga, be = G.affine(np.random.default_rng(0), 64)
    assert ffi.group_norm(np.zeros((0, 15, 15, 64), np.float32), 32, ga, be).shape == (0, 15, 15, 64)
