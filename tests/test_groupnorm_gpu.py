"""GroupNorm kernels (csrc/groupnorm.hip) through _ffi.group_norm: bit-exact against the numpy restatement in the kernel's summation order
(tests/groupnorm_ref.gn_kernel_order) at the shapes where an indexing or tail error shows, inside the derived bound against float64, NaN
containment, determinism."""
import numpy as np
import pytest

import groupnorm_ref as G

pytestmark = pytest.mark.gpu


_affine, _check_bits = G.affine, G.check_bits


# channels per group 2, 8, 64 (C = 64, 256, 2048 with 32 groups) and DIM_PER_GP 16; planes of 1, 49, 196 (slabs) and 25x42, 37x53 (chunks of 512 pixels:
# neither is a multiple); N = 1 and 3
@pytest.mark.parametrize("N,H,W,C,groups", [
    (1, 1, 1, 64, 32), (3, 7, 7, 64, 32), (1, 14, 14, 64, 32), (3, 25, 42, 64, 32), (1, 37, 53, 64, 32),
    (3, 1, 1, 256, 32), (1, 7, 7, 256, 32), (3, 14, 14, 256, 32), (1, 25, 42, 256, 32), (3, 37, 53, 256, 32),
    (1, 1, 1, 2048, 32), (3, 7, 7, 2048, 32), (1, 14, 14, 2048, 32), (1, 25, 42, 2048, 32),
    (3, 7, 7, 256, 16), (1, 37, 53, 256, 16), (1, 25, 42, 512, 32), (2, 5, 5, 32, 8),
])
def test_bit_exact_against_the_kernel_order_restatement(ffi, N, H, W, C, groups):
    rng = np.random.default_rng(N * 1000003 + H * 1009 + W * 31 + C)
    _check_bits(ffi, (rng.standard_normal((N, H, W, C)) * 2 + 0.5).astype(np.float32), groups)


def test_regime_boundary(ffi):
    """H * W = 196 is the last slab (one launch, registers), 197 the first plane (statistics + apply passes)."""
    assert G.is_slab(14, 14) and not G.is_slab(1, 197)
    rng = np.random.default_rng(5)
    for hw in ((14, 14), (1, 196), (1, 197), (197, 1)):
        _check_bits(ffi, rng.standard_normal((2,) + hw + (256,)).astype(np.float32), 32)


@pytest.mark.parametrize("R", [0, 1, 257, 2100])
def test_slab_counts(ffi, R):
    """RoI-head slabs: none (nothing launched), one, more than one wave of blocks, and slabs x groups > 65535 (2100 RoIs of 7x7x256)."""
    rng = np.random.default_rng(R)
    x = rng.standard_normal((R, 7, 7, 256)).astype(np.float32)
    ga, be = _affine(rng, 256)
    got = ffi.group_norm(x, 32, ga, be, relu=True)
    assert got.shape == x.shape and np.array_equal(got, G.gn_kernel_order(x, 32, ga, be, relu=True))


def _inputs(rng, shape):
    n01 = rng.standard_normal(shape).astype(np.float32)
    return {"normal": n01, "relu": np.maximum(n01, 0), "offset": (n01 * np.float32(0.5) + np.float32(500.0)).astype(np.float32)}


@pytest.mark.parametrize("shape", [(2, 7, 7, 256), (2, 14, 14, 256), (1, 25, 42, 256), (2, 37, 53, 64), (2, 1, 1, 2048)])
def test_inside_the_derived_bound_against_fp64(ffi, shape):
    """N(0,1), ReLU-like and offset (|mu| / sigma = 1e3) inputs: |kernel - fp64| <= the bound derived in groupnorm_ref from the summation scheme."""
    rng = np.random.default_rng(sum(shape))
    ga, be = _affine(rng, shape[-1])
    for name, x in _inputs(rng, shape).items():
        got = ffi.group_norm(x, 32, ga, be).astype(np.float64)
        err, bound = np.abs(got - G.gn_fp64(x, 32, ga, be)), G.gn_bound(x, 32, ga, be)
        print("%s %s: max err / bound = %.3f" % (shape, name, float((err / bound).max())))
        assert np.all(err <= bound), (name, float((err / bound).max()))


def test_constant_plane_gives_beta(ffi):
    """sigma^2 is exactly 0: the output is exactly beta, no NaN -- both regimes, zero and non-zero constants."""
    rng = np.random.default_rng(1)
    ga, be = _affine(rng, 256)
    for shape in ((2, 7, 7, 256), (1, 25, 42, 256)):
        for c in (0.0, 3.25, -1e6):
            got = ffi.group_norm(np.full(shape, c, np.float32), 32, ga, be)
            assert np.array_equal(got, np.broadcast_to(be, shape))


def test_nonfinite_stays_in_its_group(ffi):
    """A NaN or inf in one (image, group) reaches that group's outputs only; every other group keeps the clean run's bits."""
    rng = np.random.default_rng(2)
    ga, be = _affine(rng, 256)
    for shape in ((3, 14, 14, 256), (2, 25, 42, 256)):
        x = rng.standard_normal(shape).astype(np.float32)
        clean = ffi.group_norm(x, 32, ga, be)
        for bad in (np.nan, np.inf):
            y = x.copy()
            y[1, shape[1] // 2, 3, 8 * 5 + 2] = bad   # image 1, group 5
            got = ffi.group_norm(y, 32, ga, be)
            hit = np.zeros(shape, bool)
            hit[1, :, :, 40:48] = True
            assert np.array_equal(got[~hit], clean[~hit])
            assert not np.isfinite(got[hit]).any()


def test_two_runs_same_bits(ffi):
    rng = np.random.default_rng(3)
    ga, be = _affine(rng, 256)
    for shape in ((300, 7, 7, 256), (2, 50, 84, 256)):
        x = rng.standard_normal(shape).astype(np.float32)
        a = ffi.group_norm(x, 32, ga, be, relu=True)
        assert np.array_equal(a, ffi.group_norm(x, 32, ga, be, relu=True))


def test_bad_shapes_raise(ffi):
    z = np.zeros((1, 4, 4, 96), np.float32)
    with pytest.raises(ffi.IsegmiError):
        ffi.group_norm(z, 32, np.ones(96, np.float32), np.zeros(96, np.float32))          # 64-channel tiles do not divide 96
    with pytest.raises(ffi.IsegmiError):
        ffi.group_norm(z[..., :64], 5, np.ones(64, np.float32), np.zeros(64, np.float32))   # 5 groups do not divide 64
