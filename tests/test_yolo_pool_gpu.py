"""isegmi_op_maxpool_darknet and isegmi_op_spp_concat (csrc/yolo_pool.hip) against the numpy pool of tests/yolo_variants_ref.py.  A maximum is
exact, so every comparison is np.array_equal; tests/test_yolo_variants_cpu.py shows with the reference alone what the pad fork, the window rule and the
NaN rule are."""

import numpy as np
import pytest

import yolo_variants_ref as vr

pytestmark = pytest.mark.gpu
F32 = np.float32
MAPS = ((1, 1), (1, 2), (2, 1), (2, 3), (5, 4), (13, 13), (19, 7))
POOLS = ((2, 2), (2, 1), (3, 2), (5, 1), (9, 1), (13, 1))   # (size, stride): odd maps under stride 2, maps smaller than the window
SPP_MAPS = ((1, 1), (2, 3), (7, 32), (13, 13), (19, 19), (32, 32))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _data(kind, shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, shape).astype(F32)
    if kind == "negative":
        return -np.abs(x) - F32(0.01)
    if kind == "special":   # a tenth of the values each NaN, +inf and -inf; on the small maps whole windows hold nothing else
        k = rng.integers(0, 10, shape)
        x[k == 0] = np.nan; x[k == 1] = np.inf; x[k == 2] = -np.inf
    return x


@pytest.mark.parametrize("pool", POOLS)
def test_maxpool_darknet(ffi, pool):
    size, stride = pool
    seed = 0
    for H, W in MAPS:
        for Cc in (4, 32, 36):
            for N in (1, 2):
                for kind in ("normal", "negative", "special"):
                    seed += 1
                    x = _data(kind, (N, H, W, Cc), seed)
                    for zp in (0, 1):
                        got, want = ffi.maxpool_darknet(x, size, stride, zp), vr.maxpool_darknet(x, size, stride, bool(zp))
                        assert got.shape == want.shape == (N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cc)
                        assert np.array_equal(got, want), (H, W, Cc, N, kind, zp)


def test_maxpool_darknet_is_maxpool_for_centred_windows(ffi):
    """zero_pad 0, stride 1, odd size: bit-identical to isegmi_op_maxpool(size, 1, size // 2), signs of zero included."""
    for H, W in ((5, 4), (13, 13), (1, 1)):
        for kind in ("normal", "special"):
            x = _data(kind, (2, H, W, 36), 100 + H)
            x[0, 0, 0, :4] = [0.0, -0.0, -0.0, 0.0]; x[-1, -1, -1, :4] = [-0.0, 0.0, -0.0, -1.0]
            for size in (1, 3, 5, 9, 13):
                assert np.array_equal(_bits(ffi.maxpool_darknet(x, size, 1, 0)), _bits(ffi.maxpool(x, size, 1, size // 2))), (H, W, kind, size)


def test_maxpool_darknet_refusals(ffi):
    x = ffi.DeviceBuffer.from_numpy(np.zeros((1, 4, 4, 8), F32))
    out = ffi.DeviceBuffer((1, 4, 4, 8))
    call = ffi.lib().isegmi_op_maxpool_darknet
    assert call(x.ptr, 1, 4, 4, 8, 2, 1, 0, out.ptr, None) == 0
    for match, args in (("null", (None, 1, 4, 4, 8, 2, 1, 0, out.ptr)), ("null", (x.ptr, 1, 4, 4, 8, 2, 1, 0, None)), ("multiple of 4", (x.ptr, 1, 4, 4, 6, 2, 1, 0, out.ptr)),
                        ("multiple of 4", (x.ptr, 1, 4, 4, 0, 2, 1, 0, out.ptr)), ("size must be 1..13", (x.ptr, 1, 4, 4, 8, 0, 1, 0, out.ptr)),
                        ("size must be 1..13", (x.ptr, 1, 4, 4, 8, 14, 1, 0, out.ptr)), ("stride must be 1 or 2", (x.ptr, 1, 4, 4, 8, 2, 0, 0, out.ptr)),
                        ("stride must be 1 or 2", (x.ptr, 1, 4, 4, 8, 2, 3, 0, out.ptr)), ("zero_pad", (x.ptr, 1, 4, 4, 8, 2, 1, 2, out.ptr)),
                        ("sizes", (x.ptr, 0, 4, 4, 8, 2, 1, 0, out.ptr)), ("sizes", (x.ptr, 1, 0, 4, 8, 2, 1, 0, out.ptr))):
        with pytest.raises(ffi.IsegmiError, match=match):
            ffi.check(call(*args, None))


@pytest.mark.parametrize("hw", SPP_MAPS)
def test_spp_concat(ffi, hw):
    """Against the three pools concatenated in numpy: the device pools (themselves held against the numpy pool above) at every size, the numpy pool where it is
    quick.  A block owns a slab of 16 channels (8 on 32 x 32, whose 16-channel plane does not fit in LDS): C 32 is two slabs (four), 512 is 32 (64), and
    N 3 puts the image index above the slab index."""
    H, W = hw
    for Cc in (32, 96, 512):
        for N in (1, 3):
            x = _data("special" if Cc == 96 else "normal", (N, H, W, Cc), H * 1000 + Cc + N)
            x[..., 1::2] = -np.abs(x[..., 1::2]) - F32(0.01)   # every other channel all negative (or NaN / inf): the pad modes differ there
            for zp in (0, 1):
                got = ffi.spp_concat(x, zp)
                assert got.shape == (N, H, W, 4 * Cc)
                assert np.array_equal(_bits(got[..., 3 * Cc:]), _bits(x)), (Cc, N, zp)   # the routed input itself, NaNs and all
                want = np.concatenate([ffi.maxpool_darknet(x, k, 1, zp) for k in (13, 9, 5)], -1)
                assert np.array_equal(got[..., :3 * Cc], want), (Cc, N, zp)
                if H * W * Cc * N <= 13 * 13 * 96 * 3:
                    assert np.array_equal(got, vr.spp_concat(x, bool(zp)), equal_nan=True), (Cc, N, zp)
            assert not np.array_equal(ffi.spp_concat(x, 0)[..., :3 * Cc], ffi.spp_concat(x, 1)[..., :3 * Cc])


def test_spp_concat_refusals(ffi):
    x = ffi.DeviceBuffer.from_numpy(np.zeros((1, 33, 32, 48), F32))
    out = ffi.DeviceBuffer((1, 33, 32, 4 * 48))
    call = ffi.lib().isegmi_op_spp_concat
    assert call(x.ptr, 1, 4, 4, 32, 0, out.ptr, None) == 0
    for match, args in (("1..32", (x.ptr, 1, 33, 32, 32, 0, out.ptr)), ("1..32", (x.ptr, 1, 32, 33, 32, 0, out.ptr)), ("1..32", (x.ptr, 1, 0, 4, 32, 0, out.ptr)),
                        ("multiple of 32", (x.ptr, 1, 4, 4, 48, 0, out.ptr)), ("multiple of 32", (x.ptr, 1, 4, 4, 0, 0, out.ptr)), ("null", (None, 1, 4, 4, 32, 0, out.ptr)),
                        ("null", (x.ptr, 1, 4, 4, 32, 0, None)), ("zero_pad", (x.ptr, 1, 4, 4, 32, 2, out.ptr)), ("1..32", (x.ptr, 0, 4, 4, 32, 0, out.ptr))):
        with pytest.raises(ffi.IsegmiError, match=match):
            ffi.check(call(*args, None))


# ---- past the launchers' forks: the capped grid of maxpool_darknet and the LDS fork of spp_concat
POOL_CAP_QUADS = 2048 * 256   # pool_grid: at most 2048 blocks of 256 threads, one channel quad of one output pixel per thread and trip
SPP_PLANE = 8192              # floats of one LDS plane of spp_concat_kernel: a 16-channel slab while H * W * 16 fits, an 8-channel slab past that
SPP_FORK_MAPS = ((22, 23), (16, 32), (23, 23), (1, 32), (32, 1))


@pytest.mark.parametrize("shape,pool", [((1, 130, 130, 128), (2, 1)), ((1, 259, 260, 128), (2, 2))])
def test_maxpool_darknet_grid_stride(ffi, shape, pool):
    """yolov3-tiny's two even pools on an output of 540 800 channel quads: 16 512 of them belong to the second trip of the grid-stride loop."""
    size, stride = pool
    N, H, W, Cc = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    quads = N * Ho * Wo * (Cc // 4)
    assert (Ho, Wo) == (130, 130) and POOL_CAP_QUADS < quads < 2 * POOL_CAP_QUADS
    for kind in ("special", "negative"):
        x = _data(kind, shape, H + len(kind))
        for zp in (0, 1):
            got, want = ffi.maxpool_darknet(x, size, stride, zp), vr.maxpool_darknet(x, size, stride, bool(zp))
            assert got.shape == want.shape == (N, Ho, Wo, Cc)
            bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
            assert bad.size == 0, "%s zero_pad %d: %d floats differ, first %d, last %d; %d of them past the first sweep (%d floats)" % (
                kind, zp, bad.size, bad[0], bad[-1], (bad >= POOL_CAP_QUADS * 4).sum(), POOL_CAP_QUADS * 4)
            if kind == "negative":   # the last output row's windows leave the map at the bottom: the pad modes differ there, inside the second trip
                assert (want[0, -1] == 0).all() == bool(zp) and (want[0, 0, :-1] < 0).all()


@pytest.mark.parametrize("hw", SPP_FORK_MAPS)
def test_spp_concat_lds_fork(ffi, hw):
    """Both sides of the slab fork at its boundary: 22 x 23 = 506 and 16 x 32 = 512 pixels (the last map on 16-channel slabs), 23 x 23 = 529 (the first on
    8-channel slabs), and the two one-pixel-wide maps, whose row or column pass sees a single line."""
    H, W = hw
    sixteen = H * W * 16 <= SPP_PLANE
    assert sixteen == (hw != (23, 23)) and (H * W * 16 == SPP_PLANE) == (hw == (16, 32)) and H * W * 8 <= SPP_PLANE
    for Cc in (32, 96):
        N = 2
        x = _data("special" if Cc == 96 else "normal", (N, H, W, Cc), H * 1000 + W * 10 + Cc)
        x[..., 1::2] = -np.abs(x[..., 1::2]) - F32(0.01)   # every other channel all negative (or NaN / inf): the pad modes differ there
        for zp in (0, 1):
            got, want = ffi.spp_concat(x, zp), vr.spp_concat(x, bool(zp))
            assert got.shape == want.shape == (N, H, W, 4 * Cc)
            assert np.array_equal(got, want, equal_nan=True), (Cc, zp)
            assert np.array_equal(_bits(got), _bits(want)), (Cc, zp)
            pools = np.concatenate([ffi.maxpool_darknet(x, k, 1, zp) for k in (13, 9, 5)], -1)
            assert np.array_equal(_bits(got[..., :3 * Cc]), _bits(pools)), (Cc, zp)
