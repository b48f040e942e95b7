"""isegmi_op_resample_u8 against tests/resample_ref.py (PIL's 8-bit bilinear resize restated), bit for bit.  Both outputs are poisoned
before every launch (fp32: NaN; bytes: 255), so an element the kernel never wrote cannot pass.  The kernel owns TILE_H x TILE_W output tiles and streams
source rows through LDS CHUNK rows at a time: the shapes below sit on both sides of each of the three."""
import numpy as np
import pytest

import resample_ref as rr

pytestmark = pytest.mark.gpu
TILE_H, TILE_W, CHUNK = 16, 64, 32
PIXEL_MEAN = (102.9801, 115.9465, 122.7717)


def test_tile_constants(ffi):
    assert ffi.resample_tile() == (TILE_H, TILE_W, CHUNK)


def run_u8(ffi, images, entries):
    got = ffi.resample_u8(images, entries)
    for g, (i, oh, ow, _, _, flip, _) in zip(got, entries):
        want = rr.resize_view(images[i], oh, ow, bool(flip))
        assert g.shape == want.shape
        assert np.array_equal(g, want), ((i, oh, ow, flip), int((g != want).sum()), np.argwhere(g != want)[:4].tolist())


@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_contract_shapes_all_patterns_one_launch(ffi, shape):
    """all-255 (the accumulator's maximum and the clip), the 0 / 255 board and random bytes, three images in one launch"""
    h, w, oh, ow = shape
    ims = list(rr.patterns(h, w, seed=h + w).values())
    run_u8(ffi, ims, [(i, oh, ow, 0, 0, 0, 0) for i in range(3)])


def test_identity_and_largest_downscale(ffi):
    p = rr.patterns(37, 53, 1)
    big = rr.patterns(1024, 512, 2)   # 512 x in both axes: ksize 1025, the cap; 33 LDS chunks for the one tile
    ims = [p["random"], p["board"], big["random"], big["ones"], big["board"]]
    run_u8(ffi, ims, [(0, 37, 53, 0, 0, 0, 0), (1, 37, 53, 0, 0, 1, 0), (2, 2, 1, 0, 0, 0, 0), (3, 2, 1, 0, 0, 0, 0), (4, 2, 1, 0, 0, 0, 0),
                      (2, 1024, 1, 0, 0, 0, 0), (2, 2, 512, 0, 0, 0, 0)])   # and one axis identity, the other at the cap
    with pytest.raises(ValueError, match="within 512"):
        ffi.resample_u8([big["random"]], [(0, 1, 1, 0, 0, 0, 0)])


def test_output_sizes_around_the_tile(ffi):
    """heights tile - 1, tile, tile + 1, 2 tile + 1 times the same four widths, up- and downscaled from one odd-sized source, 16 views in one launch;
    then the same through the fp32 epilogue, where NaN marks anything unwritten"""
    im = rr.patterns(23, 91, 5)["random"]
    sizes = [(oh, ow) for oh in (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1) for ow in (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1)]
    run_u8(ffi, [im], [(0, oh, ow, 0, 0, 0, 0) for oh, ow in sizes])
    Hp, Wp = 2 * TILE_H + 1, 2 * TILE_W + 1
    got = ffi.resample_u8([im], [(0, oh, ow, 0, 0, 0, k) for k, (oh, ow) in enumerate(sizes)], canvas=(Hp, Wp), fill=-3.0)
    for k, (oh, ow) in enumerate(sizes):
        assert np.array_equal(rr.bits(got[k]), rr.bits(rr.canvas_f32(im, oh, ow, Hp, Wp, fill=-3.0))), (oh, ow)


@pytest.mark.parametrize("hin", [20, 39, 40, 60, 100, 137])
def test_source_rows_across_lds_chunks(ffi, hin):
    """20 output rows (a full tile and a partial one); the first tile reads source rows bounds[0].min .. bounds[15].min + n: 17 (one chunk), 32 (one,
    full), 33 (two, by one row), 50 (two), 83 (three), 113 (four)"""
    ims = list(rr.patterns(hin, 45, hin).values())
    b, _ = rr.coeffs(hin, 20)
    rows = int(b[TILE_H - 1, 0] + b[TILE_H - 1, 1] - b[0, 0])
    assert (rows, -(-rows // CHUNK)) == {20: (17, 1), 39: (32, 1), 40: (33, 2), 60: (50, 2), 100: (83, 3), 137: (113, 4)}[hin], rows
    run_u8(ffi, ims, [(i, 20, 30, 0, 0, 0, 0) for i in range(3)] + [(2, 20, 70, 0, 0, 1, 0)])


def test_three_sizes_at_unaligned_source_offsets(ffi):
    """A 9-byte image in front puts the three at byte offsets 9, 114 and 411 (1, 2 and 3 mod 4) with rows of 21, 33 and 39 bytes (Win * 3 odd)"""
    rng = np.random.default_rng(9)
    ims = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((1, 3), (5, 7), (9, 11), (21, 13))]
    offs = np.cumsum([0] + [im.size for im in ims])[1:4]
    assert [int(o) % 4 for o in offs] == [1, 2, 3] and all(im.shape[1] * 3 % 2 for im in ims)
    run_u8(ffi, ims, [(1, 13, 11, 0, 0, 0, 0), (2, 4, 70, 0, 0, 0, 0), (3, 40, 5, 0, 0, 1, 0)])
    got = ffi.resample_u8(ims, [(1, 13, 11, 2, 3, 0, 0), (2, 4, 70, 0, 1, 1, 1), (3, 40, 5, 0, 0, 0, 2)], canvas=(48, 96), mean3=PIXEL_MEAN, fill=0.0)
    for k, (i, oh, ow, dy, dx, flip) in enumerate(((1, 13, 11, 2, 3, False), (2, 4, 70, 0, 1, True), (3, 40, 5, 0, 0, False))):
        assert np.array_equal(rr.bits(got[k]), rr.bits(rr.canvas_f32(ims[i], oh, ow, 48, 96, dy, dx, PIXEL_MEAN, hflip=flip))), k


@pytest.mark.parametrize("ow", [53, 29, 90, 11, 64, 65])
def test_hflip_mirrors_the_resized_image(ffi, ow):
    """Output column x shows column Wout - 1 - x of the RESIZED image (upstream's order), mirrored within the image and not within the canvas.
    The issue asked for a view on which mirror-then-resize differs from resize-then-mirror in the restatement, so that only this order could pass.  There
    is none to pick: PIL's bilinear tables are mirror-symmetric as integers for every axis I, O < 400 (searched exhaustively on the CPU;
    tests/test_resample_cpu.py keeps the small range and the model sizes), so the two orders coincide bit for bit.  What is asserted is the stated order;
    the mirror's extent is pinned by a canvas wider than the image and a dst_x that is not centred."""
    im = rr.patterns(19, 37, 77)["random"]
    oh = 25
    (got,) = ffi.resample_u8([im], [(0, oh, ow, 0, 0, 1, 0)])
    assert np.array_equal(got, rr.resize_view(im, oh, ow, True)) and not np.array_equal(got, rr.resize_view(im, oh, ow, False))
    f = ffi.resample_u8([im], [(0, oh, ow, 1, 2, 1, 0)], canvas=(32, 96), mean3=PIXEL_MEAN)
    assert np.array_equal(rr.bits(f[0]), rr.bits(rr.canvas_f32(im, oh, ow, 32, 96, 1, 2, PIXEL_MEAN, hflip=True)))


@pytest.mark.parametrize("model", ["maskrcnn", "yolo"])
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("fill", [0.0, 0.5])
def test_fp32_epilogue(ffi, model, swap, fill):
    """Two images on two planes of one canvas that is neither a multiple of the tile nor filled by either image: padding on the right and at the bottom
    (dst 0, 0: to_image_list) and all round (dst in the middle: the letterbox), both mean / std pairs, the channel swap, both fills."""
    mean, std = (PIXEL_MEAN, (1.0, 1.0, 1.0)) if model == "maskrcnn" else ((0.0, 0.0, 0.0), (255.0, 255.0, 255.0))
    ims = [rr.patterns(30, 41, 3)["random"], rr.patterns(50, 20, 4)["board"], rr.patterns(8, 8, 5)["ones"]]
    Hp, Wp = 70, 150
    entries = [(0, 45, 61, 0, 0, 0, 0), (1, 66, 26, 4, 62, 0, 1), (2, 70, 150, 0, 0, 0, 2), (2, 1, 1, 69, 149, 0, 3)]
    got = ffi.resample_u8(ims, entries, canvas=(Hp, Wp), mean3=mean, std3=std, swap_rb=swap, fill=fill)
    assert got.shape == (4, Hp, Wp, 3) and not np.isnan(got).any()
    for k, (i, oh, ow, dy, dx, _, _) in enumerate(entries):
        want = rr.canvas_f32(ims[i], oh, ow, Hp, Wp, dy, dx, mean, std, swap, fill)
        assert np.array_equal(rr.bits(got[k]), rr.bits(want)), (k, np.argwhere(rr.bits(got[k]) != rr.bits(want))[:4].tolist())


def test_the_table_is_validated_before_the_launch(ffi):
    """An image outside its canvas, a plane past the planes: refused by name, nothing launched."""
    im = rr.patterns(8, 8, 1)["random"]
    for entries, kw, word in (([(0, 16, 16, 1, 0, 0, 0)], dict(canvas=(16, 16)), "outside the canvas"),
                              ([(0, 16, 16, 0, 0, 0, 2)], dict(canvas=(16, 16), planes=2), "outside the canvas")):
        with pytest.raises(ffi.IsegmiError, match=word):
            ffi.resample_u8([im], entries, **kw)
