"""isegmi_op_paint (csrc/render.hip) against its numpy restatement (tests/render_ref.paint_ref), bit for bit: every image size class of the kernel's
thread layout (4 pixels per thread, 64 threads per row tile, 4 rows per block) on planes whose pitch and size put the plane bases on every byte
alignment, list lengths 0 .. the caps, every outline and dot form of the contract, in place and out of place, and every refusal.
The launcher has no grid cap (one block per 256 x 4 pixel tile, refused past the 1-D grid limit), so there is no capped-grid case."""
import numpy as np
import pytest

import render_ref as R

gpu = pytest.mark.gpu
ERR_ARG = -2
SIZES = [(1, 1), (2, 3), (5, 63), (4, 64), (3, 65), (7, 67),
         (9, 515)]   # (9, 515): three blocks along x and three along y, the last of each partial
SENTINEL = 0xA5
TAIL = 64


def run(ffi, image, masks, entries, dots, inplace=False, offset=0):
    rc, out, src = ffi.paint(image, masks, entries, dots, inplace=inplace, tail=TAIL, sentinel=SENTINEL, offset=offset)
    assert rc == 0, ffi.lib().isegmi_last_error()
    n = image.size
    assert (out[n:] == SENTINEL).all(), "bytes past H * W * 3 were written"
    if not inplace:
        assert np.array_equal(src, image.reshape(-1)), "a separate output must leave the input alone"
    return out[:n].reshape(image.shape)


def explain(got, want):
    bad = np.argwhere((got != want).any(2))
    return "%d pixels differ, first (y, x) = %s: got %s want %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


@gpu
@pytest.mark.parametrize("D", [0, 1, 2, 100, 1024])
@pytest.mark.parametrize("pw_extra", [0, 1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_overlapping_entries(ffi, H, W, pw_extra, D):
    image, masks, e, (cx, cy) = R.overlap_case(1000 * H + 10 * W + pw_extra + D, H, W, pw_extra, D)
    assert masks.shape[1] > H and masks.shape[2] == W + pw_extra and set(np.unique(masks)) <= {0, 1, 2, 255}
    if D >= 100:
        assert (e[:, 0] == -1).any() and len(set(e[:, 0].tolist())) == masks.shape[0] + 1 and (np.diff(e[:, 0]) < 0).any()   # -1 mixed in, every slot, out of order
    for k in range(D):   # every entry touches (cx, cy)
        s, x1, y1, x2, y2 = e[k, :5]
        assert (s >= 0 and masks[s, cy, cx]) or (e[k, 6] & 1 and x1 == cx and y1 <= cy <= y2)
    want = R.paint_ref(image, masks, e, [])
    got = run(ffi, image, masks, e, None)
    assert np.array_equal(got, want), explain(got, want)
    if D == 100:   # in place; and every base (image, planes, output) off the dword grid
        got = run(ffi, image, masks, e, None, inplace=True)
        assert np.array_equal(got, want), "in place: " + explain(got, want)
        for off in (1, 2, 3):
            got = run(ffi, image, masks, e, None, offset=off)
            assert np.array_equal(got, want), "offset %d: " % off + explain(got, want)


def test_plane_bases_cover_every_alignment():
    """what the pitches of test_overlapping_entries are for: over its cases the address of a 4-pixel group inside the planes takes every value mod 4"""
    seen = set()
    for H, W in SIZES:
        for extra in (0, 1, 3):
            ph, pw = R.plane_shape(H, W, extra)
            seen |= {(s * ph * pw + y * pw) % 4 for s in range(5) for y in range(H)}
    assert seen == {0, 1, 2, 3}


@gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_outlines(ffi, H, W):
    rng = np.random.default_rng(H + W)
    image = R.random_image(rng, H, W)
    forms = R.outline_entries(H, W)
    for name, ent in forms:
        want = R.paint_ref(image, None, [ent], [])
        got = run(ffi, image, None, ent[None], None)
        assert np.array_equal(got, want), name + ": " + explain(got, want)
    every = np.stack([ent for _, ent in forms])
    want = R.paint_ref(image, None, every, [])
    got = run(ffi, image, None, every, None, inplace=True)
    assert np.array_equal(got, want), explain(got, want)


@gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_dots(ffi, H, W):
    rng = np.random.default_rng(H * W)
    image = R.random_image(rng, H, W)
    for name, dots in R.dot_cases(H, W):
        want = R.paint_ref(image, None, [], dots)
        got = run(ffi, image, None, None, dots)
        assert np.array_equal(got, want), name + ": " + explain(got, want)


@gpu
@pytest.mark.parametrize("H,W,pw_extra", [(7, 67, 1), (3, 65, 0)])
def test_dot_list_at_its_cap_after_entries(ffi, H, W, pw_extra):
    image, masks, e, _ = R.overlap_case(5, H, W, pw_extra, 100)
    dots = R.many_dots(6, H, W, 32768)
    want = R.paint_ref(image, masks, e, dots)
    assert not np.array_equal(want, R.paint_ref(image, masks, e, []))
    got = run(ffi, image, masks, e, dots)
    assert np.array_equal(got, want), explain(got, want)
    again = run(ffi, image, masks, e, dots, inplace=True)       # a repeat launch, this time in place: identical bytes
    assert np.array_equal(again, got)
    assert np.array_equal(run(ffi, image, masks, e, dots), got)


@gpu
def test_empty_lists_copy_the_image(ffi):
    for H, W in SIZES:
        image = R.random_image(np.random.default_rng(W), H, W)
        assert np.array_equal(run(ffi, image, None, None, None), image)          # D = 0, Q = 0, no planes
        ph, pw = R.plane_shape(H, W, 1)
        assert np.array_equal(run(ffi, image, np.full((2, ph, pw), 255, np.uint8), None, None, inplace=True), image)


def refusals(H, W):
    """(name, keyword changes to a valid call) of every refusal of the contract"""
    ok_e = np.array([[1, 0, 0, W - 1, H - 1, 0x112233, 1, 0]], np.int32)
    ok_d = np.array([[0, 0, 0x445566, 2]], np.int32)

    def bad(a, col, v):   # a valid first row, the offending value in the second
        b = np.concatenate([a, a], 0)
        b[1, col] = v
        return b
    return ok_e, ok_d, [
        ("H < 1", dict(H=0)), ("W < 1", dict(W=0)), ("ph < H", dict(ph=H - 1)), ("pw < W", dict(pw=W - 1)),
        ("slot = slots", dict(entries=bad(ok_e, 0, 2))), ("slot < -1", dict(entries=bad(ok_e, 0, -2))),
        ("D over its cap", dict(entries=np.repeat(ok_e, 1025, 0))), ("Q over its cap", dict(dots=np.repeat(ok_d, 32769, 0))),
        ("half > 8", dict(dots=bad(ok_d, 3, 9))), ("half < 0", dict(dots=bad(ok_d, 3, -1))),
        ("masks with slots < 1", dict(slots=0)), ("a slot without masks", dict(masks=None)),
        ("null image", dict(image=None)), ("null output", dict(out=None)),
    ]


@gpu
def test_refusals_launch_nothing(ffi):
    H, W = 5, 63
    ph, pw = R.plane_shape(H, W, 1)
    ok_e, ok_d, cases = refusals(H, W)
    lib = ffi.lib()
    d_img = ffi.DeviceBuffer.from_numpy(R.random_image(np.random.default_rng(0), H, W))
    d_m = ffi.DeviceBuffer.from_numpy(np.ones((2, ph, pw), np.uint8))
    d_out = ffi.DeviceBuffer((H * W * 3,), np.uint8)
    fill = np.full(H * W * 3, SENTINEL, np.uint8)
    d_out.upload(fill)

    def call(image=d_img, masks=d_m, entries=ok_e, dots=ok_d, out=d_out, **kw):
        a = dict(H=H, W=W, slots=2, ph=ph, pw=pw); a.update(kw)
        de, dd = ffi.DeviceBuffer.from_numpy(entries), ffi.DeviceBuffer.from_numpy(dots)
        rc = lib.isegmi_op_paint(ffi._ptr(image), a["H"], a["W"], ffi._ptr(masks), a["slots"], a["ph"], a["pw"], de.ptr, len(entries), dd.ptr, len(dots),
                                 ffi._ptr(out), None)
        ffi.sync()
        return rc
    assert len(cases) == 14
    for name, kw in cases:
        assert call(**kw) == ERR_ARG, name
        assert b"paint" in lib.isegmi_last_error(), name
        assert np.array_equal(d_out.numpy(), fill), name + ": the refused call wrote"
    # a list that is not empty and has no pointer
    assert lib.isegmi_op_paint(d_img.ptr, H, W, d_m.ptr, 2, ph, pw, None, 1, None, 0, d_out.ptr, None) == ERR_ARG
    assert lib.isegmi_op_paint(d_img.ptr, H, W, d_m.ptr, 2, ph, pw, None, 0, None, 1, d_out.ptr, None) == ERR_ARG
    ffi.sync()
    assert np.array_equal(d_out.numpy(), fill)
    assert call() == 0 and not np.array_equal(d_out.numpy(), fill)          # and the valid call the refusals were derived from paints
