"""The ViT operators and engine past the forks and grid caps of their launchers (csrc/vit_ops.hip), bit for bit against tests/vit_ref.py:
attention on both sides of the 4 -> 2 wavefront fork and at T = 1024, LayerNorm's slot geometry and row strides, GELU past one sweep of its capped grid,
class-softmax and patchify corners, and the engine at 576, 577 and 1024 tokens.  Each test that claims a path asserts the size inequality that reaches it."""
import functools

import numpy as np
import pytest

import spatial_cases as sc
import vit_ref as vr
from test_vit_cpu import tiny_cfg

gpu = pytest.mark.gpu
F = np.float32
POISON = np.uint32(0xFFFFFFFF)

# vit_attention_launch: 2560 staging floats and W score tiles of 16 x (Tc + 2) floats in at most 160 KiB of LDS
AT_STAGE, AT_LDS_MAX = 32 * 80, 160 * 1024


def attention_waves(T):
    """The launcher's rule: 4 wavefronts per workgroup until their four score tiles no longer fit the LDS, then 2."""
    Tc = -(-T // 32) * 32
    return 4 if (AT_STAGE + 4 * 16 * (Tc + 2)) * 4 <= AT_LDS_MAX else 2


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


def first_mismatch(got, want):
    bad = np.flatnonzero(u32(got).reshape(-1) != u32(want).reshape(-1))
    return "no mismatch" if bad.size == 0 else "%d of %d differ, first at flat index %d, last at %d" % (bad.size, got.size, bad[0], bad[-1])


# ---- 1. attention across its forks
def test_attention_wave_rule():
    """Host only: the two numbers the cases below stand on.  Whoever changes the staging size or the LDS limit revisits the T list."""
    assert (AT_STAGE + 4 * 16 * (576 + 2)) * 4 == 158208 and (AT_STAGE + 4 * 16 * (608 + 2)) * 4 == 166400
    assert attention_waves(576) == 4 and attention_waves(577) == 2
    assert [attention_waves(T) for T in (1, 49, 64, 65, 197, 593, 1023, 1024)] == [4, 4, 4, 4, 4, 2, 2, 2]
    assert (AT_STAGE + 2 * 16 * (1024 + 2)) * 4 <= AT_LDS_MAX          # the two-wavefront form fits at the kernel's maximum


@functools.lru_cache(maxsize=None)
def attention_case(T, heads=2, N=2):
    """(qkv, reference) of the random case at T, computed once and shared by the tests that need it; neither array is written to afterwards."""
    rng = np.random.default_rng(1000 * T + 10 * heads + N)
    qkv = rng.standard_normal((N, T, 3 * heads * 64)).astype(np.float32)
    want = vr.attention(qkv, heads)
    qkv.setflags(write=False); want.setflags(write=False)
    return qkv, want


def sentinel_attention(ffi, qkv, heads):
    # the buffer behind the last token holds 1e30: a padded key or query row read from memory would show in the max, the sum or as inf * 0
    return ffi.attention(qkv, heads, pad_floats=48 * 3 * heads * 64, pad_value=1e30)


# 49: wavefront 3 holds one live query; 64 / 65: a second workgroup starts on a full 64-query boundary with 0 / 1 queries; 576: the largest tile four wavefronts
# hold; 577: two wavefronts, the second of the last workgroup idle; 593 = 576 + 17: it has a single live query; 1023 / 1024: the last partial chunk and the maximum
@gpu
@pytest.mark.parametrize("T", [49, 64, 65, 576, 577, 593, 1023, 1024])
def test_attention_fork_bits(ffi, T):
    assert attention_waves(T) == (4 if T <= 576 else 2)
    qkv, want = attention_case(T)
    got = sentinel_attention(ffi, qkv, 2)
    assert bits_equal(got, want), (T, first_mismatch(got, want))


@gpu
def test_attention_sixteen_heads(ffi):
    """ViT-L's D = 1024: the head offset h * 64 up to 960 and the row pitch 3 D = 3072, with a second workgroup of one query."""
    qkv, want = attention_case(65, 16, 1)
    got = sentinel_attention(ffi, qkv, 16)
    assert bits_equal(got, want), first_mismatch(got, want)


@gpu
@pytest.mark.parametrize("T", [577, 1024])
def test_attention_crafted_rows_large(ffi, T):
    assert attention_waves(T) == 2
    rng = np.random.default_rng(T)
    heads, D = 2, 128
    # all scores equal: q = 0 -> s = 0, e = 1, l = T exactly (a sum of ones below 2^24), p = fl(1 / T): 2^-10 at T = 1024
    qkv = rng.standard_normal((1, T, 3 * D)).astype(np.float32)
    qkv[:, :, :D] = 0.0
    p, _ = vr.attention_head(qkv[0, :, 0:64], qkv[0, :, D:D + 64], qkv[0, :, 2 * D:2 * D + 64])
    assert np.array_equal(p, np.full((T, T), F(1.0) / F(T), np.float32))
    if T == 1024:
        assert p[0, 0] == 2.0 ** -10
    got, want = ffi.attention(qkv, heads), vr.attention(qkv, heads)
    assert bits_equal(got, want), first_mismatch(got, want)
    # one key dominant by more than 88: the others' dm_exp underflows to exactly 0 and every output row of head 0 is that key's v.  Index T - 1 is row 0
    # of chunk 18, the only live row of the last chunk (T = 577), or the last row of the last chunk (T = 1024); index 0 is the first row of the first
    for key in (T - 1, 0):
        qkv = (rng.standard_normal((1, T, 3 * D)) * 0.1).astype(np.float32)
        qkv[0, :, 0] = 32.0          # q[:, 0] (head 0)
        qkv[0, :, D] = 0.0
        qkv[0, key, D] = 32.0        # k[key, 0]: s = 128 + small, every other |s| < 1
        got, want = ffi.attention(qkv, heads), vr.attention(qkv, heads)
        assert bits_equal(got, want), (key, first_mismatch(got, want))
        assert np.array_equal(u32(got[0, :, :64]), u32(np.broadcast_to(qkv[0, key, 2 * D:2 * D + 64], (T, 64)))), key


@gpu
@pytest.mark.parametrize("T", [577, 1024])
def test_attention_wide_score_range(ffi, T):
    """q scaled until every row's scores span more than 150: most dm_exp arguments lie below -87.3 (results subnormal or exactly 0)."""
    rng = np.random.default_rng(7 * T)
    heads, D = 2, 128
    qkv = rng.standard_normal((1, T, 3 * D)).astype(np.float32)
    qkv[:, :, :D] *= F(48.0)
    s = np.einsum("hid,hjd->hij", *(qkv[0, :, w * D:(w + 1) * D].astype(np.float64).reshape(T, heads, 64).transpose(1, 0, 2) for w in (0, 1))) / 8
    R = s.max(-1) - s.min(-1)
    assert R.min() > 150, R.min()
    assert ((s - s.max(-1, keepdims=True)) < -87.3).mean() > 0.5
    got, want = ffi.attention(qkv, heads), vr.attention(qkv, heads)
    assert np.isfinite(want).all()
    assert bits_equal(got, want), first_mismatch(got, want)


@gpu
@pytest.mark.parametrize("T", [577, 1024])
def test_attention_device_against_float64(ffi, T):
    """The device's own output inside vit_ref.attention_bound (tests/test_vit_cpu.py holds the restatement to it and prints its margin: 0.0054 of the
    bound at T = 577, 0.0022 at 1024): redundant while the bits match; when they stop matching it tells a kernel that is merely ordered differently from
    one that is wrong."""
    qkv, _ = attention_case(T)
    got = ffi.attention(qkv, 2).astype(np.float64)
    want, bound = vr.attention_bound(qkv, 2)
    err = np.abs(got - want)
    print("device attention T=%d: max error / bound %.4f" % (T, (err / bound).max()))
    assert (err <= bound).all()


@gpu
def test_attention_repeat_launches_across_the_fork(ffi):
    """T = 577 (two wavefronts), T = 65 (four), T = 577 again: stale LDS or a stale function attribute would change the second result."""
    assert attention_waves(577) != attention_waves(65)
    big, want_big = attention_case(577)
    small, want_small = attention_case(65)
    a = sentinel_attention(ffi, big, 2)
    m = sentinel_attention(ffi, small, 2)
    b = sentinel_attention(ffi, big, 2)
    assert bits_equal(a, b), first_mismatch(a, b)
    assert bits_equal(a, want_big) and bits_equal(m, want_small)


# ---- 2. LayerNorm geometry
def ln_params(D, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, D).astype(np.float32), (rng.standard_normal(D) * 0.1).astype(np.float32)


# slots per row = D / 4: 1 (one lane works, K = x[0] is its own first element), 2, 63 / 64 / 65 (one slot either side of one slot per lane), 320 (ViT-H),
# 511 / 512 (the last lane's eighth slot missing / every lane full)
@gpu
@pytest.mark.parametrize("D", [4, 8, 252, 256, 260, 1280, 2044, 2048])
@pytest.mark.parametrize("rows", [1, 4, 9])
def test_layer_norm_geometry_bits(ffi, D, rows):
    rng = np.random.default_rng(10 * D + rows)
    x = rng.standard_normal((rows, D)).astype(np.float32)
    x[0] += 3000.0                            # |mean| >> sigma
    if rows > 2:
        x[2] = -7.5                           # a constant row
    ga, be = ln_params(D, D)
    want = vr.layer_norm(x, ga, be, 1e-6)
    got = ffi.layer_norm(x, ga, be, 1e-6)
    assert bits_equal(got, want), first_mismatch(got, want)
    got = ffi.layer_norm(x, ga, be, 1e-6, inplace=True)
    assert bits_equal(got, want), first_mismatch(got, want)
    if rows > 2:
        assert np.array_equal(want[2], be)


@gpu
@pytest.mark.parametrize("D", [4, 260, 2048])
def test_layer_norm_device_against_float64(ffi, D):
    """The device inside vit_ref.ln_bound on rows built as tests/test_vit_cpu.py::test_layer_norm_against_float64 builds them (the restatement stays
    under 0.2 of the bound at these widths)."""
    rng = np.random.default_rng(D)
    x = rng.standard_normal((7, D)).astype(np.float32)
    x[1] += 1000.0
    x[2] = x[2] * 1e-3 + 5.0
    ga, be = ln_params(D, D + 1)
    got = ffi.layer_norm(x, ga, be, 1e-6).astype(np.float64)
    err, bound = np.abs(got - vr.layer_norm_float64(x, ga, be, 1e-6)), vr.ln_bound(x, ga, be, 1e-6)
    print("device layer_norm D=%d: max error / bound %.3f" % (D, (err / bound).max()))
    assert (err <= bound).all()


@gpu
@pytest.mark.parametrize("D", [4, 260, 2048])
def test_layer_norm_row_strides(ffi, D):
    rows = 9
    rng = np.random.default_rng(D + 77)
    ga, be = ln_params(D, D + 2)
    # out of place, output rows D + 4 apart in a poisoned buffer: the four floats between two rows (and behind the last) keep the poison
    x = rng.standard_normal((rows, D)).astype(np.float32)
    x[0] += 3000.0
    got = ffi.layer_norm(x, ga, be, 1e-6, rows=rows, x_row_stride=D, out_row_stride=D + 4)
    assert got.shape == (rows, D + 4)
    assert bits_equal(got[:, :D], vr.layer_norm(x, ga, be, 1e-6)), first_mismatch(got[:, :D], vr.layer_norm(x, ga, be, 1e-6))
    assert (u32(got[:, D:]) == POISON).all()
    # in place, rows D + 8 apart: the eight floats between two rows keep their input bits
    buf = rng.standard_normal((rows, D + 8)).astype(np.float32)
    buf[2, :D] = -7.5
    got = ffi.layer_norm(buf, ga, be, 1e-6, inplace=True, rows=rows, x_row_stride=D + 8)
    want = vr.layer_norm(buf[:, :D], ga, be, 1e-6)
    assert got.shape == buf.shape and bits_equal(got[:, :D], want), first_mismatch(got[:, :D], want)
    assert np.array_equal(u32(got[:, D:]), u32(buf[:, D:]))


@gpu
def test_layer_norm_refusals_write_nothing(ffi):
    import ctypes as C
    R, cap = 4, 4096                                       # every buffer holds R rows of `cap` floats: more than any refused call could reach
    x = ffi.DeviceBuffer.from_numpy(np.random.default_rng(0).standard_normal((R, cap)).astype(np.float32))
    ga = ffi.DeviceBuffer.from_numpy(np.ones(cap, np.float32)); be = ffi.DeviceBuffer.from_numpy(np.zeros(cap, np.float32))
    out = ffi.DeviceBuffer((R, cap)).poison()
    call = ffi.lib().isegmi_op_layer_norm

    def off4(b):
        return C.c_void_p(b.ptr.value + 4)

    for match, args in (("multiple of 4 in 4..2048", (x.ptr, R, 2052, 2052, ga.ptr, be.ptr, 1e-6, out.ptr, 2052)),
                        ("multiple of 4 in 4..2048", (x.ptr, R, 0, 64, ga.ptr, be.ptr, 1e-6, out.ptr, 64)),
                        ("row strides", (x.ptr, R, 64, 60, ga.ptr, be.ptr, 1e-6, out.ptr, 64)),
                        ("row strides", (x.ptr, R, 64, 64, ga.ptr, be.ptr, 1e-6, out.ptr, 60)),
                        ("row strides", (x.ptr, R, 64, 66, ga.ptr, be.ptr, 1e-6, out.ptr, 64)),
                        ("row strides", (x.ptr, R, 64, 64, ga.ptr, be.ptr, 1e-6, out.ptr, 66)),
                        ("eps", (x.ptr, R, 64, 64, ga.ptr, be.ptr, -1.0, out.ptr, 64)),
                        ("eps", (x.ptr, R, 64, 64, ga.ptr, be.ptr, float("nan"), out.ptr, 64)),
                        ("16-byte aligned", (off4(x), R, 64, 64, ga.ptr, be.ptr, 1e-6, out.ptr, 64)),
                        ("16-byte aligned", (x.ptr, R, 64, 64, ga.ptr, be.ptr, 1e-6, off4(out), 64)),
                        ("16-byte aligned", (x.ptr, R, 64, 64, off4(ga), be.ptr, 1e-6, out.ptr, 64)),
                        ("16-byte aligned", (x.ptr, R, 64, 64, ga.ptr, off4(be), 1e-6, out.ptr, 64))):
        with pytest.raises(ffi.IsegmiError, match=match):
            ffi.check(call(*args, None))
    assert call(x.ptr, 0, 64, 64, ga.ptr, be.ptr, 1e-6, out.ptr, 64, None) == 0      # rows = 0: a successful no-op
    ffi.sync()
    assert (out.numpy().view(np.uint32) == POISON).all()
    assert call(x.ptr, R, 64, 64, ga.ptr, be.ptr, 1e-6, out.ptr, 64, None) == 0      # and the same arguments, accepted, do write
    ffi.sync()
    assert not (out.numpy().view(np.uint32)[0, :64] == POISON).any()


# ---- 3. GELU past the grid cap
GELU_N = 2 ** 23 + 2 ** 20 + 3        # 36 MiB: more than one sweep of CUs * 16 blocks * 256 threads * 4 floats on any device of up to 512 CUs, and a 3-float tail


@functools.lru_cache(maxsize=None)
def gelu_input():
    sweep = erf_points()
    x = (np.random.default_rng(31).standard_normal(GELU_N) * 3).astype(np.float32)
    for i0 in range(0, GELU_N - sweep.size, 1 << 16):      # the branch points in every part of the array, so also in every trip of the loop
        x[i0:i0 + sweep.size] = sweep
    x[-3:] = F([1.4142137, -2.8284273, 13.4])              # the tail: either side of dm_erf's |t| = 1 and 2 and past the erfc underflow
    x.setflags(write=False)
    return x


def erf_points():
    x = vr.erf_sweep()
    return x[np.abs(x) < 1e18]        # x^3 stays finite in the tanh form


@gpu
@pytest.mark.parametrize("gelu_tanh", [False, True])
def test_gelu_grid_stride(ffi, gelu_tanh):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = GELU_N
    assert cus * 16 * 1024 < n - 3                         # one sweep of the capped grid does not cover the array: the loop takes a second trip
    cap_items = cus * 16 * 256                             # float4 items of one sweep
    x = gelu_input()
    want = vr.gelu(x, gelu_tanh)
    for inplace in (False, True):
        got = ffi.gelu(x, gelu_tanh, inplace=inplace)
        if not bits_equal(got, want):
            bad = np.flatnonzero(u32(got) != u32(want))
            where = "n / 4 is a multiple of the sweep: no partial trip"
            if (n // 4) % cap_items:
                lo, hi = sc.grid_stride_tail(n // 4, 4, cap_items)
                where = "%d of them in the last, partial trip [%d, %d)" % (((bad >= lo) & (bad < hi)).sum(), lo, hi)
            pytest.fail("gelu(tanh=%d, inplace=%d): %d floats differ, first %d, last %d; %d past the first sweep (%d floats), %d in the 3-float tail; %s"
                        % (gelu_tanh, inplace, bad.size, bad[0], bad[-1], (bad >= cap_items * 4).sum(), cap_items * 4, (bad >= n - 3).sum(), where))


# ---- 4. class softmax and patchify corners
@gpu
def test_class_softmax_corners(ffi):
    rng = np.random.default_rng(12)
    one = (rng.standard_normal((3, 1)) * 50).astype(np.float32)
    assert np.array_equal(u32(ffi.class_softmax(one)), u32(np.ones((3, 1), np.float32)))          # n = 1: exp(0) / 1
    for rows, n in ((3, 63), (3, 128), (2, 21843)):        # one short of a wavefront, two full trips, ImageNet-21k (342 trips, the last of 19 lanes)
        x = (rng.standard_normal((rows, n)) * 4).astype(np.float32)
        x[rows - 1, n // 2] = 200.0                        # everything else underflows
        got, want = ffi.class_softmax(x), vr.class_softmax(x)
        assert bits_equal(got, want), (n, first_mismatch(got, want))
    x = np.full((2, 1000), F(-3.75))                       # all logits equal: every e is 1, every p the same
    got, want = ffi.class_softmax(x), vr.class_softmax(x)
    assert bits_equal(got, want) and (want == want[0, 0]).all() and want[0, 0] == F(1.0) / F(1000.0)


@gpu
def test_class_softmax_no_rows_and_aliasing(ffi):
    x = ffi.DeviceBuffer.from_numpy(np.zeros((2, 16), np.float32))
    out = ffi.DeviceBuffer((2, 16)).poison()
    call = ffi.lib().isegmi_op_class_softmax
    assert call(x.ptr, 0, 16, out.ptr, None) == 0
    ffi.sync()
    assert (out.numpy().view(np.uint32) == POISON).all()
    with pytest.raises(ffi.IsegmiError, match="prob == logits"):
        ffi.check(call(x.ptr, 2, 16, x.ptr, None))
    assert not x.numpy().any()


@gpu
@pytest.mark.parametrize("P,H,W,N", [(14, 28, 42, 2), (8, 8, 8, 1), (16, 16, 16, 3)])
def test_patchify_corners(ffi, P, H, W, N):
    """P = 14 (K = 588, no multiple of 32; the engine refuses it, the operator does not), a canvas of one patch, and one patch per image at N = 3."""
    x = np.random.default_rng(P + H + N).standard_normal((N, H, W, 3)).astype(np.float32)
    got, want = ffi.patchify(x, P), vr.patchify(x, P)
    assert want.shape == (N, H // P, W // P, P * P * 3) and bits_equal(got, want), first_mismatch(got, want)


# ---- 5. the engine at the token limit
EDGE_CANVASES = {(368, 400): 576, (384, 384): 577, (496, 528): 1024}


def test_edge_canvases_token_counts():
    """Host only: the canvases give the token counts the attention fork is tested at, and one patch row more is refused by name."""
    from isegmi.vit import ViT
    cfg = tiny_cfg()
    for (H, W), T in EDGE_CANVASES.items():
        assert cfg.validate(H, W).tokens(H, W) == T
    assert [attention_waves(T) for T in EDGE_CANVASES.values()] == [4, 2, 2]
    with pytest.raises(ValueError, match="1025 tokens"):
        ViT({}, cfg, 512, 512, max_batch=2)


@gpu
@pytest.mark.parametrize("canvas", list(EDGE_CANVASES))
def test_engine_at_token_limit(ffi, canvas):
    from isegmi.vit import ViT
    from isegmi.weights import vit_random_state_dict
    H, W = canvas
    T = EDGE_CANVASES[canvas]
    cfg = tiny_cfg()
    sd = vit_random_state_dict(cfg, 11, H, W)
    x = np.random.default_rng(H + W).uniform(-1, 1, (2, H, W, 3)).astype(np.float32)
    ref = vr.forward(sd, cfg, x)
    net = ViT(sd, cfg, H, W, max_batch=2)
    try:
        assert net.cfg.tokens(H, W) == T
        logits, prob, tv, ti = net(x)
        for name, a, b in (("logits", logits, ref["logits"]), ("prob", prob, ref["prob"]), ("topk_val", tv, ref["topk_val"])):
            assert bits_equal(a, b), (name, first_mismatch(a, b))
        assert np.array_equal(ti, ref["topk_idx"])
        for name, want in (("vit.attn", ref["blocks"][-1]["attn"]), ("vit.mlp", ref["blocks"][-1]["mlp"])):
            got = net.fetch(name, 2).reshape(2, T, -1)
            assert bits_equal(got, want), (name, first_mismatch(got, want))
        one = net(x[:1])                                   # batch 1 in the same engine: the same rows
        for a, b in zip(one, (logits, prob, tv, ti)):
            assert a.shape == b[:1].shape and np.array_equal(a.view(np.uint32), b[:1].view(np.uint32))
    finally:
        net.close()
