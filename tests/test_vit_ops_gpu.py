"""The ViT operators of csrc/vit_ops.hip, each alone through its isegmi_op_* entry point, bit for bit against the restatements of tests/vit_ref.py."""
import numpy as np
import pytest

import vit_ref as vr
from vit_ref import erf_sweep

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- attention: T around the 16-row tile and the 32-key chunk, one and several heads and images (head addressing, image stride)
@pytest.mark.parametrize("T", [1, 15, 16, 17, 33, 197])
@pytest.mark.parametrize("heads,N", [(1, 1), (3, 2), (1, 2), (3, 1)])
def test_attention_bits(ffi, T, heads, N):
    rng = np.random.default_rng(1000 * T + 10 * heads + N)
    qkv = rng.standard_normal((N, T, 3 * heads * 64)).astype(np.float32)
    # the buffer behind the last token holds 1e30: a padded key or query row read from memory would show in the max, the sum or as inf * 0
    got = ffi.attention(qkv, heads, pad_floats=48 * 3 * heads * 64, pad_value=1e30)
    assert bits_equal(got, vr.attention(qkv, heads)), (T, heads, N)


def test_attention_crafted_rows(ffi):
    rng = np.random.default_rng(9)
    T, heads, D = 37, 2, 128
    # all scores equal: q = 0 -> s = 0, every p is exactly e / l with e = 1
    qkv = rng.standard_normal((1, T, 3 * D)).astype(np.float32)
    qkv[:, :, :D] = 0.0
    got = ffi.attention(qkv, heads)
    p, _ = vr.attention_head(qkv[0, :, 0:64], qkv[0, :, D:D + 64], qkv[0, :, 2 * D:2 * D + 64])
    assert np.array_equal(p, np.full((T, T), np.float32(1.0) / np.float32(T), np.float32))
    assert bits_equal(got, vr.attention(qkv, heads))
    # one key dominant by more than 88: the others' dm_exp underflows to exactly 0, the output row is that key's v
    qkv = (rng.standard_normal((1, T, 3 * D)) * 0.1).astype(np.float32)
    qkv[0, :, 0] = 32.0          # q[:, 0] (head 0)
    qkv[0, :, D] = 0.0
    qkv[0, 5, D] = 32.0          # k[5, 0]: s_i5 = 128 + small, every other |s| < 1
    got = ffi.attention(qkv, heads)
    assert bits_equal(got, vr.attention(qkv, heads))
    assert np.array_equal(got[0, :, :64], np.broadcast_to(qkv[0, 5, 2 * D:2 * D + 64], (T, 64)))
    # T = 1: the output is v
    one = rng.standard_normal((3, 1, 3 * D)).astype(np.float32)
    assert bits_equal(ffi.attention(one, heads), one[:, :, 2 * D:])


def test_attention_heads_are_independent(ffi):
    rng = np.random.default_rng(4)
    T, heads, D = 21, 3, 192
    a = rng.standard_normal((2, T, 3 * D)).astype(np.float32)
    b = a.copy()
    for w in range(3):                       # head 1 keeps its q, k, v; heads 0 and 2 get new ones
        for h in (0, 2):
            b[:, :, w * D + h * 64:w * D + h * 64 + 64] = rng.standard_normal((2, T, 64)).astype(np.float32)
    ga, gb = ffi.attention(a, heads), ffi.attention(b, heads)
    assert bits_equal(ga[:, :, 64:128], gb[:, :, 64:128]) and not np.array_equal(ga[:, :, :64], gb[:, :, :64])


def test_attention_refusals(ffi):
    with pytest.raises(ffi.IsegmiError, match="T <= 1024"):
        ffi.attention(np.zeros((1, 1025, 192), np.float32), 1)
    assert ffi.attention(np.zeros((0, 5, 192), np.float32), 1).shape == (0, 5, 64)


# ---- LayerNorm
@pytest.mark.parametrize("D", [32, 192, 768, 1024])
@pytest.mark.parametrize("rows", [1, 5, 197])
def test_layer_norm_bits(ffi, D, rows):
    rng = np.random.default_rng(D + rows)
    x = rng.standard_normal((rows, D)).astype(np.float32)
    x[0] += 3000.0                            # |mean| >> sigma
    if rows > 2:
        x[2] = -7.5                           # a constant row
    ga = rng.uniform(0.5, 1.5, D).astype(np.float32); be = (rng.standard_normal(D) * 0.1).astype(np.float32)
    want = vr.layer_norm(x, ga, be, 1e-6)
    assert bits_equal(ffi.layer_norm(x, ga, be, 1e-6), want)
    assert bits_equal(ffi.layer_norm(x, ga, be, 1e-6, inplace=True), want)
    if rows > 2:
        assert np.array_equal(want[2], be)
    assert bits_equal(ffi.layer_norm(x, ga, be, 1e-5), vr.layer_norm(x, ga, be, 1e-5))


def test_layer_norm_class_rows(ffi):
    """The strided form of the final norm: row n = token 0 of image n in [N][T][D]."""
    rng = np.random.default_rng(2)
    N, T, D = 3, 13, 192
    x = rng.standard_normal((N, T, D)).astype(np.float32)
    ga = rng.uniform(0.5, 1.5, D).astype(np.float32); be = (rng.standard_normal(D) * 0.1).astype(np.float32)
    got = ffi.layer_norm(x, ga, be, 1e-6, rows=N, x_row_stride=T * D)
    assert bits_equal(got, vr.layer_norm(x[:, 0], ga, be, 1e-6))
    with pytest.raises(ffi.IsegmiError, match="multiple of 4"):
        ffi.layer_norm(np.zeros((2, 30), np.float32), np.ones(30, np.float32), np.zeros(30, np.float32))


# ---- GELU
@pytest.mark.parametrize("gelu_tanh", [False, True])
def test_gelu_bits(ffi, gelu_tanh):
    x = erf_sweep()
    x = x[np.abs(x) < 1e18]
    rng = np.random.default_rng(8)
    for v in (x, (rng.standard_normal(4099) * 3).astype(np.float32), np.float32([0.5]), (rng.standard_normal(3) * 3).astype(np.float32)):
        assert v.size % 4 != 0 or v is x
        want = vr.gelu(v, gelu_tanh)
        assert bits_equal(ffi.gelu(v, gelu_tanh), want), v.size
        assert bits_equal(ffi.gelu(v, gelu_tanh, inplace=True), want), v.size


def test_erf_through_gelu_branch_points(ffi):
    """x * sqrt(1/2) lands on both sides of dm_erf's |t| = 1 and 2 branch points and past the erfc underflow."""
    x = np.float32([1.4142135, 1.4142137, 2.828427, 2.8284273, 13.3, 13.4, -13.4, -1.4142137, 1e-45, -0.0, 0.0])
    for tanh in (False, True):
        assert bits_equal(ffi.gelu(x, tanh), vr.gelu(x, tanh))


# ---- patchify, class softmax
@pytest.mark.parametrize("P,H,W", [(16, 32, 48), (32, 64, 32), (16, 16, 80), (32, 96, 64)])
def test_patchify(ffi, P, H, W):
    x = np.random.default_rng(P + H).standard_normal((2, H, W, 3)).astype(np.float32)
    assert bits_equal(ffi.patchify(x, P), vr.patchify(x, P))
    if H == 32:
        with pytest.raises(ffi.IsegmiError, match="multiples of P"):
            ffi.patchify(x, 14)


@pytest.mark.parametrize("n", [2, 10, 64, 65, 1000])
def test_class_softmax_bits(ffi, n):
    x = (np.random.default_rng(n).standard_normal((3, n)) * 4).astype(np.float32)
    x[1, 0] = 200.0            # everything else underflows
    assert bits_equal(ffi.class_softmax(x), vr.class_softmax(x))
