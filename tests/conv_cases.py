"""The shapes, tile lists and the one skip rule shared by tests/test_conv_exact_gpu.py, tests/test_conv_edges_gpu.py (kernels against the references
of tests/conv_ref.py) and tests/test_conv_ref_cpu.py (the CPU oracle against the same references at the very same shapes, and the table test of the
skip rule).  A case is (N, H, W, Cin, Cout, R, stride, pad)."""
import zlib

import numpy as np


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def out_hw(case):
    N, H, W, Cin, Cout, R, stride, pad = case
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def k_of(case):
    return case[5] * case[5] * case[3]


def m_of(case):
    ho, wo = out_hw(case)
    return case[0] * ho * wo


# ---------------------------------------------------------------- fp16 tiles (the ids the switch of conv2d_f16_launch_impl accepts)
FEW = 2048                                   # test hook of the persistent kernels: an 8-block grid, so blocks walk several tiles
F16_GENERIC = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 20]
F16_STRIP = [26, 27, 28, 29, 30, 31]
F16_PERSIST = [32, 34, 37, 39]
F16_M16_STRIP = [40, 41]
F16_M16_PERSIST = [44, 46, 47, 49]
F16_TILES = ([0] + F16_GENERIC + F16_STRIP + F16_PERSIST + [FEW + t for t in F16_PERSIST] + F16_M16_STRIP + F16_M16_PERSIST
             + [FEW + t for t in F16_M16_PERSIST])
# rows of output pixels per block
F16_BM = {1: 256, 2: 256, 3: 128, 4: 64, 5: 64, 6: 64, 7: 128, 8: 128, 9: 192, 10: 192, 11: 160, 12: 192, 13: 256, 14: 256, 16: 160, 17: 192, 19: 128,
          20: 192, 26: 192, 27: 256, 28: 160, 29: 192, 30: 192, 31: 192, 32: 192, 34: 256, 37: 192, 39: 128, 40: 192, 41: 144, 44: 256, 46: 144, 47: 192,
          49: 128}
# output channels per block of the persistent tiles
F16_PERSIST_BN = {32: 256, 34: 128, 37: 256, 39: 256, 44: 128, 46: 256, 47: 256, 49: 256}
# one tile of each family, for the checks that need a family and not every member
F16_FAMILY = {"generic": 4, "generic_lw": 17, "strip": 30, "persistent": 37, "persistent_few": FEW + 39, "m16_strip": 40, "m16_persistent": FEW + 46, "auto": 0}

# fp32 tiles: those of test_conv_bit_exact (13 / 14 are the hybrid launches) + 15, the fixed-tree split-K
F32_TILES = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 13, 14, 15]


def f16_refused(tile, case):
    """THE skip rule: the reason the launcher's own ARG_CHECK refuses (tile, case), or None when the pair runs.  Strip tiles are 3x3 / stride 1 / pad 1
    only and cut a tile of BM rows into at most 32 image-row segments ((BM - 1) / W + 2 <= 32); every fp16 conv needs Cin % 64 == 0."""
    N, H, W, Cin, Cout, R, stride, pad = case
    if Cin % 64:
        return "Cin % 64"
    t = tile & 255
    if t in F16_STRIP or t in F16_M16_STRIP:
        if not (R == 3 and stride == 1 and pad == 1):
            return "strip tiles are 3x3 / stride 1 / pad 1 only"
        if (F16_BM[t] - 1) // W + 2 > 32:
            return "strip tile: more than 32 image-row segments"
    return None


# ---------------------------------------------------------------- the cases of the exact file
# the cases of tests/test_conv_f16_gpu.py.  The persistent kernels split cdiv(M, BM) x cdiv(Cout, BN) tiles over the 8 XCDs: (1, 30, 300, 64, 256) gives
# 47 tiles of 192 x 256 and 71 of 128 x 256, (40, 9, 9, 64, 256) 26 of 256 x 128 -- more than 8 and not a multiple of it, so the split has a remainder and,
# under + 2048 (an 8-block grid), every block walks several tiles (tests/test_conv_ref_cpu.py asserts it for every persistent tile)
BASE = [(2, 19, 23, 64, 48, 3, 1, 1), (3, 14, 14, 128, 96, 3, 1, 1), (1, 30, 300, 64, 256, 3, 1, 1), (40, 9, 9, 64, 256, 3, 1, 1),
        (64, 7, 8, 64, 256, 3, 1, 1), (1, 35, 35, 64, 64, 1, 1, 0), (2, 35, 33, 128, 128, 3, 2, 1), (1, 18, 18, 256, 405, 1, 1, 0),
        (1, 7, 7, 256, 1024, 7, 1, 0), (1, 40, 56, 256, 256, 3, 1, 1)]
# res4 / res5 / FPN-lateral depths
DEEP_CIN = [(1, 14, 15, 512, 128, 3, 1, 1), (1, 20, 30, 1024, 256, 1, 1, 0), (1, 13, 21, 2048, 256, 1, 1, 0), (2, 14, 14, 512, 136, 1, 2, 0)]
# Cout below / at / above one 8-channel vector, ragged Cout under a 3x3 and under stride 2 (per-element epilogue)
NARROW = [(2, 20, 20, 64, 1, 3, 1, 1), (2, 11, 12, 64, 7, 3, 1, 1), (1, 12, 12, 64, 8, 1, 1, 0), (1, 21, 23, 128, 9, 3, 2, 1), (1, 16, 16, 64, 15, 1, 1, 0)]
# W = 1, 2, 8 (a 3x3 whose every tap but the centre column is padding; W = 8: below the strip tiles' W >= 9 of the old test), H = 1
THIN = [(2, 40, 1, 64, 32, 3, 1, 1), (2, 24, 2, 64, 32, 3, 1, 1), (3, 10, 8, 64, 40, 3, 1, 1), (1, 1, 70, 64, 32, 3, 1, 1)]
EXACT_CASES = BASE + DEEP_CIN + NARROW + THIN
# the shallow case that gets a large integer shift, so that its fp16 results pass 2048 and the store has to round
BIG_SHIFT_CASE = (1, 35, 35, 64, 64, 1, 1, 0)
BIG_SHIFT_CASE_3X3 = (2, 19, 23, 64, 48, 3, 1, 1)   # the same for the strip tiles, which refuse a 1x1
# M just below / at / above every BM of the table: one image row of M pixels under a 3x3 (every tile family runs it)
BM_EDGES = [m + d for m in (64, 128, 144, 160, 192, 256) for d in (-1, 0, 1)]


def bm_edge_case(M):
    return (1, 1, M, 64, 24, 3, 1, 1)


DEEP_K = 2304   # from here on the order-free results must pass 2048

# ---------------------------------------------------------------- the cases of the edges file (bound + RMS): a smaller set that holds the deep ones
# K = 4608 (every tile, the strip ones included), 12544 and 2048 (the rest)
EDGE_CASES = [(1, 14, 15, 512, 128, 3, 1, 1), (1, 7, 7, 256, 1024, 7, 1, 0), (1, 13, 21, 2048, 256, 1, 1, 0), (2, 19, 23, 64, 48, 3, 1, 1),
              (2, 35, 33, 128, 128, 3, 2, 1), (1, 21, 23, 128, 9, 3, 2, 1)]

# fp32 kernels: Cin % 32 == 0 (or the Cin = 4 stem); the cases of tests/test_conv_gpu.py and a few of the above
F32_CASES = [(2, 19, 23, 32, 48, 3, 1, 1), (1, 35, 35, 64, 64, 1, 1, 0), (2, 35, 33, 64, 128, 3, 2, 1), (1, 18, 18, 256, 243, 3, 1, 1), (3, 9, 9, 128, 12, 3, 1, 1),
             (1, 40, 56, 256, 256, 1, 2, 0), (1, 7, 7, 256, 1024, 7, 1, 0), (1, 13, 21, 2048, 256, 1, 1, 0), (2, 11, 12, 64, 7, 3, 1, 1), (2, 40, 1, 64, 32, 3, 1, 1)]
# the hybrid launches (13 / 14) split only when the 64 x 64 grid is larger than the chip: two of HYBRID_CASES of tests/test_conv_gpu.py
F32_HYBRID_CASES = [(1, 150, 150, 64, 128, 3, 1, 1), (3, 83, 79, 32, 200, 1, 1, 0)]

# ---------------------------------------------------------------- fused kernels
BOTTLENECK_SHAPES = [(1, 8, 16), (1, 5, 9), (2, 19, 37), (1, 24, 48), (3, 33, 30), (1, 50, 84), (2, 9, 61)]   # SHAPES of tests/test_bottleneck_f16_gpu.py
BOTTLENECK_CH = [(256, 64), (512, 128)]
# (N, H, W): odd and even sizes, sizes below one tile / one strip, several images
STEM_SHAPES = [(1, 32, 32), (2, 50, 70), (1, 37, 45), (1, 64, 33), (3, 33, 64), (2, 17, 9), (1, 5, 5), (1, 123, 251)]
# lateral + nearest-2x add: (N, H, W, Cin, Hc, Wc).  Odd H / W read the clamped coarse pixel in the last row / column; (Hc, Wc) at both ends of what the
# launcher admits ((H + 1) / 2 <= Hc + 1): one below the half size (the clamp is what keeps the read inside) and above it
MERGE_CASES = [(2, 51, 85, 256, 26, 43), (1, 51, 85, 256, 25, 42), (1, 50, 84, 512, 25, 42), (1, 50, 84, 256, 24, 41), (1, 13, 21, 2048, 7, 11),
               (3, 25, 42, 1024, 13, 21), (1, 26, 9, 256, 20, 8), (1, 100, 168, 256, 50, 84),
               # W = 8, the narrowest the launcher admits; and 350 tiles of 192 rows on 256 blocks: blocks walk a second tile, the residual walk crosses it
               (1, 30, 8, 256, 15, 4), (2, 200, 168, 256, 100, 84)]
# 3x3 + fused 1x1 head: fused from 128 tiles of 192 rows on (N * H * W > 127 * 192)
HEAD_CASES = [(2, 100, 168, 256, 15), (1, 131, 197, 256, 3), (3, 67, 141, 256, 32), (1, 160, 155, 64, 12)]


def _self_check():
    assert len(set(EXACT_CASES)) == len(EXACT_CASES)
    assert all(c[3] % 64 == 0 for c in EXACT_CASES + EDGE_CASES)
    assert all(c[3] % 32 == 0 for c in F32_CASES + F32_HYBRID_CASES)
    assert all(np.prod(c[:3]) > 0 for c in EXACT_CASES)


_self_check()
