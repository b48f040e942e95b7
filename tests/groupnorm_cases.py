"""The edge inputs of the GroupNorm kernels (TEST INFRASTRUCTURE ONLY), shared by tests/test_groupnorm_edges_gpu.py (kernel against the restatement, bit
for bit) and tests/test_groupnorm_cpu.py (the restatement against float64 inside the derived bound, at the same inputs): what the first file rests on is
checked by the second.  Geometry names as in csrc/groupnorm.hip: TW = min(C, 64), ncol = TW / 4, rows = 256 / ncol, a slab is H * W <= 196, a plane is
cut into chunks of rows * 32 pixels."""
import numpy as np

# C < 64: rows does not divide 256 evenly and the threads with r >= rows sit out (but join the barriers); both regimes
NARROW = [
    (2, 5, 7, 4, 1), (2, 5, 7, 4, 4),                # ncol 1, rows 256
    (2, 9, 11, 12, 4), (2, 9, 11, 12, 3),            # ncol 3, rows 85, one thread idle; cpg 3 and 4
    (1, 14, 14, 48, 3), (1, 14, 14, 48, 12),         # rows 21, 4 threads idle
    (2, 15, 15, 60, 15), (1, 15, 15, 60, 5),         # plane; rows 17, one thread idle
    (1, 23, 29, 36, 9),                              # plane
    (1, 40, 52, 20, 5),                              # plane, more than one chunk (rows 51: 1632 pixels)
    (1, 1, 8193, 4, 1),                              # chunk = 8192 pixels, + 1
]
# how groups lie inside a 64-channel tile and inside a thread's float4
LAYOUTS = [
    (1, 14, 14, 64, 64),                             # cpg 1: a float4 holds four groups
    (1, 15, 15, 64, 1),                              # the tile is one group
    (1, 15, 15, 128, 2),                             # cpg 64, two tiles
    (2, 7, 7, 256, 64), (2, 7, 7, 256, 4),
]
# C = 64, 32 groups, chunk = 512 pixels: 1 | 2 chunks, 2 | 3, 64 | 65 (the finalize's second lane iteration starts), 128 | 129
CHUNK_W = [511, 512, 513, 1024, 1025, 32768, 32769, 65536, 65537]
CHUNKS = [(1, 1, w, 64, 32) for w in CHUNK_W]

EPS_SHAPES = [(2, 7, 7, 256, 32), (1, 25, 42, 256, 32)]   # a slab and a plane
EPS = [1e-3, 1e-8, 0.0]


def seed_of(case):
    N, H, W, C, groups = case
    return N * 1000003 + H * 1009 + W * 31 + C * 7 + groups


def normal(case):
    """N(0.5, 2) data of the case's shape (non-constant in every group, so eps = 0 stays finite)."""
    rng = np.random.default_rng(seed_of(case))
    return (rng.standard_normal(case[:4]) * 2 + 0.5).astype(np.float32)


def signed_affine(C, seed=17):
    """gamma from [-1.5, 1.5] with every fifth element exactly 0, beta from N(0, 1)."""
    rng = np.random.default_rng(seed)
    ga = rng.uniform(-1.5, 1.5, C).astype(np.float32)
    ga[::5] = 0.0
    return ga, rng.standard_normal(C).astype(np.float32)


def outlier_pivot(shape, seed=23):
    """N(0, 1) data whose pivots (pixel 0, first channel of each of the 32 groups of 8) sit at 30 sigma."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    x[:, 0, 0, ::8] = 30.0
    return x
