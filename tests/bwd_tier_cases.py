"""Cases of the backward kernel families (include/swinfuse.h swf_bwd_options): the shapes of the per-layer seam swf_linear_bwd with
their float64 references and a-priori error bounds, and the module shapes on which the matrix-core gradient GEMMs are held bit-equal to
the scalar-FMA family (tests/test_gpu_backward_tier.py; the option and attribute plumbing: tests/test_backward_tier_host.py)."""
import functools

import torch

from tests import golden_util as G

# (M, N, K) of y = x W^T + b: x [M][K], W [N][K], dY [M][N]
LINEAR_SHAPES = [
    (1, 1, 1),          # smallest
    (63, 3, 5),         # every edge at once, the reduction padded up to the instruction's k-step
    (65, 4, 24),        # the decoder's hidden width 4
    (196, 24, 96),      # a map of 7x7 windows
    (255, 96, 24),      # the 256-token chunk boundary of the weight gradient: below,
    (256, 96, 24),      # at,
    (257, 96, 24),      # above (a second chunk of one token)
    (515, 40, 16),      # three chunks
    (128, 192, 768),    # deep widths (level 3)
    (64, 1536, 384),    # deep widths (level 4), 24 x 6 output tiles
    (8451, 5, 3),       # 34 chunks: reduce_rows takes a second level
]
OFFSET_SHAPE = (196, 24, 96)   # run once more with every pointer 4 bytes off a 16-byte boundary (the scalar-load path at vector widths)

EPS = 2.0 ** -24   # unit roundoff of fp32


def shape_id(s):
    return "M%d_N%d_K%d" % s


@functools.lru_cache(maxsize=None)
def linear_inputs(shape):
    """x, W, dY and a prior content of dX (for accumulate), fp32 on the CPU; unchanged by the tests."""
    m, n, k = shape
    seed = 9000 + 7 * m + 3 * n + k
    return G.randn((m, k), seed), G.randn((n, k), seed + 1), G.randn((m, n), seed + 2), G.randn((m, k), seed + 3)


@functools.lru_cache(maxsize=None)
def linear_reference(shape):
    """float64 dX, dW, db and the elementwise a-priori bounds of an fp32 fmaf chain over the reduction index: a chain of L products has
    at most L roundings, the chunk tree of dW / db adds fewer levels than it removes chain steps, so
      |dX err| <= (N + 2) eps |dY| |W|,   |dW err| <= (M + 2) eps |dY|^T |X|,   |db err| <= (M + 2) eps sum |dY|."""
    m, n, k = shape
    x, w, dy, _ = (t.double() for t in linear_inputs(shape))
    ref = {"dx": dy @ w, "dw": dy.t() @ x, "db": dy.sum(0)}
    bound = {"dx": (n + 2) * EPS * (dy.abs() @ w.abs()), "dw": (m + 2) * EPS * (dy.abs().t() @ x.abs()), "db": (m + 2) * EPS * dy.abs().sum(0)}
    return ref, bound


# The eight block shapes of tests/test_gpu_backward.py::_CASES: C, heads, d, win, hidden, (B,H,W), shift, cross, dual
BLOCK_CASES = [
    (8, 2, 4, 4, 32, (2, 8, 12), True, True, True),
    (8, 2, 4, 4, 12, (1, 8, 8), False, False, True),
    (24, 8, 3, 8, 96, (1, 16, 16), True, False, True),
    (24, 8, 3, 8, 4, (1, 8, 16), True, True, True),
    (12, 4, 3, 7, 24, (1, 14, 14), True, True, True),
    (16, 2, 8, 4, 40, (2, 8, 8), True, False, False),
    (48, 8, 6, 8, 192, (1, 8, 8), True, True, True),
    (8, 2, 4, 16, 16, (1, 16, 32), True, True, True),         # 16x16 windows: the recompute attention kernel
]
BLOCK_DROP_CASE = (24, 8, 3, 8, 96, (1, 16, 16), True, True, True)   # shifted cross block, all three dropout ratios 0.1


def block_id(c):
    return f"C{c[0]}_w{c[3]}_hid{c[4]}_s{int(c[6])}c{int(c[7])}d{int(c[8])}"


# gradient-GEMM launches of one block backward per stream: dX of fc2, fc1, proj, q, k, v; dW of the same six layers
BLOCK_DX_PER_STREAM = BLOCK_DW_PER_STREAM = 6

# WindowAttention on its own: the five shapes of tests/test_gpu_backward.py::_WA_CASES (C, heads, d, win, (B,H,W), shift, mode, qkv bias)
WA_CASES = [
    (24, 8, 3, 8, (1, 16, 16), True, "self", True),
    (24, 8, 3, 8, (2, 8, 16), False, "cross", True),
    (12, 4, 3, 7, (1, 14, 7), True, "cross", True),
    (16, 2, 5, 4, (1, 8, 8), True, "mixed", False),
    (8, 2, 4, 16, (1, 16, 16), True, "self", True),
]

# whole model in train(): (config, (B, H, W))
MODEL_CASES = [("tiny", (2, 16, 16)), ("win8_4stage", (1, 128, 128))]
