"""What the per-layer GPU parity files (tests/test_gpu_patch_fast.py, tests/test_gpu_block_fast.py) share: tensors carved from guarded
allocations, the split-bf16 plane decoding and the directory of the parity records."""
import os
import re

import torch

DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
BF16_NAN = 0x7FC0


def record_dir():
    """The directory tests/test_gpu_parity.py keeps its parity.json in: that module is the one place that names it."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "test_gpu_parity.py")) as f:
        m = re.search(r'out_dir = os\.path\.join\(.*, "(\w+)"\)', f.read())
    return os.path.join(os.path.dirname(here), m.group(1))


class Guarded:
    """A tensor carved out of a larger allocation whose bytes either side hold a fixed pattern."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(torch.Size(shape).numel()) * torch.empty((), dtype=dtype).element_size()
        self.whole = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.t = self.whole[GUARD:GUARD + n].view(dtype).view(shape)
        self.n = n

    def intact(self):
        return bool((self.whole[:GUARD] == PATTERN).all()) and bool((self.whole[GUARD + self.n:] == PATTERN).all())


def planes_to_float(hi, lo):
    f = lambda p: ((p.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)
    return f(hi) + f(lo)
