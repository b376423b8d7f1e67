"""Case table of tests/test_gpu_level4_throughput.py: level-4 blocks (C = 384 = 8 heads of 48) with both hidden widths, self and cross,
plain and shifted, one and three images, on maps of one and two windows per image with 8x8 and 7x7 windows, and one stage.  The case
type, weights, inputs and the reference are those of tests/block_cases.py; tests/test_level4_cases_host.py holds every case to the
conditioning bound of that table."""
from tests import block_cases as BC

C, HEADS, HEAD_DIM = 384, 8, 48
HIDDEN = (1536, 768)
MAPS = {8: [(1, 8, 8), (3, 8, 8), (1, 16, 8), (3, 16, 8)], 7: [(1, 7, 7), (3, 7, 7), (1, 14, 7), (3, 14, 7)]}
SEED0 = 5100
SEED_OVERRIDE: dict = {}   # by case id, as in tests/block_cases.py


def _cases():
    out = []
    for win, maps in MAPS.items():
        for m in maps:
            for hid in HIDDEN:
                for cross in (False, True):
                    for shift in (False, True):
                        out.append(BC.Case("block", C, HEADS, HEAD_DIM, hid, win, *m, shift=shift, cross=cross, seed=SEED0 + len(out)))
    out.append(BC.Case("stage", C, HEADS, HEAD_DIM, 1536, 8, 3, 16, 8, seed=SEED0 + len(out)))
    return [BC.replace(c, seed=SEED_OVERRIDE.get(c.id, c.seed)) for c in out]


ALL = _cases()
BLOCKS, STAGE = ALL[:-1], ALL[-1]
