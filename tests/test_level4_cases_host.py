"""CPU-only: every case of tests/level4_cases.py is well conditioned, by the bound tests/test_block_cases_host.py sets for its table (the
float32 oracle agrees with the float64 oracle to a quarter of the exact tier's bar on every output element), so the GPU test needs no
exclusion; a case that is not gets another seed in level4_cases.SEED_OVERRIDE."""
import pytest
import torch

from tests import block_cases as BC
from tests import golden_util as G
from tests import level4_cases as L4

TOL_FP32 = 2e-5   # tests/test_gpu_parity.py


@pytest.mark.parametrize("case", L4.ALL, ids=lambda c: c.id)
def test_case_is_well_conditioned(case):
    for a, b in zip(BC.reference(case, torch.float32), BC.reference64(case)):
        assert a.shape == b.shape == (case.B, case.C, case.H, case.W)
        l2, mx = G.rel_err(a, b)
        print(f"[level4-cases] {case.id} seed {case.seed}: fp32 vs fp64 rel-L2 {l2:.3e} max-rel {mx:.3e}")
        assert l2 <= TOL_FP32 / 4 and mx <= TOL_FP32 / 4, (case.id, case.seed, l2, mx)


def test_the_table_covers_what_it_names():
    got = {(c.hidden, c.cross, c.shift, c.win, c.B, c.H, c.W) for c in L4.BLOCKS}
    assert len(got) == len(L4.BLOCKS) == 2 * 2 * 2 * 8
    assert {(c.win, c.H * c.W % 64 == 0) for c in L4.BLOCKS} == {(8, True), (7, False)}
    assert all(c.C == 384 and c.heads * c.head_dim == 384 and c.dual for c in L4.ALL) and L4.STAGE.kind == "stage"
