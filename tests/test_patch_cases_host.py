"""CPU-only: every case of tests/patch_cases.py is well conditioned, so that the GPU parity test (tests/test_gpu_patch_fast.py) needs
no exclusion.  The float32 oracle must agree with the float64 oracle to a quarter of the exact tier's bar, in rel-L2 and in
max|err| / max|ref|, on every output element; a case that does not gets another seed in patch_cases.SEED_OVERRIDE."""
import pytest
import torch

from tests import golden_util as G
from tests import patch_cases as PC

TOL_FP32 = 2e-5   # tests/test_gpu_parity.py


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.id)
def test_case_is_well_conditioned(case):
    ref64 = PC.reference64(case)
    ref32 = PC.reference(case, torch.float32)
    for a, b in zip(ref32, ref64):
        assert a.shape == b.shape == (case.B, case.cout, *case.out_hw())
        l2, mx = G.rel_err(a, b)
        assert l2 <= TOL_FP32 / 4 and mx <= TOL_FP32 / 4, (case.id, case.seed, l2, mx)


@pytest.mark.parametrize("case", PC.plane_cases(), ids=lambda c: c.id)
def test_ln1_planes_of_a_case_are_well_conditioned(case):
    for a, b in zip(PC.ln1_reference(case, torch.float32), PC.ln1_reference(case, torch.float64)):
        l2, mx = G.rel_err(a, b)
        assert l2 <= TOL_FP32 / 4 and mx <= TOL_FP32 / 4, (case.id, case.seed, l2, mx)


def test_case_table_is_the_cross_product():
    assert len(PC.MERGE_CASES) == len(PC.MERGE_WIDTHS) * len(PC.MERGE_MAPS) == 36
    assert len(PC.UNMERGE_CASES) == len(PC.UNMERGE_WIDTHS) * len(PC.UNMERGE_MAPS) == 40
    assert len({c.id for c in PC.CASES}) == len(PC.CASES) and len({c.seed for c in PC.CASES}) == len(PC.CASES)
