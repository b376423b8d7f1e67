"""The inputs of the comparative-study tests (tests/test_comparative_host.py on the CPU, tests/test_gpu_comparative.py on the kernels)
and their restatement values, computed once per case and shared.

Shapes: 1x1 is one bin of the transform, no difference and no Haar block; 5x7 and 17x23 are odd in both axes (no Nyquist bin, an odd
pixel count for the median, a dropped trailing row and column at both Haar scales), 5x7 with one second-scale block row only; 16x16
and 32x32 are whole Haar blocks with a Nyquist bin in both axes and an even pixel count; 40x36 and 100x75 have partial level tiles in
one or both axes and more than one tile of the transform, 100x75 more than one tile of the moment passes too; 64x48 is a whole number
of transform tiles; 224x224 (noise only) is the size validation runs at, with several histogram tiles.

Kinds: those of tests/perception_cases.py.  "same": fusion = ir = vis (Qmi = 2, Qsf = 0, Qm = 1, Qp = 1).  "flat3": three flat images
(Qmi = Qte = 0, Qncie = 1 - log_256 3, Qsf = 0, Qm = 0, Qp = 1).  "flat_source": vis flat, fusion = ir."""
import functools

from tests import comparative_restatement as R
from tests.perception_cases import make_inputs, shape_id  # noqa: F401

SHAPES = [(1, 1, 1, 1), (1, 1, 5, 7), (1, 1, 16, 16), (1, 1, 17, 23), (1, 1, 32, 32), (1, 1, 40, 36), (1, 1, 64, 48), (1, 1, 100, 75)]
KINDS = ["noise", "smooth", "flat_source", "same", "flat3"]
CASES = [(s, k) for s in SHAPES for k in KINDS] + [((1, 1, 224, 224), "noise")]

# (constant, another value, the one value it moves), in the order of the descriptor
CONSTANT_MOVES = [("q", 1.5, "Qte"), ("alpha1", 2.0, "Qm"), ("alpha2", 0.5, "Qm"), ("min_wavelength", 4.0, "Qp"), ("mult", 1.8, "Qp"),
                  ("sigma_onf", 0.65, "Qp"), ("k", 3.0, "Qp"), ("cutoff", 0.4, "Qp"), ("g", 8.0, "Qp"), ("eps", 1e-3, "Qp"), ("C", 1e-2, "Qp"),
                  ("ep", 2.0, "Qp"), ("eM", 2.0, "Qp"), ("em", 2.0, "Qp")]


def case_id(case):
    return f"{shape_id(case[0])}-{case[1]}"


@functools.lru_cache(maxsize=None)
def reference(shape, kind, seed=0):
    """-> (B, 6) restatement values, read-only."""
    ref = R.batch_comparative(*make_inputs(shape, kind, seed))
    ref.setflags(write=False)
    return ref
