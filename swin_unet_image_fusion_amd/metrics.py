"""Fusion-quality metrics on libswinfuse: EN, MI, SD, SF, AG, CC, SCD, MSE, PSNR and Qabf of a batch of fused images against their
infrared and visible sources in one fused HIP call (swf_fusion_metrics; include/swinfuse.h has every definition).

Every metric is a function of 8-bit levels.  The quantiser is torchvision save_image's, in fp32 with its two roundings,
`(int) min(max(x * 255 + 0.5, 0), 255)` (never one fused multiply-add; NaN -> level 0), so stored uint8 images passed as `u8 / 255`
evaluate exactly.  Conventions for degenerate images: EN of a one-level image is +0; an axis of length 1 contributes 0 to SF and makes
AG 0; Pearson's r (CC, SCD) is 0 when either variance is 0; PSNR is +inf at MSE = 0; Qabf is 0 when no source pixel has a gradient
(its Sobel responses see a zero border, so a flat non-black image has edges along its frame).

VIF (multi-scale pixel-domain, per source and summed) and Nabf with its loss term Labf come from a second fused HIP call on the same
levels, fp64 throughout (swf_fusion_fidelity: `fusion_fidelity`, or `FusionMetrics(fidelity=True)` for all fifteen values).  VIF of a
source is 0 when its denominator is (an image under 17 pixels in an axis, a flat source).

The structural-similarity group comes from a third fused HIP call on the same levels (swf_fusion_structure: `fusion_structure`, or
`FusionMetrics(structure=True)`): Wang's SSIM (per source and summed) and MS-SSIM with the 11-tap Gaussian in fp64, Piella's Q_S, Q_W
and Q_E, Cvejic's Q_C and Yang's Q_Y on exact integer window sums.  SSIM is 0 for an image under 11 pixels in an axis, MS-SSIM under
176, the Piella / Cvejic values under 8 and Yang's under 7.

The human-perception group comes from a fourth fused HIP call on the same levels, fp64 throughout (swf_fusion_perception:
`fusion_perception`, or `FusionMetrics(perception=True)`; with the three switches on, all 29 values, which cover VIFB's thirteen as well).
With A = ir, B = vis, F = fusion; stretch(X) = rint((255 (X - min X)) / (max X - min X)), a flat image becoming all zeros; s(j, n) = j if
j < ceil(n / 2) else j - n; spec(X, G) = Re(IDFT2(DFT2(X) o G)), G evaluated at bin (u, v) from rho = sqrt(s(u, H)^2 + s(v, W)^2):
  Qcb   Chen & Blum.  S = exp(-(r / f0)^2) - a exp(-(r / f1)^2), r = rho / 15.  For each X of A, B, F: X' = spec(stretch(X), S); b1, b2 =
        X' filtered with zero padding and 'same' size by the 31x31 kernels exp(-(x^2 + y^2) / (2 sd^2)) / (2 pi sd^2), x, y = -15 .. 15,
        sd = 2 and 4; C = |b1 / b2 - 1|, 0 where b2 = 0; C' = C^p / (C^q + Z).  Q_XF = min(C'_X, C'_F) / max(C'_X, C'_F), 1 where both
        are 0; lambda_A = C'_A^2 / (C'_A^2 + C'_B^2), 1/2 where the denominator is 0; Qcb = mean(lambda_A Q_AF + (1 - lambda_A) Q_BF).
  Qcv   Chen & Varshney, LOWER IS BETTER.  On stretch(A), stretch(B), stretch(F): G_X = the Sobel magnitude sqrt(gx^2 + gy^2) of the
        stretched A and B under a zero border; 16x16 blocks tiling from the top-left, partial blocks kept and zero-padded;
        lambda_X(block) = sum of G_X^alpha over the block's pixels inside the image; theta = 2.6 (0.0192 + 0.144 r) exp(-(0.144 r)^1.1),
        r = rho / 4 (Mannos-Sakrison); D_X(block) = sum of spec(X - F, theta)^2 over the block / 256;
        Qcv = sum(lambda_A D_A + lambda_B D_B) / sum(lambda_A + lambda_B), 0 where that sum is 0.
  CE    (ce(A, F) + ce(B, F)) / 2, ce(X, F) = sum_k p_X(k) log2(p_X(k) / p_F(k)) over the bins of the 256-bin histograms where both
        are non-zero.
  EI    the mean over pixels of the Sobel magnitude of F's levels with replicated borders.
  RMSE  (sqrt(mean((A - F)^2)) + sqrt(mean((B - F)^2))) / 2 on levels / 255.
So F = A = B gives Qcb = 1, Qcv = 0, CE = 0, RMSE = 0; three flat images 1, 0, 0, 0; a flat vis with F = ir gives Qcb = 1.  The filtering
is dense (fp64 DFT products on the matrix cores against twiddle matrices the call builds), for any H and W up to 16384.

The comparative-study group comes from a fifth fused HIP call on the same levels, fp64 throughout (swf_fusion_comparative:
`fusion_comparative`, or `FusionMetrics(comparative=True)`; with the four switches on, all 35 values): the six of Liu et al.'s twelve
(TPAMI 2012) that the other calls lack (they have Q_G = Qabf, Q_S, Q_C, Q_Y, Q_CV, Q_CB).  Restated from memory of the papers: PARITY
WITH ANY OF THEM IS UNPINNED, and where a paper differs, this text holds.  p_X, p_XY = the 256-bin and 256 x 256-bin relative
frequencies, H = entropy with log2, H_b = H / 8 (base 256), sums over non-zero bins, MI(X, Y) = sum p_XY log2(p_XY / (p_X p_Y)):
  Qmi   2 [MI(A, F) / (H(A) + H(F)) + MI(B, F) / (H(B) + H(F))]; a term whose denominator is 0 contributes 0.
  Qte   I(X, Y) = (1 - sum p_XY^q / (p_X p_Y)^(q - 1)) / (1 - q), Hq(X) = (1 - sum p_X^q) / (q - 1);
        Qte = (I(A, F) + I(B, F)) / (Hq(A) + Hq(B) - I(A, B)), 0 where that denominator is 0.
  Qncie NCC(X, Y) = H_b(X) + H_b(Y) - H_b(X, Y); R = the symmetric 3 x 3 matrix with unit diagonal and the NCCs in the order (A, B, F);
        lambda_i its eigenvalues (cyclic Jacobi sweeps); Qncie = 1 + sum (lambda_i / 3) log_256(lambda_i / 3), terms with lambda_i <= 0 being 0.
  Qsf   D_h, D_v, D_md, D_sd = I(i, j) minus I(i, j-1), I(i-1, j), I(i-1, j-1), I(i-1, j+1) where both pixels exist;
        SF = sqrt((sum D_h^2 + sum D_v^2 + w_d sum D_md^2 + w_d sum D_sd^2) / (H W)), w_d = 1 / sqrt 2; SF_F from F, SF_R from
        max(|D(A)|, |D(B)|) per pixel and direction; Qsf = (SF_F - SF_R) / SF_R, 0 where SF_R = 0.  An axis of one pixel leaves only the
        differences along the other.
  Qm    on levels / 255, two scales of the decimated orthonormal Haar transform (per 2 x 2 block [a b; c d]: LL = (a + b + c + d) / 2,
        LH = (a + b - c - d) / 2, HL = (a - b + c - d) / 2, HH = (a - b - c + d) / 2; an odd trailing row or column dropped).  Per scale,
        for X of A, B: EP_X = (exp(-|LH_X - LH_F|) + exp(-|HL_X - HL_F|) + exp(-|HH_X - HH_F|)) / 3, w_X = LH_X^2 + HL_X^2 + HH_X^2,
        Q_s = sum(EP_A w_A + EP_B w_B) / sum(w_A + w_B), 1 for a scale without coefficients (an axis under 2 pixels; under 4 for the
        second), 0 when the weights sum to 0; Qm = Q_1^alpha1 Q_2^alpha2.
  Qp    Zhao's, on Kovesi-style phase congruency of the levels with 4 scales and 6 orientations: log-Gabor filters
        G_s = exp(-ln(rho / f_s)^2 / (2 ln(sigma_onf)^2)) / (1 + (rho / 0.45)^30), f_s = 1 / (min_wavelength mult^(s-1)), angular spread
        (cos(min(3 dtheta, pi)) + 1) / 2 about a = (o - 1) pi / 6; per orientation the energy sum_s (E mE + O mO - |E mO - O mE|) less
        T = tt sqrt(pi / 2) + k tt sqrt((4 - pi) / 2), tt = tau (1 - mult^-4) / (1 - 1 / mult), tau = median(An at s = 1) / sqrt(ln 4),
        weighted by 1 / (1 + exp((cutoff - width) g)), width = (sumAn / (maxAn + eps) - 1) / 3, over sumAn + eps; the maps p = sum_o PC_o
        and the maximum and minimum moments M, m; for each map kind S = max(X_A, X_B), c(U, V) = (cov + C) / (sd_U sd_V + C) over the
        whole image, P = max(c(X_A, X_F), c(X_B, X_F), c(S, X_F), 0); Qp = P_p^ep P_M^eM P_m^em.  include/swinfuse.h has every step.
So F = A = B gives Qmi = 2 (not flat), Qsf = 0, Qm = 1 (not flat), Qp = 1; three flat images give Qmi = 0, Qte = 0, Qncie = 1 - log_256 3,
Qsf = 0, Qm = 0 (1 under 2 pixels in an axis: no coefficients), Qp = 1.

Feature mutual information comes from a sixth fused HIP call on the same levels, fp64 throughout (swf_fusion_feature: `fusion_feature`,
or `FusionMetrics(feature=True)`; with the five switches on, all 39 values): FMI_pixel, FMI_dct, FMI_w and FMI_edge.  Restated from
memory of Haghighat & Razian's method and of the common open evaluators: PARITY WITH ANY OF THEM IS UNPINNED, and where they differ,
this text holds.  The feature plane T(X) of X = A, B, F is
  pixel  the levels, H x W.
  edge   |sx| + |sy| of the 3x3 Sobel pair on the levels with replicated borders, H x W (exact integers).
  w      one level of the decimated orthonormal Haar transform (Qm's formulas, an odd trailing row or column dropped), the sub-bands as
         the mosaic [LL LH; HL HH], 2 floor(H / 2) x 2 floor(W / 2) (multiples of 1/2: exact).
  dct    the orthonormal 2-D DCT-II D_H L D_W^T, D_n[k][i] = s_k sqrt(2 / n) cos(pi (2 i + 1) k / (2 n)), s_0 = 1 / sqrt 2, else 1, the
         argument reduced in integers (m = ((2 i + 1) k) mod 4 n, cospi(m / (2 n))), every coefficient snapped to
         rint(T / dct_step) dct_step, ties to even; without the snap the windows of a flat or symmetric image would normalise rounding
         noise up to full range.
FMI of a feature is the mean, over every window x window patch that lies wholly inside the plane (0 when there is none), of
(I(A, F) + I(B, F)) / 2.  The l = window^2 samples of a patch are read column-major (MATLAB's (:)).  I(X, F) = 1 if x_k = f_k for every
k.  Otherwise x'_k = 1 when max x = min x, else (x_k - min x) / (max x - min x); p_k = x'_k / sum x', q_k from f likewise, P and Q their
running sums; c = sum (p_k - 1/l)(q_k - 1/l) / sqrt(sum (p_k - 1/l)^2 sum (q_k - 1/l)^2), 0 when the denominator is 0; with k counted
from 1, mu_p = sum k p_k, sigma_p = sqrt(max(sum k^2 p_k - mu_p^2, 0)); G_ij = min(P_i, Q_j) if c >= 0, max(P_i + Q_j - 1, 0) if c < 0
(the Frechet bounds); rho = sum_ij (G_ij - P_i Q_j) / (sigma_p sigma_q), 0 when sigma_p sigma_q = 0; phi = clamp(c / rho, 0, 1), 0 when
rho = 0; the joint cdf J_ij = phi G_ij + (1 - phi) P_i Q_j; the joint pdf j_ij = (J_ij - J_(i-1)j) - (J_i(j-1) - J_(i-1)(j-1)), J = 0 at
index -1; with H(t) = -sum_{t > 0} t log2 t, I(X, F) = 2 (H(p) + H(q) - H(j)) / (H(p) + H(q)), 0 when H(p) + H(q) = 0.
So F = A = B gives 1 for every feature that has a window; a 3x3 image has one pixel window and no 'w' window (its Haar plane is 2x2); an
axis shorter than the window gives 0.

The definitions are restated from the published ones and the common open evaluators; no MATLAB, VIFB or sewar copy is available to
this build, so parity with any of them is unpinned.  `MyLoss(choose_ms_ssim=False).calcu_ssim_loss` is a different
thing: the training loss's kornia-style SSIM on unit-range floats, returned as a loss; SSIM as a metric on levels is `fusion_structure`'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .modules import _ptr, _stream, _workspace

__all__ = ["METRIC_NAMES", "QABF_DEFAULTS", "FIDELITY_NAMES", "FIDELITY_DEFAULTS", "STRUCTURE_NAMES", "STRUCTURE_DEFAULTS", "PERCEPTION_NAMES",
           "PERCEPTION_DEFAULTS", "COMPARATIVE_NAMES", "COMPARATIVE_DEFAULTS", "FEATURE_NAMES", "FEATURE_DEFAULTS", "fusion_metrics",
           "fusion_fidelity", "fusion_structure", "fusion_perception", "fusion_comparative", "fusion_feature", "FusionMetrics"]

METRIC_NAMES = ("EN", "MI", "SD", "SF", "AG", "CC", "SCD", "MSE", "PSNR", "Qabf")   # the order of the header's SWF_METRIC_* enum
QABF_DEFAULTS = {"Tg": 0.9994, "kg": -15.0, "Dg": 0.5, "Ta": 0.9879, "ka": -22.0, "Da": 0.8}   # Xydeas & Petrovic
FIDELITY_NAMES = ("VIF", "VIF_IR", "VIF_VIS", "Nabf", "Labf")                        # the order of the header's SWF_FIDELITY_* enum
FIDELITY_DEFAULTS = {"sigma_nsq": 2.0, "eps": 1e-10,                                # Sheikh & Bovik (vifp_mscale)
                     "Td": 2.0, "wt_min": 0.001, "Nrg": 0.9999, "kg": 19.0, "sg": 0.5, "Nra": 0.9995, "ka": 22.0, "sa": 0.5}   # Kumar
STRUCTURE_NAMES = ("SSIM", "SSIM_IR", "SSIM_VIS", "MS_SSIM", "Qs", "Qw", "Qe", "Qc", "Qy")   # the order of the header's SWF_STRUCTURE_* enum
STRUCTURE_DEFAULTS = {"K1": 0.01, "K2": 0.03, "alpha": 1.0, "Ty": 0.75}   # Wang's SSIM constants, Piella's edge exponent, Yang's threshold
PERCEPTION_NAMES = ("Qcb", "Qcv", "CE", "EI", "RMSE")                                # the order of the header's SWF_PERCEPTION_* enum
PERCEPTION_DEFAULTS = {"f0": 15.3870, "f1": 1.3456, "a": 0.7622, "p": 3.0, "q": 2.0, "Z": 1e-4,   # Chen & Blum's filter and contrast map
                       "alpha": 1.0}                                                              # Chen & Varshney's saliency exponent
COMPARATIVE_NAMES = ("Qmi", "Qte", "Qncie", "Qm", "Qsf", "Qp")                       # the order of the header's SWF_COMPARATIVE_* enum
COMPARATIVE_DEFAULTS = {"q": 1.85, "alpha1": 1.0, "alpha2": 1.0,                                  # Tsallis order, Q_M's scale exponents
                        "min_wavelength": 3.0, "mult": 2.1, "sigma_onf": 0.55, "k": 2.0, "cutoff": 0.5, "g": 10.0, "eps": 1e-4,   # Kovesi
                        "C": 1e-4, "ep": 1.0, "eM": 1.0, "em": 1.0}                                # Zhao's stabiliser and exponents
FEATURE_NAMES = ("FMI_pixel", "FMI_dct", "FMI_w", "FMI_edge")                        # the order of the header's SWF_FEATURE_* enum
FEATURE_DEFAULTS = {"window": 3.0, "dct_step": 2.0 ** -16}                           # the window's side (3 or 5), the DCT coefficients' snap


def _check_images(fusion: Tensor, ir: Tensor, vis: Tensor) -> None:
    for name, t in (("fusion_images", fusion), ("ir_images", ir), ("vis_images", vis)):
        if t.dim() != 4:
            raise ValueError(f"{name}: expected a 4-D (batch, 1, height, width) tensor, got shape {tuple(t.shape)}")
        if t.shape[1] != 1:
            raise NotImplementedError(f"{name}: the metric kernels take single-channel images, got {t.shape[1]} channels")
        if t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: the metric kernels are fp32 only, got {t.dtype}")
        if not t.is_cuda:
            raise NotImplementedError(f"{name}: the metrics run on the GPU only (there is no CPU path), got a tensor on {t.device}")
    if not (fusion.shape == ir.shape == vis.shape):
        raise ValueError(f"shapes differ: fusion {tuple(fusion.shape)}, ir {tuple(ir.shape)}, vis {tuple(vis.shape)}")
    if torch.is_grad_enabled() and (fusion.requires_grad or ir.requires_grad or vis.requires_grad):
        raise RuntimeError("the metrics are not differentiable (functions of 8-bit levels): call them under torch.no_grad() or on "
                           "detached tensors")


class _Family(NamedTuple):
    names: Tuple[str, ...]
    defaults: dict
    desc: type      # the ctypes descriptor; its fields are the defaults, in their order
    count: int
    call: str       # the library entry; its size query is `call + "_workspace_bytes"`
    constant: str   # what the unknown-constant message calls a constant


_FAMILIES = {
    "metrics": _Family(METRIC_NAMES, QABF_DEFAULTS, L.MetricsDesc, L.METRIC_COUNT, "swf_fusion_metrics", "Qabf constant(s)"),
    "fidelity": _Family(FIDELITY_NAMES, FIDELITY_DEFAULTS, L.FidelityDesc, L.FIDELITY_COUNT, "swf_fusion_fidelity", "constant(s)"),
    "structure": _Family(STRUCTURE_NAMES, STRUCTURE_DEFAULTS, L.StructureDesc, L.STRUCTURE_COUNT, "swf_fusion_structure", "constant(s)"),
    "perception": _Family(PERCEPTION_NAMES, PERCEPTION_DEFAULTS, L.PerceptionDesc, L.PERCEPTION_COUNT, "swf_fusion_perception", "constant(s)"),
    "comparative": _Family(COMPARATIVE_NAMES, COMPARATIVE_DEFAULTS, L.ComparativeDesc, L.COMPARATIVE_COUNT, "swf_fusion_comparative",
                           "constant(s)"),
    "feature": _Family(FEATURE_NAMES, FEATURE_DEFAULTS, L.FeatureDesc, L.FEATURE_COUNT, "swf_fusion_feature", "constant(s)"),
}


def _desc(kind: str, constants: dict):
    fam = _FAMILIES[kind]
    unknown = set(constants) - set(fam.defaults)
    if unknown:
        raise TypeError(f"fusion_{kind}: unknown {fam.constant} {sorted(unknown)}; the constants are {list(fam.defaults)}")
    c = {**fam.defaults, **constants}
    return fam.desc(*(float(c[k]) for k in fam.defaults))


def _call(kind: str, fusion: Tensor, ir: Tensor, vis: Tensor, constants: dict) -> Tensor:
    fam = _FAMILIES[kind]
    desc = _desc(kind, constants)
    _check_images(fusion, ir, vis)
    f, i, v = fusion.detach().contiguous(), ir.detach().contiguous(), vis.detach().contiguous()
    b, _, h, w = f.shape
    lib = L.lib()
    need = getattr(lib, fam.call + "_workspace_bytes")(b, h, w)   # 0 for a shape the call refuses: it then raises with the library's text
    out = torch.empty((b, fam.count), dtype=torch.float64, device=f.device)
    ws, wsn = _workspace(need, f.device)
    L.check(getattr(lib, fam.call)(C.byref(desc), _ptr(f), _ptr(i), _ptr(v), out.data_ptr(), b, h, w, ws, wsn, _stream(f.device)))
    return out


def fusion_metrics(fusion: Tensor, ir: Tensor, vis: Tensor, **qabf_constants) -> Tensor:
    """-> (B, 10) float64 tensor on the inputs' device, row b = the METRIC_NAMES values of image b.  Inputs: (B, 1, H, W) fp32 CUDA
    tensors of one shape.  Keyword arguments replace Qabf constants (Tg, kg, Dg, Ta, ka, Da).  One library call on the current stream,
    no host synchronisation; bit-identical from call to call."""
    return _call("metrics", fusion, ir, vis, qabf_constants)


def fusion_fidelity(fusion: Tensor, ir: Tensor, vis: Tensor, **constants) -> Tensor:
    """-> (B, 5) float64 tensor on the inputs' device, row b = the FIDELITY_NAMES values of image b: VIF = VIF_IR + VIF_VIS, Nabf and
    Labf.  Inputs as for fusion_metrics.  Keyword arguments replace constants (FIDELITY_DEFAULTS).  One library call on the current
    stream, no host synchronisation; bit-identical from call to call."""
    return _call("fidelity", fusion, ir, vis, constants)


def fusion_structure(fusion: Tensor, ir: Tensor, vis: Tensor, **constants) -> Tensor:
    """-> (B, 9) float64 tensor on the inputs' device, row b = the STRUCTURE_NAMES values of image b: SSIM = SSIM_IR + SSIM_VIS,
    MS_SSIM, Piella's Qs, Qw, Qe, Cvejic's Qc and Yang's Qy.  Inputs as for fusion_metrics.  Keyword arguments replace constants
    (STRUCTURE_DEFAULTS); a non-finite one, K1 <= 0, K2 <= 0 or alpha < 0 raises ValueError.  One library call on the current stream,
    no host synchronisation; bit-identical from call to call."""
    return _call("structure", fusion, ir, vis, constants)


def fusion_perception(fusion: Tensor, ir: Tensor, vis: Tensor, **constants) -> Tensor:
    """-> (B, 5) float64 tensor on the inputs' device, row b = the PERCEPTION_NAMES values of image b: Chen & Blum's Qcb, Chen &
    Varshney's Qcv (lower is better), CE, EI and RMSE.  Inputs as for fusion_metrics, at most 16384 pixels in an axis
    (NotImplementedError beyond: the transforms are dense).  Keyword arguments replace constants (PERCEPTION_DEFAULTS); a non-finite
    one, f0 <= 0, f1 <= 0, Z <= 0, p < 0, q < 0 or alpha < 0 raises ValueError.  One library call on the current stream, no host
    synchronisation; bit-identical from call to call."""
    return _call("perception", fusion, ir, vis, constants)


def fusion_comparative(fusion: Tensor, ir: Tensor, vis: Tensor, **constants) -> Tensor:
    """-> (B, 6) float64 tensor on the inputs' device, row b = the COMPARATIVE_NAMES values of image b: Hossny's Qmi, the Tsallis-entropy
    Qte, Qncie, Wang & Liu's Qm, Zheng's Qsf and Zhao's Qp.  Inputs as for fusion_metrics, at most 16384 pixels in an axis and 2730
    images (NotImplementedError beyond: the transforms are dense).  Keyword arguments replace constants (COMPARATIVE_DEFAULTS); a
    non-finite one, q <= 0, q = 1, mult <= 1, sigma_onf outside (0, 1), min_wavelength < 2, eps <= 0, C <= 0 or a negative exponent
    (alpha1, alpha2, ep, eM, em) raises ValueError.  One library call on the current stream, no host synchronisation; bit-identical
    from call to call."""
    return _call("comparative", fusion, ir, vis, constants)


def fusion_feature(fusion: Tensor, ir: Tensor, vis: Tensor, **constants) -> Tensor:
    """-> (B, 4) float64 tensor on the inputs' device, row b = the FEATURE_NAMES values of image b: feature mutual information on the
    level plane, the snapped DCT, one Haar level and the Sobel edge plane.  Inputs as for fusion_metrics, at most 16384 pixels in an axis
    and 21845 images (NotImplementedError beyond: the DCT matrices are dense).  Keyword arguments replace constants (FEATURE_DEFAULTS);
    a window other than 3 or 5, or a dct_step that is not finite and > 0, raises ValueError.  One library call on the current stream, no
    host synchronisation; bit-identical from call to call."""
    return _call("feature", fusion, ir, vis, constants)


class FusionMetrics:
    """Running mean of the ten metrics over every image passed to update(); with `fidelity=True` the FIDELITY_NAMES values (constants:
    `fidelity_constants`) follow the ten, with `structure=True` the STRUCTURE_NAMES values (constants: `structure_constants`) follow
    those, with `perception=True` the PERCEPTION_NAMES values (constants: `perception_constants`) follow those, with `comparative=True` the
    COMPARATIVE_NAMES values (constants: `comparative_constants`) follow those: 10, 15, 19 or 24 values without the last two groups, five
    more with the perception group, six more with the comparative group (up to 35); with `feature=True` the FEATURE_NAMES values (constants:
    `feature_constants`) follow the comparative group's place, four more (up to 39).  The sum lives on the device and update() does not synchronise; compute() reads it back once.  The
    image count is a host int (`count`): the batch size is known on the host, so counting there needs no synchronisation and no
    device scalar."""

    def __init__(self, fidelity: bool = False, fidelity_constants: Optional[dict] = None, structure: bool = False,
                 structure_constants: Optional[dict] = None, perception: bool = False, perception_constants: Optional[dict] = None,
                 comparative: bool = False, comparative_constants: Optional[dict] = None, feature: bool = False,
                 feature_constants: Optional[dict] = None, **qabf_constants):
        self.qabf_constants = qabf_constants
        self.fidelity = bool(fidelity)
        self.fidelity_constants = dict(fidelity_constants or {})
        self.structure = bool(structure)
        self.structure_constants = dict(structure_constants or {})
        self.perception = bool(perception)
        self.perception_constants = dict(perception_constants or {})
        self.comparative = bool(comparative)
        self.comparative_constants = dict(comparative_constants or {})
        self.feature = bool(feature)
        self.feature_constants = dict(feature_constants or {})
        families = (("metrics", True, self.qabf_constants), ("fidelity", self.fidelity, self.fidelity_constants),
                    ("structure", self.structure, self.structure_constants), ("perception", self.perception, self.perception_constants),
                    ("comparative", self.comparative, self.comparative_constants), ("feature", self.feature, self.feature_constants))
        for kind, _, constants in families:
            _desc(kind, constants)   # refuse a misspelt constant here, not at the first batch, of a family that is off too
        self._families = [(kind, constants) for kind, on, constants in families if on]
        self.names = sum((_FAMILIES[kind].names for kind, _ in self._families), ())
        self.reset()

    def reset(self) -> None:
        self._sum: Optional[Tensor] = None
        self.count = 0

    def update(self, fusion: Tensor, ir: Tensor, vis: Tensor) -> Tensor:
        """Adds the batch's rows; -> the rows, (B, len(names)) float64 on the device."""
        parts = [globals()["fusion_" + kind](fusion, ir, vis, **c) for kind, c in self._families]   # the public functions, as bound now
        rows = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        s = rows.sum(dim=0)
        self._sum = s if self._sum is None else self._sum + s
        self.count += rows.shape[0]
        return rows

    def compute(self) -> Dict[str, float]:
        """{name: mean over the images seen since reset()}, one device-to-host copy."""
        if self.count == 0:
            raise RuntimeError("FusionMetrics.compute(): no image since reset()")
        return dict(zip(self.names, (self._sum / self.count).tolist()))
