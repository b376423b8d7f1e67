"""Q_CB, Q_CV, CE, EI and RMSE of include/swinfuse.h (swf_fusion_perception) restated in numpy float64: the quantiser of
tests/metrics_restatement.py, the contrast-sensitivity filtering through np.fft (spec), and a second route for the same filtering
through explicit twiddle matrices exp(-+2 pi i ((j k) mod n) / n), which is how the kernels transform.  This is the oracle of
tests/test_perception_host.py (identities, conventions, the conditions of the gate) and tests/test_gpu_perception.py (the kernels).
Restated from the published definitions (Chen & Blum 2009, Chen & Varshney 2007) and the open MATLAB evaluators; parity with any of
them is unpinned.

A = ir, B = vis, F = fusion, all as 8-bit levels.
  stretch(X)   rint((255 (X - min X)) / (max X - min X)); a flat image becomes all zeros
  s(j, n)      j if j < ceil(n / 2) else j - n: freqspace with fftshift, written without the shift
  spec(X, G)   Re(IDFT2(DFT2(X) o G)), G evaluated at bin (u, v) from rho = sqrt(s(u, H)^2 + s(v, W)^2)
"""
import numpy as np

from tests.fidelity_restatement import sobel_replicated
from tests.metrics_restatement import quantise, sobel

NAMES = ("Qcb", "Qcv", "CE", "EI", "RMSE")
DEFAULTS = {"f0": 15.3870, "f1": 1.3456, "a": 0.7622, "p": 3.0, "q": 2.0, "Z": 1e-4, "alpha": 1.0}
TAPS, SIGMAS = 31, (2.0, 4.0)
BLOCK = 16
NEAR = 1e-6        # a pixel with 0 < |b2| < NEAR max|b2| counts as near zero: b1 / b2 is ill-conditioned there


def stretch(X):
    """The integer image X to 0..255 over its own range, float64; a flat image becomes all zeros."""
    X = np.asarray(X, dtype=np.int64)
    lo, hi = int(X.min()), int(X.max())
    if hi == lo:
        return np.zeros(X.shape, dtype=np.float64)
    return np.rint((255.0 * (X - lo).astype(np.float64)) / float(hi - lo))


def signed_frequency(n):
    j = np.arange(n, dtype=np.int64)
    return np.where(j < (n + 1) // 2, j, j - n)


def rho(H, W):
    su, sv = signed_frequency(H), signed_frequency(W)
    return np.sqrt((su[:, None] ** 2 + sv[None, :] ** 2).astype(np.float64))


def csf_dog(H, W, f0, f1, a):
    """Q_CB's filter: the difference of Gaussians of Chen & Blum on r = rho / 15."""
    r = rho(H, W) / 15.0
    return np.exp(-(r / f0) ** 2) - a * np.exp(-(r / f1) ** 2)


def csf_mannos(H, W):
    """Q_CV's filter: Mannos-Sakrison on r = rho / 4."""
    r = rho(H, W) / 4.0
    return 2.6 * (0.0192 + 0.144 * r) * np.exp(-((0.144 * r) ** 1.1))


def twiddles(n, sign):
    """exp(sign 2 pi i ((j k) mod n) / n): the argument reduced in integers before the sine and cosine."""
    j = np.arange(n, dtype=np.int64)
    m = (j[:, None] * j[None, :]) % n
    ang = 2.0 * np.pi * m.astype(np.float64) / float(n)
    return np.cos(ang) + sign * 1j * np.sin(ang)


def spec(X, G, route="fft"):
    """Re(IDFT2(DFT2(X) o G)); route "fft": np.fft, route "matrix": dense products with twiddle matrices."""
    H, W = X.shape
    if route == "fft":
        return np.real(np.fft.ifft2(np.fft.fft2(X) * G))
    assert route == "matrix", route
    Z = (twiddles(H, -1.0) @ X.astype(np.complex128) @ twiddles(W, -1.0)) * G
    return np.real(twiddles(H, 1.0) @ Z @ twiddles(W, 1.0)) / float(H * W)


def gauss_taps(sigma):
    """The 1-D factor of exp(-(x^2 + y^2) / (2 sigma^2)) / (2 pi sigma^2) over x = -15..15 (not normalised to sum 1)."""
    x = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) // 2
    return np.exp(-(x * x) / (2.0 * sigma * sigma)) / np.sqrt(2.0 * np.pi * sigma * sigma)


def filter_same(X, g):
    """'same' filtering of X with outer(g, g) under zero padding: rows first, then columns, taps in ascending order."""
    n = len(g)
    H, W = X.shape
    P = np.zeros((H + n - 1, W + n - 1), dtype=np.float64)
    P[n // 2:n // 2 + H, n // 2:n // 2 + W] = X
    rows = np.zeros((H + n - 1, W), dtype=np.float64)
    for k in range(n):
        rows += g[k] * P[:, k:k + W]
    out = np.zeros((H, W), dtype=np.float64)
    for k in range(n):
        out += g[k] * rows[k:k + H, :]
    return out


def local_contrast(X, G, p, q, Z, route="fft"):
    """-> (C' of the level image X, its b2 plane)."""
    Xf = spec(stretch(X), G, route)
    b1, b2 = filter_same(Xf, gauss_taps(SIGMAS[0])), filter_same(Xf, gauss_taps(SIGMAS[1]))
    zero = b2 == 0.0
    C = np.where(zero, 0.0, np.abs(b1 / np.where(zero, 1.0, b2) - 1.0))
    return C ** p / (C ** q + Z), b2


def qcb(F, A, B, f0, f1, a, p, q, Z, route="fft"):
    """-> (Q_CB, near-zero b2 pixels, {"both_zero": pixels where a Q_XF took the both-zero rule, "lam_half": pixels with lambda = 1/2})."""
    G = csf_dog(F.shape[0], F.shape[1], f0, f1, a)
    (cA, bA), (cB, bB), (cF, bF) = (local_contrast(X, G, p, q, Z, route) for X in (A, B, F))
    near = 0
    for b2 in (bA, bB, bF):
        m = np.abs(b2)
        near += int(np.count_nonzero((m > 0.0) & (m < NEAR * m.max())))

    def ratio(cX):
        both = (cX == 0.0) & (cF == 0.0)
        hi = np.maximum(cX, cF)
        return np.where(both, 1.0, np.minimum(cX, cF) / np.where(both, 1.0, hi)), both

    qA, bothA = ratio(cA)
    qB, bothB = ratio(cB)
    den = cA * cA + cB * cB
    half = den == 0.0
    lam = np.where(half, 0.5, (cA * cA) / np.where(half, 1.0, den))
    value = lam * qA + (1.0 - lam) * qB
    return float(value.sum() / value.size), near, {"both_zero": int(bothA.sum() + bothB.sum()), "lam_half": int(half.sum())}


def block_sums(X):
    """Sums over the 16x16 blocks tiling from the top-left; partial blocks are kept (the missing pixels add nothing)."""
    H, W = X.shape
    bh, bw = -(-H // BLOCK), -(-W // BLOCK)
    P = np.zeros((bh * BLOCK, bw * BLOCK), dtype=np.float64)
    P[:H, :W] = X
    return P.reshape(bh, BLOCK, bw, BLOCK).sum(axis=(1, 3))


def qcv(F, A, B, alpha, route="fft"):
    """-> (Q_CV, {"den_zero": bool, "partial_blocks": count}).  lambda_X(block) = sum of G_X^alpha over the block's pixels inside the
    image; D_X(block) = (sum of spec(X - F, theta)^2 over those pixels) / 256."""
    H, W = F.shape
    sA, sB, sF = stretch(A), stretch(B), stretch(F)
    theta = csf_mannos(H, W)
    num, den = 0.0, 0.0
    lam, D = [], []
    for sX in (sA, sB):
        gx, gy = sobel(sX.astype(np.int64))
        g = np.sqrt((gx * gx + gy * gy).astype(np.float64))
        lam.append(block_sums(g ** alpha))
        Y = spec(sX - sF, theta, route)
        D.append(block_sums(Y * Y) / float(BLOCK * BLOCK))
    num = float((lam[0] * D[0] + lam[1] * D[1]).sum())
    den = float((lam[0] + lam[1]).sum())
    info = {"den_zero": den == 0.0, "partial_blocks": int(lam[0].size - (H // BLOCK) * (W // BLOCK))}
    return (0.0 if den == 0.0 else num / den), info


def cross_entropy(X, Fl):
    """-> (ce(X, F), bins skipped because exactly one of the two is empty)."""
    pX = np.bincount(X.ravel(), minlength=256).astype(np.float64) / X.size
    pF = np.bincount(Fl.ravel(), minlength=256).astype(np.float64) / Fl.size
    m = (pX > 0) & (pF > 0)
    return float(np.sum(pX[m] * np.log2(pX[m] / pF[m]))), int(np.count_nonzero((pX > 0) != (pF > 0)))


def edge_intensity(Fl):
    gv, gh = sobel_replicated(Fl)
    return float(np.sqrt((gv * gv + gh * gh).astype(np.float64)).sum() / Fl.size)


def rmse(X, Fl):
    d = X.astype(np.int64) - Fl.astype(np.int64)
    return float(np.sqrt(float((d * d).sum()) / d.size) / 255.0)


def image_perception(fusion, ir, vis, route="fft", with_near=False, with_info=False, **constants_):
    """The five values of one image: fusion, ir, vis are (H, W) float32 arrays.  with_near: also the count of near-zero b2 pixels.
    with_info: also a dict of which conventions the image took."""
    unknown = set(constants_) - set(DEFAULTS)
    assert not unknown, unknown
    c = {**DEFAULTS, **constants_}
    F, A, B = quantise(fusion), quantise(ir), quantise(vis)
    row = np.zeros(len(NAMES), dtype=np.float64)
    row[0], near, info = qcb(F, A, B, c["f0"], c["f1"], c["a"], c["p"], c["q"], c["Z"], route)
    row[1], info_cv = qcv(F, A, B, c["alpha"], route)
    ceA, skipA = cross_entropy(A, F)
    ceB, skipB = cross_entropy(B, F)
    row[2] = (ceA + ceB) / 2.0
    row[3] = edge_intensity(F)
    row[4] = (rmse(A, F) + rmse(B, F)) / 2.0
    info.update(info_cv, ce_skipped=skipA + skipB, flat=sum(int(X.min() == X.max()) for X in (F, A, B)))
    out = (row,)
    if with_near:
        out += (near,)
    if with_info:
        out += (info,)
    return out if len(out) > 1 else row


def batch_perception(fusion, ir, vis, route="fft", with_near=False, with_info=False, **constants_):
    """(B, 1, H, W) float32 arrays or CPU tensors -> (B, 5) float64 (with_near: and the per-image near-zero counts; with_info: and the
    per-image convention reports)."""
    f, i, v = (np.asarray(t, dtype=np.float32) for t in (fusion, ir, vis))
    res = [image_perception(f[b, 0], i[b, 0], v[b, 0], route=route, with_near=with_near, with_info=with_info, **constants_)
           for b in range(f.shape[0])]
    if not (with_near or with_info):
        return np.stack(res)
    return (np.stack([r[0] for r in res]),) + tuple([r[k] for r in res] for k in range(1, len(res[0])))
