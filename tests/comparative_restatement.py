"""The comparative-study group of include/swinfuse.h (Qmi, Qte, Qncie, Qm, Qsf, Qp) restated in numpy float64: what the HIP kernels of
csrc/kernels_comparative.hip are checked against.  The text is the header's, written from memory of the papers; parity with any
published evaluator is unpinned.  Transforms through np.fft, the 3 x 3 eigenvalues through a Jacobi solver of its own, the median
through np.median.

A = ir, B = vis, F = fusion as 8-bit levels (tests/metrics_restatement.quantise)."""
import numpy as np

from tests.metrics_restatement import quantise
from tests.perception_restatement import signed_frequency

NAMES = ("Qmi", "Qte", "Qncie", "Qm", "Qsf", "Qp")
DEFAULTS = {"q": 1.85, "alpha1": 1.0, "alpha2": 1.0, "min_wavelength": 3.0, "mult": 2.1, "sigma_onf": 0.55, "k": 2.0, "cutoff": 0.5,
            "g": 10.0, "eps": 1e-4, "C": 1e-4, "ep": 1.0, "eM": 1.0, "em": 1.0}
SCALES, ORIENTS = 4, 6


# ---------------------------------------------------------------------------------------------------------------------------------
# Information measures
# ---------------------------------------------------------------------------------------------------------------------------------
def marginal(X):
    return np.bincount(X.ravel(), minlength=256).astype(np.float64) / X.size


def joint(X, Y):
    return np.bincount(X.ravel() * 256 + Y.ravel(), minlength=65536).astype(np.float64).reshape(256, 256) / X.size


def entropy2(p):
    p = p[p > 0]
    return 0.0 - float(np.sum(p * np.log2(p)))


def mutual_information(X, Y):
    pxy, px, py = joint(X, Y), marginal(X), marginal(Y)
    nz = pxy > 0
    return float(np.sum(pxy[nz] * np.log2(pxy[nz] / np.outer(px, py)[nz])))


def qmi(F, A, B):
    total = 0.0
    for X in (A, B):
        den = entropy2(marginal(X)) + entropy2(marginal(F))
        total += 0.0 if den == 0.0 else mutual_information(X, F) / den
    return 2.0 * total


def tsallis_information(X, Y, q):
    pxy, pp = joint(X, Y), np.outer(marginal(X), marginal(Y))
    nz = pxy > 0
    return (1.0 - float(np.sum(pxy[nz] ** q / pp[nz] ** (q - 1.0)))) / (1.0 - q)


def tsallis_entropy(X, q):
    p = marginal(X)
    return (1.0 - float(np.sum(p[p > 0] ** q))) / (q - 1.0)


def qte(F, A, B, q):
    den = tsallis_entropy(A, q) + tsallis_entropy(B, q) - tsallis_information(A, B, q)
    return 0.0 if den == 0.0 else (tsallis_information(A, F, q) + tsallis_information(B, F, q)) / den


def jacobi_eigenvalues3(r01, r02, r12):
    """Eigenvalues of [[1, r01, r02], [r01, 1, r12], [r02, r12, 1]] by cyclic Jacobi sweeps."""
    a = np.array([[1.0, r01, r02], [r01, 1.0, r12], [r02, r12, 1.0]], dtype=np.float64)
    for _ in range(64):
        if a[0, 1] ** 2 + a[0, 2] ** 2 + a[1, 2] ** 2 <= 1e-60:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p, q]
            if apq == 0.0:
                continue
            theta = (a[q, q] - a[p, p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            r = 3 - p - q
            arp, arq = a[r, p], a[r, q]
            a[p, p] -= t * apq
            a[q, q] += t * apq
            a[p, q] = a[q, p] = 0.0
            a[r, p] = a[p, r] = c * arp - s * arq
            a[r, q] = a[q, r] = s * arp + c * arq
    return np.diag(a).copy()


def ncc(X, Y):
    return entropy2(marginal(X)) / 8.0 + entropy2(marginal(Y)) / 8.0 - entropy2(joint(X, Y)) / 8.0


def qncie(F, A, B):
    lam = jacobi_eigenvalues3(ncc(A, B), ncc(A, F), ncc(B, F))
    return 1.0 + float(sum((l / 3.0) * (np.log2(l / 3.0) / 8.0) for l in lam if l > 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# Qsf, Qm
# ---------------------------------------------------------------------------------------------------------------------------------
def differences(X):
    """D_h, D_v, D_md, D_sd of the integer image X, each over the pixels where both exist."""
    return X[:, 1:] - X[:, :-1], X[1:, :] - X[:-1, :], X[1:, 1:] - X[:-1, :-1], X[1:, :-1] - X[:-1, 1:]


def qsf(F, A, B):
    wd = 1.0 / np.sqrt(2.0)
    w = (1.0, 1.0, wd, wd)
    n = float(F.size)
    sf_f = np.sqrt(sum(wk * float(np.sum(d * d)) for wk, d in zip(w, differences(F))) / n)
    ref = [np.maximum(np.abs(da), np.abs(db)) for da, db in zip(differences(A), differences(B))]
    sf_r = np.sqrt(sum(wk * float(np.sum(d * d)) for wk, d in zip(w, ref)) / n)
    return 0.0 if sf_r == 0.0 else float((sf_f - sf_r) / sf_r)


def haar(X):
    """One scale of the decimated orthonormal Haar transform of the float image X -> (LL, LH, HL, HH); an odd trailing row or column
    is dropped."""
    h, w = X.shape[0] // 2 * 2, X.shape[1] // 2 * 2
    a, b, c, d = X[0:h:2, 0:w:2], X[0:h:2, 1:w:2], X[1:h:2, 0:w:2], X[1:h:2, 1:w:2]
    return (a + b + c + d) / 2.0, (a + b - c - d) / 2.0, (a - b + c - d) / 2.0, (a - b - c + d) / 2.0


def qm(F, A, B, alpha1, alpha2):
    x = {k: v.astype(np.float64) / 255.0 for k, v in (("F", F), ("A", A), ("B", B))}
    scales = []
    for _ in range(2):
        t = {k: haar(v) for k, v in x.items()}
        if t["F"][0].size == 0:
            scales.append(1.0)
        else:
            num = den = 0.0
            for k in ("A", "B"):
                ep = sum(np.exp(-np.abs(t[k][j] - t["F"][j])) for j in (1, 2, 3)) / 3.0
                wgt = t[k][1] ** 2 + t[k][2] ** 2 + t[k][3] ** 2
                num += float(np.sum(ep * wgt))
                den += float(np.sum(wgt))
            scales.append(0.0 if den == 0.0 else num / den)
        x = {k: v[0] for k, v in t.items()}
    return float(scales[0] ** alpha1 * scales[1] ** alpha2)


# ---------------------------------------------------------------------------------------------------------------------------------
# Qp
# ---------------------------------------------------------------------------------------------------------------------------------
def pc_filters(H, W, min_wavelength, mult, sigma_onf):
    """-> filt[s][o], the H x W filters G_s spread_o."""
    fy = signed_frequency(H)[:, None].astype(np.float64) / H * np.ones((1, W))
    fx = signed_frequency(W)[None, :].astype(np.float64) / W * np.ones((H, 1))
    rho = np.sqrt(fx * fx + fy * fy)
    rho[0, 0] = 1.0
    theta = np.arctan2(-fy, fx)
    lp = 1.0 / (1.0 + (rho / 0.45) ** 30)
    sint, cost = np.sin(theta), np.cos(theta)
    out = []
    for s in range(SCALES):
        fs = 1.0 / (min_wavelength * mult ** s)
        G = np.exp(-np.log(rho / fs) ** 2 / (2.0 * np.log(sigma_onf) ** 2)) * lp
        G[0, 0] = 0.0
        row = []
        for o in range(ORIENTS):
            a = o * np.pi / 6.0
            ds, dc = sint * np.cos(a) - cost * np.sin(a), cost * np.cos(a) + sint * np.sin(a)
            dth = np.minimum(np.abs(np.arctan2(ds, dc)) * 3.0, np.pi)
            row.append(G * ((np.cos(dth) + 1.0) / 2.0))
        out.append(row)
    return out


def phase_congruency(X, filt, mult, k, cutoff, g, eps, perturb=None):
    """-> (p, M, m) maps of the level image X.  perturb: a function applied to the spectrum (the tests' sensitivity measurement)."""
    spectrum = np.fft.fft2(X.astype(np.float64))
    if perturb is not None:
        spectrum = perturb(spectrum)
    p = np.zeros(X.shape)
    sxx, syy, sxy = np.zeros(X.shape), np.zeros(X.shape), np.zeros(X.shape)
    for o in range(ORIENTS):
        a = o * np.pi / 6.0
        EO = [np.fft.ifft2(spectrum * filt[s][o]) for s in range(SCALES)]
        An = [np.abs(e) for e in EO]
        sumE, sumO, sumAn = sum(e.real for e in EO), sum(e.imag for e in EO), sum(An)
        maxAn = np.maximum.reduce(An)
        XE = np.sqrt(sumE ** 2 + sumO ** 2) + eps
        mE, mO = sumE / XE, sumO / XE
        energy = sum(e.real * mE + e.imag * mO - np.abs(e.real * mO - e.imag * mE) for e in EO)
        tau = float(np.median(An[0])) / np.sqrt(np.log(4.0))
        tt = tau * (1.0 - (1.0 / mult) ** 4) / (1.0 - 1.0 / mult)
        T = tt * np.sqrt(np.pi / 2.0) + k * tt * np.sqrt((4.0 - np.pi) / 2.0)
        energy = np.maximum(energy - T, 0.0)
        width = (sumAn / (maxAn + eps) - 1.0) / 3.0
        weight = 1.0 / (1.0 + np.exp((cutoff - width) * g))
        pc = weight * energy / (sumAn + eps)
        p += pc
        sxx += (pc * np.cos(a)) ** 2
        syy += (pc * np.sin(a)) ** 2
        sxy += pc * pc * np.cos(a) * np.sin(a)
    cx2, cy2, cxy = sxx / 3.0, syy / 3.0, sxy / 3.0
    den = np.sqrt(cxy ** 2 + (cx2 - cy2) ** 2) + eps
    return p, (cy2 + cx2 + den) / 2.0, (cy2 + cx2 - den) / 2.0


def stabilised_correlation(U, V, C):
    du, dv = U - U.mean(), V - V.mean()
    return (float(np.mean(du * dv)) + C) / (float(np.sqrt(np.mean(du * du)) * np.sqrt(np.mean(dv * dv))) + C)


def qp(F, A, B, min_wavelength, mult, sigma_onf, k, cutoff, g, eps, C, ep, eM, em, perturb=None):
    filt = pc_filters(F.shape[0], F.shape[1], min_wavelength, mult, sigma_onf)
    maps = {n: phase_congruency(X, filt, mult, k, cutoff, g, eps, perturb) for n, X in (("A", A), ("B", B), ("F", F))}
    out = 1.0
    for j, e in enumerate((ep, eM, em)):
        xa, xb, xf = maps["A"][j], maps["B"][j], maps["F"][j]
        best = max(stabilised_correlation(xa, xf, C), stabilised_correlation(xb, xf, C), stabilised_correlation(np.maximum(xa, xb), xf, C), 0.0)
        out *= best ** e
    return float(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# The call
# ---------------------------------------------------------------------------------------------------------------------------------
def check_constants(c):
    """The refusals of the header."""
    ok = all(np.isfinite(v) for v in c.values()) and c["q"] > 0 and c["q"] != 1 and c["mult"] > 1 and 0 < c["sigma_onf"] < 1 \
        and c["min_wavelength"] >= 2 and c["eps"] > 0 and c["C"] > 0 and all(c[n] >= 0 for n in ("alpha1", "alpha2", "ep", "eM", "em"))
    if not ok:
        raise ValueError(f"constants {c}")


def image_comparative(fusion, ir, vis, perturb=None, **constants):
    """(H, W) float32 images -> the six values, float64."""
    unknown = set(constants) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown constant(s) {sorted(unknown)}")
    c = {**DEFAULTS, **constants}
    check_constants(c)
    F, A, B = quantise(fusion), quantise(ir), quantise(vis)
    return np.array([qmi(F, A, B), qte(F, A, B, c["q"]), qncie(F, A, B), qm(F, A, B, c["alpha1"], c["alpha2"]), qsf(F, A, B),
                     qp(F, A, B, c["min_wavelength"], c["mult"], c["sigma_onf"], c["k"], c["cutoff"], c["g"], c["eps"], c["C"], c["ep"],
                        c["eM"], c["em"], perturb)], dtype=np.float64)


def batch_comparative(fusion, ir, vis, perturb=None, **constants):
    """(B, 1, H, W) float32 arrays or CPU tensors -> (B, 6) float64."""
    f, i, v = (np.asarray(t, dtype=np.float32) for t in (fusion, ir, vis))
    return np.stack([image_comparative(f[b, 0], i[b, 0], v[b, 0], perturb=perturb, **constants) for b in range(f.shape[0])])
