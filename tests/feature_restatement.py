"""Feature mutual information of include/swinfuse.h (FMI_pixel, FMI_dct, FMI_w, FMI_edge) restated in numpy float64: what the HIP kernels
of csrc/kernels_feature.hip are checked against.  The text is the header's, written from memory of Haghighat & Razian's method and of
the common open evaluators; parity with any of them is unpinned.  Vectorised over the windows with sliding_window_view; the DCT through
scipy.fft.dctn (`dct_plane_matrix` is the header's cosine-matrix product, which the host tests hold the snapped planes of to the bit);
`window_information_loop` is the same text as a plain triple loop over one window.

A = ir, B = vis, F = fusion as 8-bit levels (tests/metrics_restatement.quantise)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.fft import dctn

from tests.metrics_restatement import quantise

NAMES = ("FMI_pixel", "FMI_dct", "FMI_w", "FMI_edge")
DEFAULTS = {"window": 3.0, "dct_step": 2.0 ** -16}
FEATURES = ("pixel", "dct", "w", "edge")   # the order of NAMES


# ---------------------------------------------------------------------------------------------------------------------------------
# Feature planes
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_plane(X):
    """|sx| + |sy| of the 3x3 Sobel pair on the levels with replicated borders."""
    p = np.pad(X.astype(np.int64), 1, mode="edge")
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, e = p[1:-1, :-2], p[1:-1, 2:]
    f, g, h = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    sx = (c - a) + 2 * (e - d) + (h - f)
    sy = (a + 2 * b + c) - (f + 2 * g + h)
    return (np.abs(sx) + np.abs(sy)).astype(np.float64)


def haar_plane(X):
    """The mosaic [LL LH; HL HH] of one level of the decimated orthonormal Haar transform; an odd trailing row or column is dropped."""
    hh, wh = X.shape[0] // 2, X.shape[1] // 2
    x = X[:2 * hh, :2 * wh].astype(np.float64)
    a, b, c, d = x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]
    out = np.empty((2 * hh, 2 * wh), dtype=np.float64)
    out[:hh, :wh] = (a + b + c + d) / 2.0
    out[:hh, wh:] = (a + b - c - d) / 2.0
    out[hh:, :wh] = (a - b + c - d) / 2.0
    out[hh:, wh:] = (a - b - c + d) / 2.0
    return out


def snap(T, step):
    return np.rint(T / step) * step


def dct_plane(X, step):
    return snap(dctn(X.astype(np.float64), type=2, norm="ortho"), step)


def dct_matrix(n):
    """D_n[k][i] = s_k sqrt(2 / n) cos(pi ((2 i + 1) k mod 4 n) / (2 n))."""
    k, i = np.arange(n, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    m = ((2 * i + 1) * k) % (4 * n)
    s = np.where(k == 0, 1.0 / np.sqrt(2.0), 1.0)
    return s * np.sqrt(2.0 / n) * np.cos(np.pi * (m.astype(np.float64) / (2 * n)))


def dct_plane_matrix(X, step):
    h, w = X.shape
    return snap(dct_matrix(h) @ X.astype(np.float64) @ dct_matrix(w).T, step)


def feature_plane(X, feature, step):
    if feature == "pixel":
        return X.astype(np.float64)
    if feature == "edge":
        return edge_plane(X)
    if feature == "w":
        return haar_plane(X)
    if feature == "dct":
        return dct_plane(X, step)
    raise ValueError(feature)


# ---------------------------------------------------------------------------------------------------------------------------------
# FMI of one feature
# ---------------------------------------------------------------------------------------------------------------------------------
def windows(T, win):
    """-> (count, win^2): every window wholly inside the plane, its samples column-major."""
    if T.shape[0] < win or T.shape[1] < win:
        return np.zeros((0, win * win), dtype=np.float64)
    v = sliding_window_view(T, (win, win))               # (oh, ow, row offset, column offset)
    return np.ascontiguousarray(v.transpose(0, 1, 3, 2)).reshape(-1, win * win)


def _pdf(x):
    mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    flat = mx == mn
    xn = np.where(flat, 1.0, (x - mn) / np.where(flat, 1.0, mx - mn))
    return xn / xn.sum(axis=1, keepdims=True)


def _entropy(t):
    safe = np.where(t > 0, t, 1.0)
    return 0.0 - np.sum(np.where(t > 0, t * np.log2(safe), 0.0), axis=tuple(range(1, t.ndim)))


def pair_information(x, f, with_info=False):
    """x, f: (count, l) window samples -> I(X, F) per window."""
    n, l = x.shape
    same = np.all(x == f, axis=1)
    p, q = _pdf(x), _pdf(f)
    P, Q = np.cumsum(p, axis=1), np.cumsum(q, axis=1)
    pc, qc = p - 1.0 / l, q - 1.0 / l
    den = np.sqrt(np.sum(pc * pc, axis=1) * np.sum(qc * qc, axis=1))
    c = np.where(den == 0.0, 0.0, np.sum(pc * qc, axis=1) / np.where(den == 0.0, 1.0, den))
    k = np.arange(1, l + 1, dtype=np.float64)
    sigma = lambda t: np.sqrt(np.maximum(np.sum(k * k * t, axis=1) - np.sum(k * t, axis=1) ** 2, 0.0))
    ss = sigma(p) * sigma(q)
    Pi, Qj = P[:, :, None], Q[:, None, :]
    G = np.where((c >= 0.0)[:, None, None], np.minimum(Pi, Qj), np.maximum(Pi + Qj - 1.0, 0.0))
    PQ = Pi * Qj
    rho = np.where(ss == 0.0, 0.0, np.sum(G - PQ, axis=(1, 2)) / np.where(ss == 0.0, 1.0, ss))
    ratio = c / np.where(rho == 0.0, 1.0, rho)
    phi = np.where(rho == 0.0, 0.0, np.clip(ratio, 0.0, 1.0))
    J = phi[:, None, None] * G + (1.0 - phi)[:, None, None] * PQ
    Jp = np.zeros((n, l + 1, l + 1), dtype=np.float64)   # J = 0 at index -1
    Jp[:, 1:, 1:] = J
    j = (Jp[:, 1:, 1:] - Jp[:, :-1, 1:]) - (Jp[:, 1:, :-1] - Jp[:, :-1, :-1])
    hs = _entropy(p) + _entropy(q)
    info = np.where(hs == 0.0, 0.0, 2.0 * (hs - _entropy(j)) / np.where(hs == 0.0, 1.0, hs))
    info = np.where(same, 1.0, info)
    if with_info:
        live = ~same
        return info, {"windows": n, "same": int(same.sum()), "negative_c": int(np.sum(live & (c < 0.0))),
                      "ratio_above_1": int(np.sum(live & (rho != 0.0) & (ratio > 1.0))),
                      "ratio_below_0": int(np.sum(live & (rho != 0.0) & (ratio < 0.0)))}
    return info


def window_information_loop(x, f):
    """The same text for one window, as plain loops over k, i and j."""
    l = len(x)
    if all(x[k] == f[k] for k in range(l)):
        return 1.0

    def pdf(v):
        mn, mx = min(v), max(v)
        vn = [1.0 if mx == mn else (t - mn) / (mx - mn) for t in v]
        s = 0.0
        for t in vn:
            s += t
        return [t / s for t in vn]

    def cdf(p):
        out, run = [], 0.0
        for t in p:
            run += t
            out.append(run)
        return out

    def entropy(ts):
        h = 0.0
        for t in ts:
            if t > 0:
                h -= t * np.log2(t)
        return h

    p, q = pdf(x), pdf(f)
    P, Q = cdf(p), cdf(q)
    spp = spq = sqq = 0.0
    mup = m2p = muq = m2q = 0.0
    for k in range(l):
        pc, qc = p[k] - 1.0 / l, q[k] - 1.0 / l
        spp, sqq, spq = spp + pc * pc, sqq + qc * qc, spq + pc * qc
        mup, m2p = mup + (k + 1) * p[k], m2p + (k + 1) ** 2 * p[k]
        muq, m2q = muq + (k + 1) * q[k], m2q + (k + 1) ** 2 * q[k]
    den = np.sqrt(spp * sqq)
    c = 0.0 if den == 0.0 else spq / den
    ss = np.sqrt(max(m2p - mup * mup, 0.0)) * np.sqrt(max(m2q - muq * muq, 0.0))
    G = lambda a, b: min(a, b) if c >= 0.0 else max(a + b - 1.0, 0.0)
    excess = 0.0
    for i in range(l):
        for j in range(l):
            excess += G(P[i], Q[j]) - P[i] * Q[j]
    rho = 0.0 if ss == 0.0 else excess / ss
    phi = 0.0 if rho == 0.0 else min(max(c / rho, 0.0), 1.0)
    J = lambda i, j: 0.0 if i < 0 or j < 0 else phi * G(P[i], Q[j]) + (1.0 - phi) * (P[i] * Q[j])
    cells = []
    for i in range(l):
        for j in range(l):
            cells.append((J(i, j) - J(i - 1, j)) - (J(i, j - 1) - J(i - 1, j - 1)))
    hs = entropy(p) + entropy(q)
    return 0.0 if hs == 0.0 else 2.0 * (hs - entropy(cells)) / hs


def feature_fmi(TA, TB, TF, win, with_info=False):
    """FMI of one feature from its three planes: the mean over the windows of (I(A, F) + I(B, F)) / 2; 0 without a window."""
    a, b, f = windows(TA, win), windows(TB, win), windows(TF, win)
    if a.shape[0] == 0:
        return (0.0, []) if with_info else 0.0
    ia, info_a = pair_information(a, f, with_info=True)
    ib, info_b = pair_information(b, f, with_info=True)
    value = float(np.sum((ia + ib) / 2.0) / a.shape[0])
    return (value, [info_a, info_b]) if with_info else value


def _constants(constants):
    unknown = set(constants) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown constant(s) {sorted(unknown)}")
    c = {**DEFAULTS, **constants}
    if c["window"] not in (3.0, 5.0) or not np.isfinite(c["dct_step"]) or not c["dct_step"] > 0.0:
        raise ValueError(f"constants {c}")
    return int(c["window"]), float(c["dct_step"])


def image_feature(fusion, ir, vis, with_info=False, **constants):
    """-> the four NAMES values of one image (2-D float32 arrays of one shape)."""
    win, step = _constants(constants)
    F, A, B = (quantise(np.asarray(x)) for x in (fusion, ir, vis))
    out, infos = np.zeros(len(NAMES), dtype=np.float64), {}
    for n, feature in enumerate(FEATURES):
        out[n], infos[feature] = feature_fmi(*(feature_plane(X, feature, step) for X in (A, B, F)), win, with_info=True)
    return (out, infos) if with_info else out


def batch_feature(fusion, ir, vis, **constants):
    """(B, 1, H, W) float32 tensors or arrays -> (B, 4) float64."""
    f, i, v = (np.asarray(x, dtype=np.float32) for x in (fusion, ir, vis))
    return np.stack([image_feature(f[b, 0], i[b, 0], v[b, 0], **constants) for b in range(f.shape[0])])
