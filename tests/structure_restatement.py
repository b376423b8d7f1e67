"""SSIM, MS-SSIM and the Piella / Cvejic / Yang indices of include/swinfuse.h (swf_fusion_structure) restated in numpy: the quantiser
of tests/metrics_restatement.py, the Gaussian group in float64 in the straightforward separable form (rows, then columns), the box
group on integer arrays (window sums, V and C in int64, every zero test on them) with one float64 expression per window.  This is the
oracle of tests/test_structure_host.py (identities) and tests/test_gpu_structure.py (the kernels).  Restated from the published
definitions; parity with any MATLAB or toolbox implementation is unpinned."""
import numpy as np

from tests.metrics_restatement import quantise, sobel

NAMES = ("SSIM", "SSIM_IR", "SSIM_VIS", "MS_SSIM", "Qs", "Qw", "Qe", "Qc", "Qy")
DEFAULTS = {"K1": 0.01, "K2": 0.03, "alpha": 1.0, "Ty": 0.75}
TAPS, SIGMA = 11, 1.5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_MIN = TAPS << (len(MS_WEIGHTS) - 1)   # 176: the smallest axis whose scale-5 plane holds one window
NEAR = 1e-9                              # |s(A, B) - Ty| within which a 7x7 window counts as near Yang's threshold


def window():
    """The normalised 1-D factor of the 11 x 11 Gaussian window, standard deviation 1.5."""
    i = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-((i - (TAPS - 1) // 2) ** 2) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def filter_valid(X, g):
    """'valid' filtering of X (h, w) with outer(g, g): rows first, then columns, taps added in ascending order."""
    n = len(g)
    h, w = X.shape
    rows = np.zeros((h, w - n + 1), dtype=X.dtype)
    for k in range(n):
        rows += g[k] * X[:, k:k + w - n + 1]
    out = np.zeros((h - n + 1, w - n + 1), dtype=X.dtype)
    for k in range(n):
        out += g[k] * rows[k:k + h - n + 1, :]
    return out


def constants(K1, K2):
    return (255.0 * K1) ** 2, (255.0 * K2) ** 2


def ssim_means(X, Y, C1, C2, filt=filter_valid, g=None):
    """-> (mean(l cs), mean(cs)) of two float planes of at least 11 x 11: biased moments, not clamped."""
    g = window() if g is None else g
    mx, my = filt(X, g), filt(Y, g)
    vx = filt(X * X, g) - mx * mx
    vy = filt(Y * Y, g) - my * my
    cxy = filt(X * Y, g) - mx * my
    l = (2.0 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2.0 * cxy + C2) / (vx + vy + C2)
    return (l * cs).sum() / l.size, cs.sum() / l.size


def mean2x2(X):
    """The mean of the non-overlapping 2x2 blocks: floor(h / 2) x floor(w / 2), an odd last row or column dropped."""
    h, w = X.shape[0] // 2, X.shape[1] // 2
    X = X[:2 * h, :2 * w]
    return 0.25 * ((X[0::2, 0::2] + X[0::2, 1::2]) + (X[1::2, 0::2] + X[1::2, 1::2]))


def ssim(X, Y, C1, C2, **kw):
    """ssim(X, Y) of level images; exactly 0 under 11 pixels in an axis."""
    if min(X.shape) < TAPS:
        return 0.0
    return float(ssim_means(X.astype(np.float64), Y.astype(np.float64), C1, C2, **kw)[0])


def msssim(X, Y, C1, C2, with_scales=False, dtype=np.float64, **kw):
    """msssim(X, Y) of level images; exactly 0 under 176 pixels in an axis.  with_scales: also the list of (mean l cs, mean cs)."""
    if min(X.shape) < MS_MIN:
        return (0.0, []) if with_scales else 0.0
    X, Y = X.astype(dtype), Y.astype(dtype)
    value, scales = dtype(1.0), []
    for j, wj in enumerate(MS_WEIGHTS):
        if j > 0:
            X, Y = mean2x2(X), mean2x2(Y)
        lcs, cs = ssim_means(X, Y, C1, C2, **kw)
        scales.append((float(lcs), float(cs)))
        v = lcs if j == len(MS_WEIGHTS) - 1 else cs
        value = value * max(v, dtype(0.0)) ** dtype(wj)
    return (float(value), scales) if with_scales else float(value)


def box_sums(X, w):
    """Sums of the integer image X over every valid w x w window (int64; exact)."""
    I = np.zeros((X.shape[0] + 1, X.shape[1] + 1), dtype=np.int64)
    I[1:, 1:] = X.astype(np.int64).cumsum(0).cumsum(1)
    return I[w:, w:] - I[:-w, w:] - I[w:, :-w] + I[:-w, :-w]


def box_moments(F, A, B, w):
    """-> dict of the integer arrays S_X, V_X, C_XY of the header over the valid w x w windows of three integer images."""
    n = w * w
    F, A, B = (X.astype(np.int64) for X in (F, A, B))
    S = {k: box_sums(X, w) for k, X in (("A", A), ("B", B), ("F", F))}
    m = dict(n=n, SA=S["A"], SB=S["B"], SF=S["F"])
    for k, X in (("A", A), ("B", B), ("F", F)):
        m["V" + k] = n * box_sums(X * X, w) - S[k] * S[k]
    for k, (X, Y) in (("AF", (A, F)), ("BF", (B, F)), ("AB", (A, B))):
        m["C" + k] = n * box_sums(X * Y, w) - S[k[0]] * S[k[1]]
    return m


def s_index(SX, SY, VX, VY, CXY, n, C1, C2):
    n2 = float(n) * float(n)
    mx, my = SX / float(n), SY / float(n)
    vx, vy, cxy = VX / n2, VY / n2, CXY / n2
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def _ratio(num, den):
    """num / den on integer arrays as float64, 1/2 where den = 0 (the test is made on the integers)."""
    zero = den == 0
    return np.where(zero, 0.5, num.astype(np.float64) / np.where(zero, 1, den).astype(np.float64)), zero


def box_terms(F, A, B, w, C1, C2):
    """Per window: s(A, F), s(B, F), s(A, B), lambda, t, m (int64), and the masks of the two zero rules."""
    m = box_moments(F, A, B, w)
    n = m["n"]
    sAF = s_index(m["SA"], m["SF"], m["VA"], m["VF"], m["CAF"], n, C1, C2)
    sBF = s_index(m["SB"], m["SF"], m["VB"], m["VF"], m["CBF"], n, C1, C2)
    sAB = s_index(m["SA"], m["SB"], m["VA"], m["VB"], m["CAB"], n, C1, C2)
    lam, v_zero = _ratio(m["VA"], m["VA"] + m["VB"])
    sim, c_zero = _ratio(m["CAF"], m["CAF"] + m["CBF"])
    sim = np.clip(sim, 0.0, 1.0)
    return dict(sAF=sAF, sBF=sBF, sAB=sAB, lam=lam, t=lam * sAF + (1.0 - lam) * sBF, m=np.maximum(m["VA"], m["VB"]), sim=sim,
                v_zero=v_zero, c_zero=c_zero)


def piella(F, A, B, C1, C2):
    """-> (Qs, Qw, Qc, terms) of three integer images with 8x8 windows."""
    x = box_terms(F, A, B, 8, C1, C2)
    qs = float(x["t"].sum() / x["t"].size)
    sm = int(x["m"].sum())
    qw = qs if sm == 0 else float((x["m"].astype(np.float64) * x["t"]).sum() / float(sm))
    qc = float((x["sim"] * x["sAF"] + (1.0 - x["sim"]) * x["sBF"]).sum() / x["t"].size)
    x["m_zero"] = sm == 0
    return qs, qw, qc, x


def edge_image(X):
    """E = |sx| + |sy| of the QABF section's Sobel responses (zero border): integers of at most 2040."""
    sx, sy = sobel(X)
    return np.abs(sx) + np.abs(sy)


def yang(F, A, B, C1, C2, Ty):
    """-> (Qy, number of windows within NEAR of Ty, fraction of windows on the >= Ty side)."""
    x = box_terms(F, A, B, 7, C1, C2)
    high = x["sAB"] >= Ty
    q = np.where(high, x["t"], np.maximum(x["sAF"], x["sBF"]))
    return float(q.sum() / q.size), int(np.count_nonzero(np.abs(x["sAB"] - Ty) <= NEAR)), float(high.mean()), x


def image_structure(fusion, ir, vis, with_near=False, with_info=False, **constants_):
    """The nine values of one image: fusion, ir, vis are (H, W) float32 arrays.  with_near: also the count of 7x7 windows with
    |s(A, B) - Ty| <= 1e-9.  with_info: also a dict of which rules the image took."""
    unknown = set(constants_) - set(DEFAULTS)
    assert not unknown, unknown
    c = {**DEFAULTS, **constants_}
    C1, C2 = constants(c["K1"], c["K2"])
    F, A, B = quantise(fusion), quantise(ir), quantise(vis)
    sa, sb = ssim(A, F, C1, C2), ssim(B, F, C1, C2)
    (ma, sc_a), (mb, sc_b) = msssim(A, F, C1, C2, with_scales=True), msssim(B, F, C1, C2, with_scales=True)
    row = np.zeros(len(NAMES), dtype=np.float64)
    row[:4] = sa + sb, sa, sb, ma + mb
    near, info = 0, {"v_zero": 0, "c_zero": 0, "edge_v_zero": 0, "m_zero": False, "high": None,
                     "min_cs": min([cs for _, cs in sc_a + sc_b], default=None)}
    if min(F.shape) >= 8:
        qs, qw, qc, x = piella(F, A, B, C1, C2)
        _, qw_edge, _, xe = piella(edge_image(F), edge_image(A), edge_image(B), C1, C2)
        row[4:8] = qs, qw, qw * max(qw_edge, 0.0) ** c["alpha"], qc
        info.update(v_zero=int(x["v_zero"].sum()), c_zero=int(x["c_zero"].sum()), edge_v_zero=int(xe["v_zero"].sum()), m_zero=x["m_zero"])
    if min(F.shape) >= 7:
        row[8], near, info["high"], _ = yang(F, A, B, C1, C2, c["Ty"])
    out = (row,)
    if with_near:
        out += (near,)
    if with_info:
        out += (info,)
    return out if len(out) > 1 else row


def batch_structure(fusion, ir, vis, with_near=False, with_info=False, **constants_):
    """(B, 1, H, W) float32 arrays or CPU tensors -> (B, 9) float64 (with_near: and the per-image near-threshold counts; with_info: and the
    per-image rule reports)."""
    f, i, v = (np.asarray(t, dtype=np.float32) for t in (fusion, ir, vis))
    res = [image_structure(f[b, 0], i[b, 0], v[b, 0], with_near=with_near, with_info=with_info, **constants_) for b in range(f.shape[0])]
    if not (with_near or with_info):
        return np.stack(res)
    return (np.stack([r[0] for r in res]),) + tuple([r[k] for r in res] for k in range(1, len(res[0])))
