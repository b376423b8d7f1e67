"""VIF and Nabf / Labf of include/swinfuse.h (swf_fusion_fidelity) restated in numpy: the quantiser of tests/metrics_restatement.py,
everything after it in float64, VIF in the straightforward separable form (rows, then columns, then the decimation).  This is the
oracle of tests/test_fidelity_host.py (identities) and tests/test_gpu_fidelity.py (the kernels).  Restated from the published
definitions and the common open evaluators (vifp_mscale; Kumar's objective fusion performance scheme); parity with any MATLAB / VIFB /
sewar implementation is unpinned."""
import numpy as np

from tests.metrics_restatement import quantise

NAMES = ("VIF", "VIF_IR", "VIF_VIS", "Nabf", "Labf")
DEFAULTS = {"sigma_nsq": 2.0, "eps": 1e-10, "Td": 2.0, "wt_min": 0.001, "Nrg": 0.9999, "kg": 19.0, "sg": 0.5, "Nra": 0.9995, "ka": 22.0,
            "sa": 0.5}
TAPS = (17, 9, 5, 3)   # N = 2^(5 - s) + 1, s = 1..4


def window(n):
    """The normalised 1-D factor of the n x n Gaussian window, standard deviation n / 5."""
    i = np.arange(n, dtype=np.float64)
    g = np.exp(-((i - (n - 1) / 2) ** 2) / (2.0 * (n / 5.0) ** 2))
    return g / g.sum()


def filter_valid(X, g):
    """'valid' filtering of X (h, w) with outer(g, g): rows first, then columns, taps added in ascending order."""
    n = len(g)
    h, w = X.shape
    rows = np.zeros((h, w - n + 1))
    for k in range(n):
        rows += g[k] * X[:, k:k + w - n + 1]
    out = np.zeros((h - n + 1, w - n + 1))
    for k in range(n):
        out += g[k] * rows[k:k + h - n + 1, :]
    return out


def scale_shapes(h, w):
    """[(N, input height, input width)] of the scales that contribute to an h x w image."""
    out = []
    for s, n in enumerate(TAPS):
        if h < n or w < n:
            break
        if s > 0:
            h, w = (h - n + 2) // 2, (w - n + 2) // 2
            if h < n or w < n:
                break
        out.append((n, h, w))
    return out


def vifp(R, D, sigma_nsq=2.0, eps=1e-10):
    """-> (vifp(R, D), [per scale: number of pixels whose unclamped s1 or s2 lies within [eps / 3, 3 eps]]).  R, D: level images."""
    R, D = R.astype(np.float64), D.astype(np.float64)
    num = den = 0.0
    near = []
    for s, n in enumerate(TAPS):
        g = window(n)
        if R.shape[0] < n or R.shape[1] < n:
            break
        if s > 0:
            R, D = filter_valid(R, g)[::2, ::2], filter_valid(D, g)[::2, ::2]
            if R.shape[0] < n or R.shape[1] < n:
                break
        mu1, mu2 = filter_valid(R, g), filter_valid(D, g)
        s1 = filter_valid(R * R, g) - mu1 * mu1
        s2 = filter_valid(D * D, g) - mu2 * mu2
        s12 = filter_valid(R * D, g) - mu1 * mu2
        near.append(int(np.count_nonzero(((s1 >= eps / 3) & (s1 <= 3 * eps)) | ((s2 >= eps / 3) & (s2 <= 3 * eps)))))
        s1, s2 = np.maximum(s1, 0.0), np.maximum(s2, 0.0)
        gg = s12 / (s1 + eps)
        sv = s2 - gg * s12
        m = s1 < eps
        gg[m], sv[m], s1[m] = 0.0, s2[m], 0.0
        m = s2 < eps
        gg[m], sv[m] = 0.0, 0.0
        m = gg < 0
        sv[m], gg[m] = s2[m], 0.0
        sv[sv <= eps] = eps
        num += float(np.sum(np.log10(1.0 + gg * gg * s1 / (sv + sigma_nsq))))
        den += float(np.sum(np.log10(1.0 + s1 / sigma_nsq)))
    return (0.0 if den == 0.0 else num / den), near


def sobel_replicated(X):
    """The unnormalised sums 8 gv, 8 gh with a replicated border: gv with [-1 0 1; -2 0 2; -1 0 1], gh with [-1 -2 -1; 0 0 0; 1 2 1].
    Exact integers."""
    P = np.pad(X.astype(np.int64), 1, mode="edge")
    H, W = X.shape
    a, b, c = P[0:H, 0:W], P[0:H, 1:W + 1], P[0:H, 2:W + 2]
    d, e = P[1:H + 1, 0:W], P[1:H + 1, 2:W + 2]
    f, g, h = P[2:H + 2, 0:W], P[2:H + 2, 1:W + 1], P[2:H + 2, 2:W + 2]
    return (c - a) + 2 * (e - d) + (h - f), (f + 2 * g + h) - (a + 2 * b + c)


def _edge(X):
    gv, gh = sobel_replicated(X)
    n = gv * gv + gh * gh   # 64 g^2
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(gh == 0, np.sign(gv) * (np.pi / 2), np.arctan(gv.astype(np.float64) / gh.astype(np.float64)))
    return n, np.sqrt(n.astype(np.float64)) / 8.0, alpha


def nabf_parts(F, A, B, Td=2.0, wt_min=0.001, Nrg=0.9999, kg=19.0, sg=0.5, Nra=0.9995, ka=22.0, sa=0.5):
    """-> (Nabf, Labf, sum(Q_AF w_A + Q_BF w_B) / W) of level images."""
    nF, gF, aF = _edge(F)
    loss = np.zeros(F.shape)
    kept = np.zeros(F.shape)
    wsum = np.zeros(F.shape)
    na = np.ones(F.shape, dtype=bool)
    for X in (A, B):
        nX, gX, aX = _edge(X)
        with np.errstate(divide="ignore", invalid="ignore"):
            G = np.where((nX == 0) | (nF == 0), 0.0, np.where(nX > nF, gF / gX, gX / gF))
        Aa = np.abs(np.abs(aX - aF) - np.pi / 2) * (2 / np.pi)
        Q = np.sqrt(Nrg / (1.0 + np.exp(-kg * (G - sg))) * (Nra / (1.0 + np.exp(-ka * (Aa - sa)))))
        w = np.where(nX.astype(np.float64) >= 64.0 * Td * Td, gX * np.sqrt(gX), wt_min)
        loss += (1.0 - Q) * w
        kept += Q * w
        wsum += w
        na &= nF > nX
    W = float(np.sum(wsum))
    return float(np.sum(np.where(na, loss, 0.0))) / W, float(np.sum(np.where(na, 0.0, loss))) / W, float(np.sum(kept)) / W


def image_fidelity(fusion, ir, vis, with_near=False, **constants):
    """The five values of one image: fusion, ir, vis are (H, W) float32 arrays.  with_near: also the near-threshold pixel counts of
    vifp, {"IR": [per scale], "VIS": [per scale]}."""
    unknown = set(constants) - set(DEFAULTS)
    assert not unknown, unknown
    c = {**DEFAULTS, **constants}
    F, A, B = quantise(fusion), quantise(ir), quantise(vis)
    va, near_a = vifp(A, F, c["sigma_nsq"], c["eps"])
    vb, near_b = vifp(B, F, c["sigma_nsq"], c["eps"])
    nabf, labf, _ = nabf_parts(F, A, B, **{k: c[k] for k in ("Td", "wt_min", "Nrg", "kg", "sg", "Nra", "ka", "sa")})
    row = np.array([va + vb, va, vb, nabf, labf], dtype=np.float64)
    return (row, {"IR": near_a, "VIS": near_b}) if with_near else row


def batch_fidelity(fusion, ir, vis, with_near=False, **constants):
    """(B, 1, H, W) float32 arrays or CPU tensors -> (B, 5) float64 (and the list of per-image near-threshold counts)."""
    f, i, v = (np.asarray(t, dtype=np.float32) for t in (fusion, ir, vis))
    res = [image_fidelity(f[b, 0], i[b, 0], v[b, 0], with_near=with_near, **constants) for b in range(f.shape[0])]
    if with_near:
        return np.stack([r for r, _ in res]), [n for _, n in res]
    return np.stack(res)
