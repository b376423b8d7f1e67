"""The fusion-quality metrics of include/swinfuse.h (swf_fusion_metrics) restated in numpy: the quantiser in float32 with its two
roundings, everything after it in float64 over pixels.  This is the oracle of tests/test_metrics_host.py (hand arithmetic and
identities) and tests/test_gpu_metrics.py (the kernels).  Restated from the published definitions and the common open evaluators;
parity with any MATLAB / VIFB implementation is unpinned."""
import numpy as np

NAMES = ("EN", "MI", "SD", "SF", "AG", "CC", "SCD", "MSE", "PSNR", "Qabf")
QABF_DEFAULTS = {"Tg": 0.9994, "kg": -15.0, "Dg": 0.5, "Ta": 0.9879, "ka": -22.0, "Da": 0.8}


def quantise(x):
    """torchvision save_image's levels: float32 multiply, float32 add (two roundings), clamp, truncate; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.add(np.multiply(x, np.float32(255.0), dtype=np.float32), np.float32(0.5), dtype=np.float32)
        v = np.fmin(np.fmax(v, np.float32(0.0)), np.float32(255.0))
    return v.astype(np.int64)


def entropy(F):
    p = np.bincount(F.ravel(), minlength=256).astype(np.float64) / F.size
    p = p[p > 0]
    return 0.0 - float(np.sum(p * np.log2(p)))


def mutual_information(X, Y):
    n = X.size
    pxy = np.bincount(X.ravel() * 256 + Y.ravel(), minlength=65536).astype(np.float64).reshape(256, 256) / n
    px, py = pxy.sum(axis=1, keepdims=True), pxy.sum(axis=0, keepdims=True)
    m = pxy > 0
    return float(np.sum(pxy[m] * np.log2(pxy[m] / (px * py)[m])))


def pearson(X, Y):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    dx, dy = X - X.mean(), Y - Y.mean()
    vx, vy = np.mean(dx * dx), np.mean(dy * dy)
    if vx == 0.0 or vy == 0.0:
        return 0.0
    return float(np.mean(dx * dy) / np.sqrt(vx * vy))


def sobel(X):
    """Responses with a zero border: sx with [-1 0 1; -2 0 2; -1 0 1], sy with [1 2 1; 0 0 0; -1 -2 -1], applied as written (conv2's flip
    negates both, which changes neither g nor sy / sx).  Exact integers."""
    P = np.pad(X.astype(np.int64), 1)
    H, W = X.shape
    a, b, c = P[0:H, 0:W], P[0:H, 1:W + 1], P[0:H, 2:W + 2]
    d, e = P[1:H + 1, 0:W], P[1:H + 1, 2:W + 2]
    f, g, h = P[2:H + 2, 0:W], P[2:H + 2, 1:W + 1], P[2:H + 2, 2:W + 2]
    return (c - a) + 2 * (e - d) + (h - f), (a + 2 * b + c) - (f + 2 * g + h)


def _edge(X):
    sx, sy = sobel(X)
    n = sx * sx + sy * sy
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(sx == 0, np.pi / 2, np.arctan(sy.astype(np.float64) / sx.astype(np.float64)))
    return n, np.sqrt(n.astype(np.float64)), alpha


def qabf(F, A, B, Tg=0.9994, kg=-15.0, Dg=0.5, Ta=0.9879, ka=-22.0, Da=0.8):
    nF, gF, aF = _edge(F)
    terms = []
    for X in (A, B):
        nX, gX, aX = _edge(X)
        with np.errstate(divide="ignore", invalid="ignore"):
            G = np.where(nX > nF, gF / gX, np.where(nX == nF, gF, gX / gF))
        Aa = 1.0 - np.abs(aX - aF) / (np.pi / 2)
        Q = Tg / (1.0 + np.exp(kg * (G - Dg))) * (Ta / (1.0 + np.exp(ka * (Aa - Da))))
        terms.append((Q * gX, gX))
    num = float(np.sum(terms[0][0] + terms[1][0]))
    den = float(np.sum(terms[0][1] + terms[1][1]))
    return 0.0 if den == 0.0 else num / den


def image_metrics(fusion, ir, vis, **qabf_constants):
    """The ten values of one image: fusion, ir, vis are (H, W) float32 arrays."""
    F, A, B = quantise(fusion), quantise(ir), quantise(vis)
    H, W = F.shape
    Fd, Ad, Bd = F.astype(np.float64), A.astype(np.float64), B.astype(np.float64)
    en = entropy(F)
    mi = mutual_information(F, A) + mutual_information(F, B)
    sd = float(np.sqrt(np.mean((Fd - Fd.mean()) ** 2)))
    rf2 = float(np.mean((Fd[:, 1:] - Fd[:, :-1]) ** 2)) if W > 1 else 0.0
    cf2 = float(np.mean((Fd[1:, :] - Fd[:-1, :]) ** 2)) if H > 1 else 0.0
    sf = float(np.sqrt(rf2 + cf2))
    if H > 1 and W > 1:
        gx, gy = Fd[:-1, 1:] - Fd[:-1, :-1], Fd[1:, :-1] - Fd[:-1, :-1]
        ag = float(np.mean(np.sqrt((gx * gx + gy * gy) / 2.0)))
    else:
        ag = 0.0
    cc = (pearson(A, F) + pearson(B, F)) / 2.0
    scd = pearson(F - B, A) + pearson(F - A, B)
    mse = (float(np.mean((Fd - Ad) ** 2)) + float(np.mean((Fd - Bd) ** 2))) / 2.0
    psnr = float("inf") if mse == 0.0 else float(10.0 * np.log10(255.0 * 255.0 / mse))
    return np.array([en, mi, sd, sf, ag, cc, scd, mse, psnr, qabf(F, A, B, **qabf_constants)], dtype=np.float64)


def batch_metrics(fusion, ir, vis, **qabf_constants):
    """(B, 1, H, W) float32 arrays or CPU tensors -> (B, 10) float64."""
    f, i, v = (np.asarray(t, dtype=np.float32) for t in (fusion, ir, vis))
    return np.stack([image_metrics(f[b, 0], i[b, 0], v[b, 0], **qabf_constants) for b in range(f.shape[0])])
