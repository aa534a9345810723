"""numpy restatement (fp64) of the two full-reference metrics of evreal_amd/csrc/frmetrics.hip: pyiqa's `psnr` and `ms_ssim` on
[0,1] gray frames with data_range 1 -- Wang, Simoncelli & Bovik 2003 in the form pytorch-msssim computes it.  TEST INFRASTRUCTURE
ONLY (nothing in evreal_amd/ imports this); tests/test_frmetrics_cpu.py holds it to a conv2d / avg_pool2d restatement in float64
and, at scale 1, to scikit-image's SSIM."""
import math

import numpy as np

W5 = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
MIN_SIDE = 161                       # pytorch-msssim: min(H, W) > (11 - 1) * 2 ** 4


def gauss():
    r = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-0.5 * r * r / 2.25)
    return g / g.sum()


def filt_valid(a, g):
    """The 11-tap window along axis 0 then axis 1, over the valid region only: [H, W] -> [H - 10, W - 10]."""
    H, W = a.shape
    t = sum(g[k] * a[k:H - 10 + k, :] for k in range(11))
    return sum(g[k] * t[:, k:W - 10 + k] for k in range(11))


def pool(a):
    """F.avg_pool2d(a, 2, padding=(H % 2, W % 2)): an odd side gets one zero row / column on BOTH ends, zeros counted."""
    H, W = a.shape
    ph, pw = H % 2, W % 2
    b = np.zeros((H + 2 * ph, W + 2 * pw))
    b[ph:ph + H, pw:pw + W] = a
    Ho, Wo = (H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1
    b = b[:2 * Ho, :2 * Wo]
    return 0.25 * (b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2])


def scale_stats(X, Y, g, C1=1e-4, C2=9e-4):
    """-> (S_l, CS_l): the means of the SSIM map and of the contrast-structure map of one scale."""
    ux, uy = filt_valid(X, g), filt_valid(Y, g)
    vx = filt_valid(X * X, g) - ux * ux
    vy = filt_valid(Y * Y, g) - uy * uy
    vxy = filt_valid(X * Y, g) - ux * uy
    cs = (2 * vxy + C2) / (vx + vy + C2)
    return ((2 * ux * uy + C1) / (ux * ux + uy * uy + C1) * cs).mean(), cs.mean()


def level_sizes(H, W):
    out = [(H, W)]
    for _ in range(4):
        H, W = pool(np.zeros((H, W))).shape
        out.append((H, W))
    return out


def ms_ssim(img, ref, clip=True):
    """float32 [H, W] pair, min(H, W) >= 161 -> (score, [(S_l, CS_l) for the five scales])."""
    X, Y = np.asarray(ref, np.float64), np.asarray(img, np.float64)
    if min(X.shape) < MIN_SIDE:
        raise ValueError(f"ms_ssim needs frames of at least {MIN_SIDE}x{MIN_SIDE} pixels")
    if clip:
        X, Y = np.clip(X, 0, 1), np.clip(Y, 0, 1)
    g, per = gauss(), []
    for l in range(5):
        per.append(scale_stats(X, Y, g))
        if l < 4:
            X, Y = pool(X), pool(Y)
    v = np.array([max(per[l][1], 0.0) for l in range(4)] + [max(per[4][0], 0.0)])
    return float(np.prod(v ** W5)), per


def scales_row(per):
    """The kernels' per-scale layout: CS_1..5, then S_1..5."""
    return np.array([p[1] for p in per] + [p[0] for p in per])


def combine(row):
    """The product formula on a CS_1..5, S_1..5 row."""
    row = np.asarray(row, np.float64)
    v = np.maximum(np.concatenate([row[:4], row[9:10]]), 0.0)
    return float(np.prod(v ** W5))


def psnr(img, ref, clip=True):
    """10 log10(1 / (mse + 1e-8)); mse as oracle.metrics.mse: fp32 difference and square, fp64 mean."""
    a, b = (np.clip(x, 0, 1) if clip else x for x in (np.asarray(ref, np.float32), np.asarray(img, np.float32)))
    d = (a - b).astype(np.float32)
    return 10.0 * math.log10(1.0 / (float(np.mean((d * d).astype(np.float32), dtype=np.float64)) + 1e-8))
