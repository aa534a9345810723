"""VIFp (Sheikh & Bovik, "Image Information and Visual Quality", IEEE TIP 2006, in its pixel-domain multi-scale form:
vifp_mscale.m of the LIVE release, sewar.vifp) restated in numpy fp64: the oracle csrc/vifp.hip is held to.  The conventions, in
the words of the kernel's header comment -- for one frame pair `img` (the reconstruction, "distorted") and `ref`, both float32
[H, W]:

  0. input     with clip, both are clamped to [0,1] in fp32; then x = 255.0 * (double)ref, y = 255.0 * (double)img.  Nothing is
               quantised to bytes; everything from here on is fp64.
  1. windows   scale s = 1..4 has N = 2^(5-s) + 1 = 17, 9, 5, 3 taps, w_k = exp(-(k - (N-1)/2)^2 / (2 (N/5)^2)) normalised to sum 1;
               F(a) is the window w (x) w over the VALID region only, as two separable passes, axis 0 first and then axis 1, the
               taps added in index order (a = w0*v0; a += wk*vk).
  2. pyramid   for s > 1: x = F(x)[::2, ::2], y = F(y)[::2, ::2] with this scale's own window: a side becomes
               ceil((side - N + 1) / 2).
  3. moments   mu1 = F(x), mu2 = F(y), s1 = F(x*x) - mu1*mu1, s2 = F(y*y) - mu2*mu2, s12 = F(x*y) - mu1*mu2;
               s1 = max(s1, 0), s2 = max(s2, 0); g = s12 / (s1 + EPS); sv = s2 - g*s12; then, in this order:
               s1 < EPS: g = 0, sv = s2, s1 = 0;  s2 < EPS: g = 0, sv = 0;  g < 0: sv = s2, g = 0;  sv <= EPS: sv = EPS.
  4. score     num_s = sum log10(1 + g*g*s1 / (sv + sigma_nsq)), den_s = sum log10(1 + s1 / sigma_nsq);
               vifp = (sum_s num_s) / (sum_s den_s), no epsilon: a reference that is flat everywhere gives NaN.

EPS = 1e-10 and the bare ratio follow the MATLAB release and sewar (piq.vif_p uses 1e-8 in both places).  Needs
min(H, W) >= 41: the sides go 41 -> 17 -> 7 -> 3.  `taps` (a list of four arrays) replaces numpy's own windows, so that a test can
hand in the bits the kernels use (evr_vifp_taps): with identical taps and operation order every threshold falls the same way.
"""
import numpy as np

SIGMA_NSQ = 2.0
EPS = 1e-10
SCALES = 4
MIN_SIDE = 41


def window(scale):
    """The N = 2^(5 - scale) + 1 taps of scale 1..4, summed in index order before the division."""
    N = 2 ** (5 - scale) + 1
    d = np.arange(N, dtype=np.float64) - (N - 1) / 2.0
    sd = N / 5.0
    w = np.exp(-(d * d) / (2.0 * sd * sd))
    total = 0.0
    for v in w:
        total += float(v)
    return w / total


def filt(a, w):
    """F(a): the separable window over the valid region, axis 0 first, taps added in index order."""
    N = len(w)
    h, wd = a.shape
    t = w[0] * a[0:h - N + 1, :]
    for k in range(1, N):
        t = t + w[k] * a[k:k + h - N + 1, :]
    u = w[0] * t[:, 0:wd - N + 1]
    for k in range(1, N):
        u = u + w[k] * t[:, k:k + wd - N + 1]
    return u


def _check(img, ref):
    img, ref = np.asarray(img), np.asarray(ref)
    if img.ndim != 2 or img.shape != ref.shape:
        raise ValueError(f"vifp takes two [H, W] frames of one shape, got {img.shape} and {ref.shape}")
    if min(img.shape) < MIN_SIDE:
        raise ValueError(f"vifp needs frames of at least {MIN_SIDE}x{MIN_SIDE} pixels, got {img.shape[0]}x{img.shape[1]}")
    return img, ref


def _planes(v, clip):
    v = np.asarray(v, dtype=np.float32)
    if clip:
        v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))
    return 255.0 * v.astype(np.float64)


def terms(img, ref, clip=True, taps=None, filt=filt):
    """-> per scale (the log10 terms of num, of den, s1 after its clamp, s2 after its clamp): the maps before they are summed."""
    img, ref = _check(img, ref)
    x, y = _planes(ref, clip), _planes(img, clip)
    out = []
    for s in range(1, SCALES + 1):
        w = np.asarray(taps[s - 1], dtype=np.float64) if taps is not None else window(s)
        if s > 1:
            x, y = filt(x, w)[::2, ::2], filt(y, w)[::2, ::2]
        mu1, mu2 = filt(x, w), filt(y, w)
        s1 = filt(x * x, w) - mu1 * mu1
        s2 = filt(y * y, w) - mu2 * mu2
        s12 = filt(x * y, w) - mu1 * mu2
        s1 = np.where(s1 < 0.0, 0.0, s1)
        s2 = np.where(s2 < 0.0, 0.0, s2)
        v1, v2 = s1.copy(), s2.copy()
        g = s12 / (s1 + EPS)
        sv = s2 - g * s12
        m = s1 < EPS
        g[m] = 0.0; sv[m] = s2[m]; s1[m] = 0.0
        m = s2 < EPS
        g[m] = 0.0; sv[m] = 0.0
        m = g < 0.0
        sv[m] = s2[m]; g[m] = 0.0
        sv[sv <= EPS] = EPS
        out.append((np.log10(1.0 + ((g * g) * s1) / (sv + SIGMA_NSQ)), np.log10(1.0 + s1 / SIGMA_NSQ), v1, v2))
    return out


def scales(img, ref, clip=True, taps=None, filt=filt):
    """-> float64 [4, 2]: (num_s, den_s)."""
    return np.array([[np.sum(n), np.sum(d)] for n, d, _, _ in terms(img, ref, clip, taps, filt)], dtype=np.float64)


def vifp(img, ref, clip=True, taps=None, filt=filt):
    """The score; NaN where the reference is flat everywhere."""
    sc = scales(img, ref, clip, taps, filt)
    num = ((sc[0, 0] + sc[1, 0]) + sc[2, 0]) + sc[3, 0]
    den = ((sc[0, 1] + sc[1, 1]) + sc[2, 1]) + sc[3, 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float64(num) / np.float64(den))


def min_variances(img, ref, clip=True, taps=None):
    """-> (the smallest s1, the smallest s2) over all windows and scales: how far the pair stays from the thresholds."""
    t = terms(img, ref, clip, taps)
    return min(float(v1.min()) for _, _, v1, _ in t), min(float(v2.min()) for _, _, _, v2 in t)
