"""BRISQUE oracle: a plain numpy fp64 restatement of the published MATLAB release (Mittal, Moorthy, Bovik 2012:
brisquescore.m, brisque_feature.m, estimateggdparam.m, estimateaggdparam.m) and of libsvm's svm-scale -r / svm-predict,
under the conventions this project pins (csrc/nriqa.hip states them in the same words):

  input     u = rint(255 * clip(v)) in fp32 (half to even), fp64 from here on; no crop: the whole frame is used
  MSCN      at each of two scales: mu = filter2(w, I, 'same'), sigma = sqrt(|filter2(w, I.*I) - mu^2|),
            M = (I - mu)/(sigma + 1); w: 7x7 Gaussian, sigma 7/6, sum 1; ZERO padding; the 49 taps accumulated row by row
  resize    MATLAB imresize(I, 0.5), bicubic, antialiased, symmetric borders: ceil(H/2) x ceil(W/2)
  features  18 per scale, 36 in all, scale 1 first.  GGD fit of all of M: rho = mean(M^2)/mean(|M|)^2, alpha = the grid
            point 0.2 + 0.001 k minimising |rho - G(1/a)G(3/a)/G(2/a)^2| -> [alpha, mean(M^2)].  For each circshift
            (0,1) (1,0) (1,1) (-1,1) of the whole frame (wrapping at its edges), the AGGD fit of P = M . circshift(M, s)
            (NIQE's estimateaggdparam) -> [alpha, (sr - sl) G(2/a)/G(1/a) sqrt(G(1/a)/G(3/a)), sl^2, sr^2].  Every grid
            search takes the first point on ties; a NaN ratio takes k = 0 (numpy's argmin); an empty AGGD side is NaN.
  scaling   svm-scale: x' = lower + (upper - lower)(x - min)/(max - min); x == min -> lower, x == max -> upper; a feature
            whose range has min == max is dropped (0 in the sparse vector)
  score     RBF SVR: sum_i coef_i exp(-gamma |x' - sv_i|^2) - rho, |.|^2 a sum of squared differences in feature order.
            A frame with any NaN feature scores NaN (a flat frame is one).  Nothing goes through the release's %f / %g
            text round trips: fp64 throughout.

Nothing here is shared with the kernels except these definitions.
"""
import math
import warnings

import numpy as np

from nriqa_ref import ALPHA, R_GAM, BETA_FACTOR, MEAN_FACTOR, gaussian_window, imresize_half, quantize

SHIFTS = ((0, 1), (1, 0), (1, 1), (-1, 1))          # circshift / np.roll (rows, cols), over the whole frame


def _ggd_table():
    g1 = np.array([math.gamma(1.0 / a) for a in ALPHA])
    g2 = np.array([math.gamma(2.0 / a) for a in ALPHA])
    g3 = np.array([math.gamma(3.0 / a) for a in ALPHA])
    return (g1 * g3) / (g2 * g2)


R_GGD = _ggd_table()


def filter2_zero(img, w):
    """filter2(w, img, 'same'): correlation with zero padding, the 49 taps accumulated row by row."""
    H, W = img.shape
    p = np.pad(img, 3, mode='constant')
    acc = np.zeros((H, W))
    for i in range(7):
        for j in range(7):
            acc = acc + w[i, j] * p[i:i + H, j:j + W]
    return acc


def mscn(img):
    w = gaussian_window()
    mu = filter2_zero(img, w)
    s2 = filter2_zero(img * img, w)
    sigma = np.sqrt(np.abs(s2 - mu * mu))
    return (img - mu) / (sigma + 1.0)


def ggd_fit(x):
    """estimateggdparam.m -> (alpha index k, mean(x^2), |rho - r| distances)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        msq = np.mean(x * x)
        e = np.mean(np.abs(x))
        rho = msq / (e * e)
        d = np.abs(rho - R_GGD)
    return int(np.argmin(d)), float(msq), d


def aggd_fit(x):
    """estimateaggdparam.m -> (alpha index k, leftstd, rightstd, squared distances)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        left, right = x[x < 0], x[x > 0]
        ls = np.sqrt(np.mean(left * left))
        rs = np.sqrt(np.mean(right * right))
        g = ls / rs
        ma = np.mean(np.abs(x))
        rhat = (ma * ma) / np.mean(x * x)
        rn = (rhat * (g * g * g + 1.0) * (g + 1.0)) / ((g * g + 1.0) * (g * g + 1.0))
        d = (R_GAM - rn) ** 2
    return int(np.argmin(d)), float(ls), float(rs), d


def pairs(m, shift):
    """P = M . circshift(M, shift) over the whole frame."""
    return m * np.roll(m, shift, axis=(0, 1))


def scale_features(m):
    """brisque_feature.m at one scale: 18 features of one MSCN map."""
    k, msq, _ = ggd_fit(m)
    feat = [ALPHA[k], msq]
    for s in SHIFTS:
        k, ls, rs, _ = aggd_fit(pairs(m, s))
        feat += [ALPHA[k], ((rs - ls) * MEAN_FACTOR[k]) * BETA_FACTOR[k], ls * ls, rs * rs]
    return feat


def features(v, clip=True):
    """The 36 BRISQUE features of one [H, W] frame in [0, 1]: scale 1, then scale 2 (imresize 0.5)."""
    img = quantize(v, clip)
    f1 = scale_features(mscn(img))
    f2 = scale_features(mscn(imresize_half(img)))
    return np.array(f1 + f2)


def svm_scale(x, fmin, fmax, lower=-1.0, upper=1.0):
    """svm-scale -r with an x section: a feature whose range has min == max is dropped (0)."""
    x, fmin, fmax = (np.asarray(a, dtype=np.float64) for a in (x, fmin, fmax))
    out = np.zeros_like(x)
    for k in range(len(x)):
        if fmin[k] == fmax[k]:
            continue
        if x[k] == fmin[k]:
            out[k] = lower
        elif x[k] == fmax[k]:
            out[k] = upper
        else:
            out[k] = lower + ((upper - lower) * (x[k] - fmin[k])) / (fmax[k] - fmin[k])
    return out


def svr_predict(xs, sv, coef, gamma, rho):
    """svm-predict for an epsilon / nu SVR with an RBF kernel: sum_i coef_i exp(-gamma |x - sv_i|^2) - rho."""
    sv = np.asarray(sv, dtype=np.float64).reshape(-1, 36)
    d = np.sum((np.asarray(xs, dtype=np.float64)[None, :] - sv) ** 2, axis=1)
    return float(np.sum(np.asarray(coef, dtype=np.float64) * np.exp(-gamma * d)) - rho)


def score_features(feat, model):
    if np.any(np.isnan(feat)):
        return float('nan')
    xs = svm_scale(feat, model['fmin'], model['fmax'], model['lower'], model['upper'])
    return svr_predict(xs, model['sv'], model['coef'], model['gamma'], model['rho'])


def brisque(v, model, clip=True):
    return score_features(features(v, clip), model)
