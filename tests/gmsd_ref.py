"""GMSD (Xue, Zhang, Mou & Bovik, "Gradient Magnitude Similarity Deviation", IEEE TIP 2014; pyiqa's `gmsd`) restated in numpy
fp64: the oracle csrc/gmsd.hip is held to.  The conventions, in the words of the kernel's header comment -- for one frame pair
`img`, `ref`, both float32 [H, W]:

  1. luminance  u = rint(255 * clip(v, 0, 1)) in float32, round half to even, then exact in fp64 (what the NIQE, BRISQUE and
                PIQE kernels do; pyiqa's to_y_channel(x, 255) on a grey frame replicated to three channels is recalled to round
                the same way: a convention until tests/test_gmsd_pins.py has run).  With clip = 0 the clamp is left out and
                the rounding stays.
  2. pooling    2x2 mean at stride 2 with no padding: h2 = H // 2, w2 = W // 2, a trailing odd row or column is dropped (it
                does not exist in the pooled plane).  p = 0.25 * (((a00 + a01) + a10) + a11): exact, the inputs being integers.
  3. gradients  Prewitt on the pooled plane with zero padding of one pixel (F.conv2d(..., padding=1) in pyiqa, conv2 'same' in
                MATLAB), indices [row offset, column offset], the three-term sums added left to right:
                gx = ((p[-1,-1] + p[0,-1] + p[+1,-1]) - (p[-1,+1] + p[0,+1] + p[+1,+1])) / 3,
                gy the same with the roles of row and column exchanged (the sign does not reach the score);
                g = sqrt((gx*gx + gy*gy) + 1e-12).
  4. GMS map    q = (2 * g_img * g_ref + 170) / ((g_img^2 + g_ref^2) + 170), so q in (0, 1].
  5. score      the standard deviation of q over the N = h2 * w2 pooled pixels with N - 1 in the denominator (torch.std's
                default, MATLAB's std2).  The kernel forms it from the moments of d = 1 - q:
                var = (sum d^2 - (sum d)^2 / N) / (N - 1), clamped at 0 before the square root; the oracle takes the two-pass
                value.  Needs H >= 2 and W >= 2; N == 1 gives NaN, as torch.std does.

Everything from step 1's output onward is fp64.  The score is symmetric in its two arguments to the last bit: (2a) * b is an
exact scaling and the two additions commute.
"""
import numpy as np

C = 170.0
EPS = 1e-12


def luminance(v, clip=True):
    v = np.asarray(v, dtype=np.float32)
    if clip:
        v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))
    return np.rint(np.float32(255.0) * v).astype(np.float64)


def pool(u):
    """2x2 mean, stride 2, no padding: a trailing odd row or column is dropped."""
    h2, w2 = u.shape[0] // 2, u.shape[1] // 2
    u = u[:2 * h2, :2 * w2]
    return 0.25 * (((u[0::2, 0::2] + u[0::2, 1::2]) + u[1::2, 0::2]) + u[1::2, 1::2])


def gradient_magnitude(p):
    """Prewitt / 3 with one pixel of zero padding."""
    h, w = p.shape
    z = np.zeros((h + 2, w + 2), np.float64)
    z[1:-1, 1:-1] = p
    s = lambda dr, dc: z[1 + dr:1 + dr + h, 1 + dc:1 + dc + w]
    gx = (((s(-1, -1) + s(0, -1)) + s(1, -1)) - ((s(-1, 1) + s(0, 1)) + s(1, 1))) / 3.0
    gy = (((s(-1, -1) + s(-1, 0)) + s(-1, 1)) - ((s(1, -1) + s(1, 0)) + s(1, 1))) / 3.0
    return np.sqrt((gx * gx + gy * gy) + EPS)


def _check(img, ref):
    img, ref = np.asarray(img), np.asarray(ref)
    if img.ndim != 2 or img.shape != ref.shape:
        raise ValueError(f"gmsd takes two [H, W] frames of one shape, got {img.shape} and {ref.shape}")
    if min(img.shape) < 2:
        raise ValueError(f"gmsd needs frames of at least 2x2 pixels, got {img.shape[0]}x{img.shape[1]}")
    return img, ref


def gms_map(img, ref, clip=True):
    """-> q [H // 2, W // 2] float64."""
    img, ref = _check(img, ref)
    ga = gradient_magnitude(pool(luminance(img, clip)))
    gb = gradient_magnitude(pool(luminance(ref, clip)))
    return ((2.0 * ga) * gb + C) / ((ga * ga + gb * gb) + C)


def gmsd(img, ref, clip=True):
    """The score: std of the GMS map with N - 1 (two-pass); NaN for a single pooled pixel."""
    q = gms_map(img, ref, clip)
    if q.size == 1:
        return float('nan')
    return float(np.std(q, ddof=1))


def mean_gms(img, ref, clip=True):
    return float(np.mean(gms_map(img, ref, clip)))
