"""PIQE oracle: a plain numpy fp64 restatement of N. Venkatanath, D. Praneeth, M. Chandrasekhar Bh, S. S. Channappayya,
S. S. Medasani, "Blind image quality evaluation using perception based features", NCC 2015, as MATLAB's `piqe` and pyiqa's
`piqe` compute it, under the conventions this project pins (csrc/nriqa.hip states them in the same words).  Opinion-unaware
and training-free: no model file, no weights.

  input     u = rint(255 * clip(v)) in fp32 (half to even), fp64 from here on
  padding   bottom and right up to multiples of 16 by edge replication (MATLAB's padarray(..., 'replicate', 'post')),
            THEN the filter
  MSCN      mu = G*u, sigma = sqrt(|G*(u.u) - mu^2|), m = (u - mu)/(sigma + 1); G: NIQE's 7x7 Gaussian, sigma 7/6, sum 1,
            a correlation with a replicate border over the padded image, the 49 taps accumulated row by row
  block     per 16 x 16 block of m: var = the unbiased variance of its 256 values (N - 1); active iff var > 0.1
  whsa      (noticeable artefacts) the four edges of an active block -- first row, last row, first column, last column --
            have 16 values and 11 sliding segments of length 6 each; set iff any of the 44 segments has an unbiased
            standard deviation < 0.1
  wnc       (noise) centre = the two central columns (0-based 7 and 8, 32 values), surround = the other 14 columns (224
            values); r = std(centre)/std(surround), unbiased, a NaN ratio (0/0) becomes 0; sg = sqrt(var),
            beta = |sg - r| / max(sg, r); set iff sg > 2 beta
  block     contribution: 1 - var if whsa (with or without wnc), var if only wnc, 0 otherwise
  score     100 (sum of contributions + 1) / (1 + number of active blocks); a frame with no active block (a constant
            frame) scores exactly 100: the formula's own value, not a special case
  NaN       comparisons with NaN are false

The centre columns and the 'post' padding are this project's reading of the ports, stated here as conventions: parity with
pyiqa is unpinned until tests/test_piqe_pins.py has run on a box that has pyiqa.

Nothing here is shared with the kernels except these definitions.
"""
import warnings

import numpy as np

from nriqa_ref import gaussian_window, quantize

BLOCK = 16
ACTIVITY_THRESHOLD = 0.1
EDGE_THRESHOLD = 0.1
SEGMENT = 6
CENTRE = (7, 8)                 # 0-based columns of the block
ACTIVE, WHSA, WNC = 1, 2, 4     # the bits of a block's flag byte (evr_piqe_blocks)


def pad_post(u):
    """padarray(u, [ph pw], 'replicate', 'post'): bottom and right up to multiples of 16."""
    H, W = u.shape
    return np.pad(u, ((0, -H % BLOCK), (0, -W % BLOCK)), mode='edge')


def filter_replicate(img, w):
    """Correlation with a replicate border, the 49 taps accumulated row by row."""
    H, W = img.shape
    p = np.pad(img, 3, mode='edge')
    acc = np.zeros((H, W))
    for i in range(7):
        for j in range(7):
            acc = acc + w[i, j] * p[i:i + H, j:j + W]
    return acc


def mscn_parts(img):
    """(mu, sigma, m) of one fp64 image."""
    w = gaussian_window()
    mu = filter_replicate(img, w)
    s2 = filter_replicate(img * img, w)
    sigma = np.sqrt(np.abs(s2 - mu * mu))
    return mu, sigma, (img - mu) / (sigma + 1.0)


def unbiased_var(x):
    """sum((x - mean)^2) / (N - 1) over all of x (two passes)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    d = x - np.sum(x) / x.size
    return float(np.sum(d * d) / (x.size - 1))


def edges(block):
    """The four edges of a 16 x 16 block: first row, last row, first column, last column."""
    return [block[0, :], block[-1, :], block[:, 0], block[:, -1]]


def segment_stds(block):
    """[4, 11]: the unbiased standard deviation of every length-6 sliding segment of every edge."""
    out = np.empty((4, BLOCK - SEGMENT + 1))
    for e, edge in enumerate(edges(block)):
        for s in range(BLOCK - SEGMENT + 1):
            out[e, s] = np.sqrt(unbiased_var(edge[s:s + SEGMENT]))
    return out


def noise_quantities(block, var):
    """-> (sg, beta) of the noise criterion."""
    cols = np.zeros(BLOCK, bool)
    cols[list(CENTRE)] = True
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        r = np.sqrt(unbiased_var(block[:, cols])) / np.sqrt(unbiased_var(block[:, ~cols]))
        if np.isnan(r):
            r = 0.0
        sg = np.sqrt(var)
        beta = np.abs(sg - r) / np.maximum(sg, r)
    return float(sg), float(beta)


def blocks(v, clip=True):
    """One [H, W] frame -> dict of [ceil(H/16), ceil(W/16)] arrays: var (fp64), flags (uint8: ACTIVE | WHSA | WNC),
    contribution (fp64) and margin (fp64: the smallest distance of a deciding quantity from its threshold -- |var - 0.1|,
    and for an active block |segstd - 0.1| over the 44 segments and |sg - 2 beta|; NaN distances are left out)."""
    m = mscn_parts(pad_post(quantize(v, clip)))[2]
    nby, nbx = m.shape[0] // BLOCK, m.shape[1] // BLOCK
    var = np.empty((nby, nbx))
    flags = np.zeros((nby, nbx), np.uint8)
    contribution = np.zeros((nby, nbx))
    margin = np.empty((nby, nbx))
    for by in range(nby):
        for bx in range(nbx):
            b = m[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK]
            bv = unbiased_var(b)
            var[by, bx] = bv
            dist = [abs(bv - ACTIVITY_THRESHOLD)]
            if bv > ACTIVITY_THRESHOLD:
                seg = segment_stds(b)
                whsa = bool(np.any(seg < EDGE_THRESHOLD))
                sg, beta = noise_quantities(b, bv)
                wnc = bool(sg > 2.0 * beta)
                flags[by, bx] = ACTIVE | (WHSA if whsa else 0) | (WNC if wnc else 0)
                contribution[by, bx] = (1.0 - bv) if whsa else (bv if wnc else 0.0)
                dist += list(np.abs(seg - EDGE_THRESHOLD).ravel()) + [abs(sg - 2.0 * beta)]
            dist = [d for d in dist if not np.isnan(d)]
            margin[by, bx] = min(dist) if dist else np.inf
    return dict(var=var, flags=flags, contribution=contribution, margin=margin)


def score_blocks(b):
    active = int(np.count_nonzero(b['flags'] & ACTIVE))
    return float(100.0 * ((np.sum(b['contribution']) + 1.0) / (1.0 + active)))


def piqe(v, clip=True):
    return score_blocks(blocks(v, clip))


def block_class(flags):
    """0 inactive, 1 active and unflagged, 2 whsa only, 3 wnc only, 4 both."""
    f = np.asarray(flags).astype(np.int64)
    return np.where(f & ACTIVE, np.array([1, 0, 2, 0, 3, 0, 4])[f & (WHSA | WNC)], 0)


# ---- the input set of tests/test_gpu_piqe.py (tests/test_piqe_cpu.py holds it to coverage of the five block classes and to a
# margin of every deciding quantity from its threshold) ------------------------------------------------------------------------
def texture(H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return 0.5 + 0.25 * np.sin(xx / (4.0 + seed % 3)) * np.cos(yy / 6.0) + 0.1 * np.sin((xx + 2.0 * yy) / 17.0)


def block_average(a, k=8):
    """k x k block averaging (each k x k cell replaced by its mean; ragged cells at the bottom and right by theirs)."""
    out = np.empty_like(a)
    for y in range(0, a.shape[0], k):
        for x in range(0, a.shape[1], k):
            out[y:y + k, x:x + k] = a[y:y + k, x:x + k].mean()
    return out


def inputs():
    """[(name, float32 [H, W])], seeded."""
    rng = np.random.default_rng(2015)
    out = [('8x8', rng.random((8, 8))),
           ('16x16', rng.random((16, 16))),
           ('17x33', rng.random((17, 33))),
           ('81x113 uniform noise', rng.random((81, 113))),
           ('81x113 texture + noise', texture(81, 113, 1) + 0.03 * rng.standard_normal((81, 113))),
           ('96x128 block-averaged', block_average(texture(96, 128, 2) + 0.1 * rng.standard_normal((96, 128)))),
           ('40x40 constant', np.full((40, 40), 0.4))]
    mix = texture(260, 346, 3)
    mix[:, :173] = block_average(mix[:, :173] + 0.1 * rng.standard_normal((260, 173)))
    mix[:, 173:] = mix[:, 173:] + 0.04 * rng.standard_normal((260, 173))
    out.append(('260x346 mix', mix))
    return [(n, np.ascontiguousarray(a, dtype=np.float32)) for n, a in out]


UNCLIPPED = ('81x113 texture + noise', '260x346 mix')      # also run with clip=False and values outside [0, 1]


def unclipped(a):
    """The frame stretched beyond [0, 1] (and a few codes beyond 255 / below 0 after quantisation)."""
    return np.ascontiguousarray(1.6 * a - 0.3, dtype=np.float32)
