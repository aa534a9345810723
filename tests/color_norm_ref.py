"""numpy restatement of the post-process normalisation of a merged colour frame (uint8 BGR [H,W,3]) as the reference applies it in
colour mode, down to the bytes of the PNG -- evreal_amd/csrc/color.hip, evr_color_percentile_normalize.  TEST INFRASTRUCTURE ONLY
(nothing in evreal_amd/ imports this).

  direct(u8, norm)   the float path: float32(u8)/255 (exp of that for 'exprobust'), np.percentile over all 3*H*W values together,
                     (img - lo) / (hi - lo), clip to [0,1], round(. * 255) as uint8; 0/0 = NaN (hi == lo) becomes byte 0.
  table(u8, norm)    the same bytes from the frame's 256-bin histogram alone: the percentile rule in float32 scalars (q/100,
                     (n-1)*q, gamma, numpy's _lerp), a 256-entry value table and a 256-entry byte table.  This is the form the
                     kernels compute; tests/test_color_norm_cpu.py holds it to direct().
  frame(kind, ...)   the seeded test frames both test files use."""
import numpy as np

F32 = np.float32
NORMS = ('robust', 'standard', 'exprobust')
KINDS = ('uniform', 'four_levels', 'dark_clipped', 'band_outliers', 'constant', 'two_levels')


def percentiles(norm):
    return (0, 100) if norm == 'standard' else (1, 99)


def values(norm):
    """byte level -> float32 image value"""
    v = np.arange(256).astype(np.uint8).astype(F32) / F32(255)
    return np.exp(v) if norm == 'exprobust' else v


def _bytes(img):
    """what the image writer stores: round(clip(img, 0, 1) * 255), NaN -> 0"""
    img = np.where(np.isnan(img), F32(0), img)
    return np.round(np.clip(img, 0, 1) * F32(255)).astype(np.uint8)


def direct(u8, norm):
    """-> (bytes uint8 like u8, lo, hi)"""
    assert u8.dtype == np.uint8 and norm in NORMS
    img = u8.astype(F32) / F32(255)
    if norm == 'exprobust':
        img = np.exp(img)
    q_lo, q_hi = percentiles(norm)
    lo = np.percentile(img.ravel(), q_lo)
    hi = np.percentile(img.ravel(), q_hi)
    assert lo.dtype == F32 and hi.dtype == F32
    with np.errstate(divide='ignore', invalid='ignore'):
        img = (img - lo) / (hi - lo)
    assert img.dtype == F32
    return _bytes(img), lo, hi


def _percentile_from_counts(cum, val, q100):
    n = int(cum[-1])
    q = F32(q100) / F32(100)
    vi = F32(n - 1) * q
    prev = int(np.floor(vi)); nxt = prev + 1
    if vi >= F32(n - 1):
        prev = nxt = n - 1; gamma = vi - F32(-1)
    elif vi < 0:
        prev = nxt = 0; gamma = vi - F32(0)
    else:
        gamma = vi - F32(prev)
    a = val[np.searchsorted(cum, prev, side='right')]       # the level of the byte of rank prev: first level with cum > prev
    b = val[np.searchsorted(cum, nxt, side='right')]
    diff = b - a
    r = a + diff * gamma
    if gamma >= F32(0.5):
        r = b - diff * (F32(1) - gamma)
    assert r.dtype == F32
    return r


def table(u8, norm):
    """-> (bytes uint8 like u8, lo, hi), through the histogram"""
    assert u8.dtype == np.uint8 and norm in NORMS
    val = values(norm)
    cum = np.cumsum(np.bincount(u8.ravel(), minlength=256))
    q_lo, q_hi = percentiles(norm)
    lo = _percentile_from_counts(cum, val, q_lo)
    hi = _percentile_from_counts(cum, val, q_hi)
    with np.errstate(divide='ignore', invalid='ignore'):
        tab = _bytes((val - lo) / (hi - lo))
    return tab[u8], lo, hi


def frame(kind, H, W, seed):
    """One uint8 [H,W,3] test frame."""
    rng = np.random.default_rng([seed, KINDS.index(kind), H, W])
    n = 3 * H * W
    if kind == 'uniform':
        a = rng.integers(0, 256, n)
    elif kind == 'four_levels':                 # four adjacent levels only
        a = int(rng.integers(0, 252)) + rng.integers(0, 4, n)
    elif kind == 'dark_clipped':                # most of the frame clipped at 0
        a = np.clip(rng.normal(-20.0, 30.0, n), 0, 255)
    elif kind == 'band_outliers':               # 99.5 % in three levels, the rest at 255: the 99th percentile is in the band, the 100th is not
        a = 100 + rng.integers(0, 3, n)
        a[rng.choice(n, max(1, n // 200), replace=False)] = 255
    elif kind == 'constant':
        a = np.full(n, int(rng.integers(0, 256)))
    elif kind == 'two_levels':                  # 0.2 % at level 200, the rest at 60: lo == hi for (1, 99), not for (0, 100)
        a = np.full(n, 60)
        a[rng.choice(n, max(1, n // 500), replace=False)] = 200
    else:
        raise ValueError(kind)
    return a.astype(np.uint8).reshape(H, W, 3)
