"""Which selection path of evr_percentile_normalize (csrc/prepost.hip) a frame takes, decided on the CPU, and the named frames the
path tests run.

classify() restates the BRANCH DECISION of pct_select_fast_kernel in numpy -- pct_rank in float32, the evenly spaced sample, the
rank window around the expected sample rank, the two sentinels, the f2key order, the count below the bracket and inside it, the `ok`
condition -- and the launcher's conditions for the four-pass kernel.  It never computes a percentile: it classifies inputs, it does
not judge results.  PCT_S and PCT_CAP are read out of the kernel source, so a changed constant moves the classification (and fails
tests/test_pct_paths_cpu.py) rather than silently un-covering a branch.

    fast       the bracket holds and the candidate list fits: the one-pass select answers
    overflow   more than PCT_CAP keys inside the bracket (ties at the percentile): four-pass fallback
    miss_low   next >= below + candidates: the sample put the bracket too low, fallback
    miss_high  below > prev: the sample put the bracket too high, fallback
    slow       the launcher takes pct_select_kernel: H*W % 4 != 0, H*W < 1024 or a base that is not 16-B aligned
"""
import os
import re

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'evreal_amd', 'csrc', 'prepost.hip')
CLASSES = ('fast', 'overflow', 'miss_low', 'miss_high', 'slow')
QS = (0.0, 1.0, 99.0, 100.0)          # 'standard' is (0, 100), 'robust' / 'exprobust' are (1, 99)
FAST_MIN_PX = 1024                    # the launcher's `px >= 1024`


def kernel_constants():
    """(PCT_S, PCT_CAP) as csrc/prepost.hip declares them."""
    with open(SOURCE) as f:
        src = f.read()
    out = []
    for name in ('PCT_S', 'PCT_CAP'):
        m = re.findall(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, src)
        assert len(m) == 1, (name, m)
        out.append(int(m[0]))
    return tuple(out)


def f2key(a):
    """The kernel's order-preserving float -> unsigned map (-0.0 sorts below +0.0)."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def pct_rank(n, q100):
    """csrc/pct.h pct_rank: (prev, next) of numpy's 'linear' rule, every operation one float32 rounding."""
    q = F32(q100) / F32(100.0)
    vi = F32(n - 1) * q
    prev = int(np.floor(vi)); nxt = prev + 1
    if vi >= F32(n - 1):
        prev = nxt = n - 1
    elif vi < F32(0):
        prev = nxt = 0
    return prev, nxt


def bracket(frame, q100, S=None, cap=None):
    """The numbers the `ok` condition of pct_select_fast_kernel sees: dict(prev, next, below, cand, overflow)."""
    if S is None or cap is None:
        S, cap = kernel_constants()
    keys = f2key(np.asarray(frame, dtype=F32).ravel())
    n = keys.size
    prev, nxt = pct_rank(n, q100)
    s = min(n, S)
    sample = np.sort(keys[(np.arange(s, dtype=np.int64) * n) // s])
    sr = F32(prev) * F32(s) / F32(n)
    var = sr * (F32(1.0) - sr / F32(s))
    d = 24 + int(F32(4.0) * np.sqrt(var if var > 0 else F32(0.0)))
    r_lo, r_hi = int(sr) - d, int(sr) + d + 1
    lo_t = np.uint32(0) if r_lo <= 0 else sample[r_lo]
    hi_t = np.uint32(0xFFFFFFFF) if r_hi >= s - 1 else sample[r_hi]
    below = int((keys < lo_t).sum())
    cand = int(((keys >= lo_t) & (keys <= hi_t)).sum())
    return dict(prev=prev, next=nxt, below=below, cand=cand, overflow=cand > cap)


def classify(frame, q100, aligned=True, S=None, cap=None):
    """One of CLASSES for the work-group that selects percentile q100 of `frame` (any shape, float32)."""
    n = int(np.asarray(frame).size)
    if n % 4 != 0 or n < FAST_MIN_PX or not aligned:
        return 'slow'
    b = bracket(frame, q100, S, cap)
    if b['overflow']:
        return 'overflow'
    if b['below'] > b['prev']:
        return 'miss_high'
    if b['next'] >= b['below'] + b['cand']:
        return 'miss_low'
    return 'fast'


# ---------------------------------------------------------------------------------------------------------------- the case table
H0, W0 = 96, 128                      # 12288 px: with S = 4096 the sampled positions are every third pixel


def _uniform(seed, shape=(H0, W0)):
    return np.random.default_rng(seed).random(shape, dtype=F32)


def _pinned(seed, value, shape=(H0, W0)):
    """uniform, 75 % of the pixels set to `value`"""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=F32)
    a[rng.random(shape) < 0.75] = F32(value)
    return a


def _sample_lies(seed):
    """uniform, but every SAMPLED pixel is tiny (even sample index) or close to 1 (odd): the sample's order statistics say nothing
    about the frame's, so both brackets miss -- without a single tie"""
    rng = np.random.default_rng(seed)
    S, _ = kernel_constants()
    a = rng.random(H0 * W0, dtype=F32)
    idx = (np.arange(S, dtype=np.int64) * a.size) // S
    u = rng.random(S, dtype=F32)
    a[idx[0::2]] = F32(0.002) * u[0::2]
    a[idx[1::2]] = F32(1.0) - F32(0.002) * u[1::2]
    return a.reshape(H0, W0)


def _dense_band(seed):
    """the sampled pixels uniform in (0, 1), every other pixel (8192 of them, all different) inside a band 1e-4 wide at the 1st
    percentile of the sample: that bracket holds, but with more DISTINCT keys than the list does -- the fallback has to tell them
    apart down to the last radix level (and the frame's 99th percentile lies far below the sample's)"""
    rng = np.random.default_rng(seed)
    S, _ = kernel_constants()
    a = (F32(0.0100) + F32(0.0001) * rng.permutation(H0 * W0).astype(F32) / F32(H0 * W0)).astype(F32)
    idx = (np.arange(S, dtype=np.int64) * a.size) // S
    a[idx] = rng.random(S, dtype=F32)
    return a.reshape(H0, W0)


def _pm_zero(seed, neg, zero):
    """a share `neg` of -0.0, `zero - neg` of +0.0, the rest uniform in (0.1, 1)"""
    rng = np.random.default_rng(seed)
    r = rng.random((H0, W0))
    a = (F32(0.1) + F32(0.9) * rng.random((H0, W0), dtype=F32)).astype(F32)
    a[r < zero] = F32(0.0)
    a[r < neg] = F32(-0.0)
    return a


def _two_level(seed):
    return np.where(np.random.default_rng(seed).random((H0, W0)) < 0.5, F32(0.25), F32(0.75)).astype(F32)


def _build():
    t = []

    def add(name, frame, branch, misaligned=False, exp=False):
        frame = np.ascontiguousarray(frame, dtype=F32)
        t.append(dict(name=name, frame=frame, misaligned=misaligned, exp=exp, branch=dict(zip(QS, branch.split()))))

    # name, frame, branch at q = 0, 1, 99, 100; exp: the two percentiles differ, so 'exprobust' is finite
    add('uniform', _uniform(101), 'fast fast fast fast', exp=True)
    add('signed', F32(3.0) * np.random.default_rng(102).standard_normal((H0, W0), dtype=F32), 'fast fast fast fast', exp=True)
    add('zeros75', _pinned(103, 0.0), 'overflow overflow fast fast', exp=True)
    add('ones75', _pinned(104, 1.0), 'fast fast overflow overflow', exp=True)
    add('const', np.full((H0, W0), 0.25, F32), 'overflow overflow overflow overflow')
    add('two_level', _two_level(105), 'fast fast fast fast')
    add('sample_lies', _sample_lies(106), 'fast miss_low miss_high fast', exp=True)
    # -0.0 and +0.0 are DIFFERENT keys (f2key sorts -0.0 below +0.0) and equal floats: the 5838 keys of -0.0 alone fit the list, so
    # this frame stays on the fast path; pm_zero_heavy has more copies of -0.0 than the list holds and takes the fallback
    add('pm_zero', _pm_zero(107, 0.475, 0.95), 'fast fast fast fast')
    add('pm_zero_heavy', _pm_zero(113, 0.70, 0.95), 'overflow overflow fast fast')
    add('dense_band', _dense_band(114), 'fast overflow miss_high fast', exp=True)
    add('levels9', np.round(F32(8.0) * _uniform(108)) / F32(8.0), 'fast fast fast fast', exp=True)
    add('px1024', _uniform(109, (32, 32)), 'fast fast fast fast')
    add('px1020', _uniform(110, (30, 34)), 'slow slow slow slow')
    add('px_odd', _uniform(111, (33, 47)), 'slow slow slow slow')
    add('px_odd_zeros75', _pinned(112, 0.0, (33, 47)), 'slow slow slow slow')
    add('misaligned', _uniform(101), 'slow slow slow slow', misaligned=True)
    add('misaligned_zeros75', _pinned(103, 0.0), 'slow slow slow slow', misaligned=True)
    return t


_cases = None


def cases():
    """The named frames, built once: list of dict(name, frame [H, W] float32, misaligned, exp, branch {1.0: .., 99.0: ..})."""
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


def classify_case(case, q100):
    return classify(case['frame'], q100, aligned=not case['misaligned'])
