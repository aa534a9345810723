"""The frames of tests/pct_paths.py take the selection paths their table says (CPU only: a numpy restatement of the branch decision of
pct_select_fast_kernel, csrc/prepost.hip).  tests/test_gpu_prepost_edges.py relies on this: it can only see a wrong fallback if some
frame reaches it."""
import numpy as np
import pytest

import pct_paths as pp


def test_kernel_constants_are_found():
    S, cap = pp.kernel_constants()
    assert S >= 1024 and cap >= S      # the sample shares the candidate list's space


def test_f2key_is_the_float_order():
    a = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 0.25, 3.5, np.inf], np.float32)
    k = pp.f2key(a)
    assert np.all(k[1:] > k[:-1])      # strictly increasing, -0.0 below +0.0


def test_pct_rank_matches_numpy_indexes():
    for n in (63, 1020, 1024, 1551, 12288, 89960):
        assert pp.pct_rank(n, 0.0) == (0, 1)
        assert pp.pct_rank(n, 100.0) == (n - 1, n - 1)
        for q in (1.0, 99.0):
            vi = np.float32(n - 1) * (np.float32(q) / np.float32(100))
            assert pp.pct_rank(n, q) == (int(np.floor(vi)), int(np.floor(vi)) + 1)


@pytest.mark.parametrize('case', pp.cases(), ids=[c['name'] for c in pp.cases()])
def test_case_takes_the_branch_of_the_table(case):
    assert case['frame'].dtype == np.float32 and case['frame'].ndim == 2
    got = {q: pp.classify_case(case, q) for q in pp.QS}
    assert got == case['branch'], (case['name'], {q: pp.bracket(case['frame'], q) for q in pp.QS})


def test_table_reaches_every_branch():
    robust = {c['branch'][q] for c in pp.cases() for q in (1.0, 99.0)}
    assert robust == set(pp.CLASSES), robust
    standard = {c['branch'][q] for c in pp.cases() for q in (0.0, 100.0)}
    assert {'fast', 'overflow', 'slow'} <= standard, standard
    # fast and fallback work-groups of ONE frame (the two percentiles are the two work-groups of blockIdx.y)
    assert any(sorted((c['branch'][1.0], c['branch'][99.0])) == ['fast', 'overflow'] for c in pp.cases())
    # a slow case with ties at the percentile, and a fast one at the launcher's smallest size
    names = {c['name']: c for c in pp.cases()}
    assert names['px1024']['frame'].size == pp.FAST_MIN_PX and names['px1020']['frame'].size % 4 == 0
    assert names['px_odd']['frame'].size % 4 != 0 and names['px_odd']['frame'].size >= pp.FAST_MIN_PX
    # exprobust cases: the two percentiles differ
    for c in pp.cases():
        if c['exp']:
            e = np.exp(c['frame'])
            assert np.percentile(e, 1) < np.percentile(e, 99), c['name']


def test_a_changed_cap_moves_the_classification():
    """The classifier follows the constants: with a list twice as long zeros75 would fit it, with a short one `uniform` would not."""
    S, cap = pp.kernel_constants()
    names = {c['name']: c for c in pp.cases()}
    assert pp.classify(names['zeros75']['frame'], 1.0, S=S, cap=2 * cap) == 'fast'
    assert pp.classify(names['uniform']['frame'], 1.0, S=S, cap=64) == 'overflow'


def test_misaligned_cases_share_their_frames():
    names = {c['name']: c for c in pp.cases()}
    assert np.array_equal(names['misaligned']['frame'], names['uniform']['frame'])
    assert np.array_equal(names['misaligned_zeros75']['frame'], names['zeros75']['frame'])
