"""CPU checks of the BRISQUE oracle (tests/brisque_ref.py) against facts that do not depend on it, of the model loaders
(libsvm text model + svm-scale range file, .npz), and of the tracker without a model file."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT
import brisque_ref as B


def test_ggd_fit_recovers_beta_of_generalised_gaussian_samples():
    from scipy.stats import gennorm
    from scipy.special import gamma as G
    for beta in (0.8, 1.5, 2.0, 3.0):
        x = gennorm.rvs(beta, size=10 ** 6, random_state=np.random.default_rng(int(beta * 10)))
        k, msq, _ = B.ggd_fit(x)
        assert abs(B.ALPHA[k] - beta) <= 0.05, (beta, B.ALPHA[k])
        assert msq == np.mean(x * x)
        var = G(3.0 / beta) / G(1.0 / beta)
        assert abs(msq - var) <= 0.01 * var, (beta, msq, var)


def test_white_noise_frame_scale1_alpha_from_an_independent_mscn():
    """Gaussian white noise: the MSCN map, built here with scipy.ndimage, is near-Gaussian but lighter-tailed (the 7x7
    window holds the pixel itself, which bounds |M|), so alpha lies a little above 2.  The oracle's grid alpha is the
    continuous root of rho = G(1/a)G(3/a)/G(2/a)^2, found by brentq, to the grid step."""
    from scipy.ndimage import correlate
    from scipy.optimize import brentq
    from scipy.special import gammaln
    rng = np.random.default_rng(4)
    v = (0.5 + 0.08 * rng.standard_normal((480, 640))).astype(np.float32)
    u = np.rint(np.float32(255) * np.clip(v, 0, 1)).astype(np.float64)
    w = B.gaussian_window()
    mu = correlate(u, w, mode='constant')
    m = (u - mu) / (np.sqrt(np.abs(correlate(u * u, w, mode='constant') - mu * mu)) + 1.0)
    rho = np.mean(m * m) / np.mean(np.abs(m)) ** 2
    a = brentq(lambda a: np.exp(gammaln(1 / a) + gammaln(3 / a) - 2 * gammaln(2 / a)) - rho, 0.3, 9.9)
    f = B.features(v)
    assert 2.0 < a < 3.2
    assert abs(f[0] - a) <= 0.0006, (f[0], a)
    assert f[1] == pytest.approx(np.mean(m * m), rel=1e-10)


def test_filter_is_correlation_with_zero_padding():
    from scipy.ndimage import correlate
    rng = np.random.default_rng(1)
    w = B.gaussian_window()
    img = np.rint(255 * rng.random((23, 31)))
    np.testing.assert_allclose(B.filter2_zero(img, w), correlate(img, w, mode='constant', cval=0.0), rtol=1e-13, atol=1e-11)
    # zero padding (not NIQE's replicate): a constant image falls off at the border
    mu = B.filter2_zero(np.full((20, 20), 100.0), w)
    assert mu[10, 10] == pytest.approx(100.0, rel=1e-14) and mu[0, 0] < 60.0


def test_circshift_pairs_wrap_over_the_whole_frame():
    rng = np.random.default_rng(2)
    H, W = 7, 9
    m = rng.standard_normal((H, W))
    for dr, dc in B.SHIFTS:
        want = np.array([[m[y, x] * m[(y - dr) % H, (x - dc) % W] for x in range(W)] for y in range(H)])
        assert np.array_equal(B.pairs(m, (dr, dc)), want)
    # (-1, 1): M(y, x) . M(y + 1, x - 1); the last row pairs with the first
    assert B.pairs(m, (-1, 1))[H - 1, 0] == m[H - 1, 0] * m[0, W - 1]
    # a frame where the wrap matters: a vertical ramp, whose first and last rows differ most
    ramp = np.repeat(np.linspace(0.1, 0.9, 64)[:, None], 48, axis=1) + 0.05 * rng.standard_normal((64, 48))
    mm = B.mscn(B.quantize(ramp.astype(np.float32)))
    p = B.pairs(mm, (1, 0))
    no_wrap = mm[1:] * mm[:-1]
    assert p[1:].sum() == pytest.approx(no_wrap.sum(), rel=1e-12)
    assert p.sum() != pytest.approx(no_wrap.sum(), rel=1e-6)       # row 0 pairs with the last row


def test_odd_resize_has_ceil_shape_and_keeps_a_constant_image():
    for H, W in ((9, 13), (625, 970), (8, 8), (5, 3)):
        out = B.imresize_half(np.full((H, W), 137.0))
        assert out.shape == ((H + 1) // 2, (W + 1) // 2)
        assert np.all(out == 137.0), (H, W)


def _model(rng, nsv=20, lower=-1.0, upper=1.0):
    fmin = -np.abs(rng.standard_normal(36))
    fmax = fmin + np.abs(rng.standard_normal(36)) + 0.1
    fmax[7] = fmin[7]
    return dict(sv=rng.uniform(lower, upper, (nsv, 36)), coef=rng.standard_normal(nsv), gamma=0.05, rho=0.3,
                fmin=fmin, fmax=fmax, lower=lower, upper=upper)


def test_flat_frame_scores_nan():
    m = _model(np.random.default_rng(0))
    f = B.features(np.full((64, 80), 0.4, np.float32))
    assert np.any(np.isnan(f))
    assert math.isnan(B.brisque(np.full((64, 80), 0.4, np.float32), m))


def test_svm_scale_semantics():
    fmin = np.array([0.0, 1.0, 2.0, -3.0] + [0.0] * 32)
    fmax = np.array([4.0, 1.0, 6.0, 5.0] + [1.0] * 32)
    x = np.array([1.0, 7.0, 2.0, 5.0] + [0.5] * 32)
    y = B.svm_scale(x, fmin, fmax, -1.0, 1.0)
    assert y[0] == -1.0 + 2.0 * 1.0 / 4.0
    assert y[1] == 0.0                  # min == max: dropped, whatever the value
    assert y[2] == -1.0 and y[3] == 1.0
    assert np.all(y[4:] == 0.0)
    y = B.svm_scale(x, fmin, fmax, 0.0, 1.0)
    assert y[0] == 0.25 and y[2] == 0.0 and y[3] == 1.0
    assert B.svm_scale(np.full(36, 9.0), np.zeros(36), np.ones(36))[0] == 17.0      # outside the range: extrapolated


def _write_libsvm(path, sv, coef, gamma, rho, svm_type='epsilon_svr', kernel='rbf', extra=()):
    r = lambda x: repr(float(x))                        # shortest round-trip text of an fp64 (libsvm writes %.17g)
    lines = [f'svm_type {svm_type}', f'kernel_type {kernel}', f'gamma {r(gamma)}', 'nr_class 2', f'total_sv {len(coef)}',
             f'rho {r(rho)}', 'probA 0.125', *extra, 'SV']
    for c, row in zip(coef, sv):
        lines.append(f'{r(c)} ' + ' '.join(f'{i + 1}:{r(v)}' for i, v in enumerate(row) if v != 0.0))
    open(path, 'w').write('\n'.join(lines) + '\n')


def _write_range(path, fmin, fmax, lower=-1.0, upper=1.0, skip=(), y=False):
    r = lambda x: repr(float(x))
    lines = (['y', '0 100', '0 100'] if y else []) + ['x', f'{r(lower)} {r(upper)}']
    lines += [f'{i + 1} {r(a)} {r(b)}' for i, (a, b) in enumerate(zip(fmin, fmax)) if i not in skip]
    open(path, 'w').write('\n'.join(lines) + '\n')


def test_libsvm_model_and_range_reproduce_sklearn_svr(tmp_path):
    svm = pytest.importorskip('sklearn.svm')
    from evreal_amd.nriqa import load_brisque_model
    rng = np.random.default_rng(7)
    fmin = rng.uniform(-2, 0, 36)
    fmax = fmin + rng.uniform(0.5, 3, 36)
    fmax[11] = fmin[11]                                        # a feature svm-scale drops
    raw = fmin + (fmax - fmin) * rng.random((150, 36))
    raw[:, 11] = fmin[11]
    scaled = np.array([B.svm_scale(r, fmin, fmax) for r in raw])
    scaled[np.abs(scaled) < 0.15] = 0.0                       # zero entries, left out of the sparse lines
    y = np.sin(scaled[:, 0] * 2) + scaled[:, 1] * scaled[:, 2] + 0.1 * rng.standard_normal(150)
    reg = svm.SVR(kernel='rbf', gamma=0.05, C=3.0, epsilon=0.05).fit(scaled, y)
    _write_libsvm(tmp_path / 'allmodel', reg.support_vectors_, reg.dual_coef_[0], 0.05, float(-reg.intercept_[0]))
    _write_range(tmp_path / 'allrange', fmin, fmax)
    m = load_brisque_model(str(tmp_path / 'allmodel'))
    assert m['sv'].shape == (len(reg.support_), 36) and m['fmin'][11] == m['fmax'][11]
    test = fmin + (fmax - fmin) * rng.random((40, 36))
    test[:, 11] = fmin[11] + 1.0                                # dropped: its value does not matter
    got = np.array([B.score_features(t, m) for t in test])
    want = reg.predict(np.array([B.svm_scale(t, fmin, fmax) for t in test]))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_loader_refusals(tmp_path):
    from evreal_amd.nriqa import load_brisque_model
    rng = np.random.default_rng(3)
    m = _model(rng)
    _write_range(tmp_path / 'allrange', m['fmin'], m['fmax'])

    def refused(match, **kw):
        _write_libsvm(tmp_path / 'bad', m['sv'], m['coef'], 0.05, 0.3, **kw)
        with pytest.raises(ValueError, match=match):
            load_brisque_model(str(tmp_path / 'bad'), str(tmp_path / 'allrange'))

    refused('kernel_type', kernel='linear')
    refused('svm_type', svm_type='c_svc')
    refused('svm_type', svm_type='one_class')
    _write_libsvm(tmp_path / 'ok', m['sv'], m['coef'], 0.05, 0.3, svm_type='nu_svr',
                  extra=('probB 0.5', 'label 1 2', 'nr_sv 3 4'))
    assert load_brisque_model(str(tmp_path / 'ok'), str(tmp_path / 'allrange'))['sv'].shape == (20, 36)
    open(tmp_path / 'idx', 'w').write('svm_type epsilon_svr\nkernel_type rbf\ngamma 0.1\nrho 0\nSV\n0.5 1:0.1 37:0.2\n')
    with pytest.raises(ValueError, match='37'):
        load_brisque_model(str(tmp_path / 'idx'), str(tmp_path / 'allrange'))
    _write_range(tmp_path / 'short', m['fmin'], m['fmax'], skip=(20,))
    with pytest.raises(ValueError, match='21'):
        load_brisque_model(str(tmp_path / 'ok'), str(tmp_path / 'short'))
    _write_range(tmp_path / 'yrange', m['fmin'], m['fmax'], y=True)
    with pytest.raises(ValueError, match='y section'):
        load_brisque_model(str(tmp_path / 'ok'), str(tmp_path / 'yrange'))
    lo, hi = m['fmin'].copy(), m['fmax'].copy()
    lo[3] = hi[3] + 1.0
    _write_range(tmp_path / 'inverted', lo, hi)
    with pytest.raises(ValueError, match='min > max'):
        load_brisque_model(str(tmp_path / 'ok'), str(tmp_path / 'inverted'))
    _write_range(tmp_path / 'interval', m['fmin'], m['fmax'], lower=1.0, upper=-1.0)
    with pytest.raises(ValueError, match='lower'):
        load_brisque_model(str(tmp_path / 'ok'), str(tmp_path / 'interval'))
    open(tmp_path / 'brisque_svm_weights.pth', 'wb').write(b'\0')
    with pytest.raises(ValueError, match='no feature ranges'):
        load_brisque_model(str(tmp_path / 'brisque_svm_weights.pth'))


def test_npz_round_trip_and_convert_command(tmp_path):
    from evreal_amd.nriqa import load_brisque_model, main, save_brisque_model
    rng = np.random.default_rng(9)
    m = _model(rng)
    keys = ('sv', 'coef', 'gamma', 'rho', 'fmin', 'fmax', 'lower', 'upper')
    save_brisque_model(str(tmp_path / 'm.npz'), *(m[k] for k in keys), 'unit test')
    got = load_brisque_model(str(tmp_path / 'm.npz'))
    assert got['source'] == 'unit test'
    for k in keys:
        assert np.array_equal(got[k], m[k]), k
    bad = dict(m, coef=m['coef'].copy())
    bad['coef'][2] = np.inf
    np.savez(str(tmp_path / 'bad.npz'), **bad, source=np.array('x'))
    with pytest.raises(ValueError, match='non-finite'):
        load_brisque_model(str(tmp_path / 'bad.npz'))
    # brisque-convert: libsvm text + range -> the same model as an .npz
    _write_libsvm(tmp_path / 'allmodel', m['sv'], m['coef'], m['gamma'], m['rho'])
    _write_range(tmp_path / 'allrange', m['fmin'], m['fmax'])
    assert main(['brisque-convert', '--model', str(tmp_path / 'allmodel'), '--out', str(tmp_path / 'c.npz')]) == 0
    got = load_brisque_model(str(tmp_path / 'c.npz'))
    for k in keys:
        assert np.array_equal(got[k], m[k]), k
    assert 'allmodel' in got['source'] and 'allrange' in got['source']


def test_model_file_lookup_order(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(em.BRISQUE_MODEL_ENV, raising=False)
    monkeypatch.delenv(em.BRISQUE_RANGE_ENV, raising=False)
    assert em.brisque_model_path() is None
    os.makedirs('pretrained')
    open(os.path.join('pretrained', 'allmodel'), 'w').close()
    assert em.brisque_model_path() is None                    # a libsvm model needs its range file
    open(os.path.join('pretrained', 'allrange'), 'w').close()
    assert em.brisque_model_path() == (os.path.join('pretrained', 'allmodel'), os.path.join('pretrained', 'allrange'))
    open(os.path.join('pretrained', 'brisque_model.npz'), 'w').close()
    assert em.brisque_model_path() == (os.path.join('pretrained', 'brisque_model.npz'), None)
    os.makedirs('mine')
    open(os.path.join('mine', 'model.txt'), 'w').close()
    monkeypatch.setenv(em.BRISQUE_MODEL_ENV, os.path.join('mine', 'model.txt'))
    assert em.brisque_model_path() == (os.path.join('mine', 'model.txt'), os.path.join('mine', 'allrange'))
    monkeypatch.setenv(em.BRISQUE_RANGE_ENV, 'r.txt')
    assert em.brisque_model_path() == (os.path.join('mine', 'model.txt'), 'r.txt')
    open('m.npz', 'w').close()
    monkeypatch.setenv(em.BRISQUE_MODEL_ENV, 'm.npz')
    assert em.brisque_model_path() == ('m.npz', None)
    monkeypatch.setenv(em.BRISQUE_MODEL_ENV, 'missing.npz')   # a path that does not exist: the next in line
    assert em.brisque_model_path() == (os.path.join('pretrained', 'brisque_model.npz'), None)


def test_tracker_without_a_model_file_keeps_brisque_unknown(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(em.BRISQUE_MODEL_ENV, raising=False)
    monkeypatch.setattr(em.EvalMetricsTracker, '_brisque_cache', [False, None])
    assert em.brisque_model_path() is None
    if 'brisque' in em.pyiqa_metric_factory().list_of_metrics:
        pytest.skip("pyiqa is installed: brisque goes to pyiqa without a model file")
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['brisque'], has_reference_frames=False)
    assert t.metrics == [] and 'Unknown metric brisque' in capsys.readouterr().out
    assert t.wants_precomputed() == []


def test_header_and_bindings_declare_the_brisque_entry_points():
    from evreal_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'evreal_hip.h')).read()
    for name in ('evr_brisque_create', 'evr_brisque_destroy', 'evr_brisque_workspace_bytes', 'evr_brisque_score',
                 'evr_brisque_features'):
        assert name + '(' in hdr and name in lib.SYMBOLS, name
    assert 'return 1005;' in open(os.path.join(ROOT, 'evreal_amd', 'csrc', 'common.cpp')).read()
