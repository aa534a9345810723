"""CPU checks of the NIQE oracle (tests/nriqa_ref.py) against facts that do not depend on it, of the model files, and of
the tracker without a model file."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT
import nriqa_ref as R


def test_aggd_fit_recovers_alpha_of_a_generalised_gaussian():
    from scipy.stats import gennorm
    for alpha in (0.8, 2.0, 3.5):
        x = gennorm.rvs(alpha, size=10 ** 6, random_state=np.random.default_rng(int(alpha * 10)))
        k, ls, rs, _ = R.aggd_fit(x)
        assert abs(R.ALPHA[k] - alpha) <= 0.002 + 1e-12 or abs(R.ALPHA[k] - alpha) / alpha < 0.02, (alpha, R.ALPHA[k])
        assert abs(ls / rs - 1.0) < 0.01


def test_aggd_fit_is_exact_on_the_alpha_grid_for_a_two_point_law():
    # x = +-1 with equal weight: r_hat = 1, gamma_hat = 1 -> r_hat_norm = 1 > max r(alpha): the last grid point
    k, ls, rs, _ = R.aggd_fit(np.array([1.0, -1.0] * 50))
    assert k == len(R.ALPHA) - 1 and ls == 1.0 and rs == 1.0


def test_imresize_keeps_a_constant_image_constant():
    img = np.full((192, 288), 137.0)
    out = R.imresize_half(img)
    assert out.shape == (96, 144) and np.all(out == 137.0)


def test_imresize_weights_match_the_hand_written_8_tap_table():
    w, idx = R.contributions(96, 48, 0.5)
    # 0.5 * cubic(0.5 * d), d = 3.5 .. -3.5, cubic with a = -0.5
    want = np.array([-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875])
    assert w.shape == (48, 8)
    assert np.array_equal(w, np.tile(want, (48, 1)))
    assert list(idx[10]) == list(range(17, 25))                  # output 10 reads inputs 2*10-3 .. 2*10+4
    assert list(idx[0]) == [2, 1, 0, 0, 1, 2, 3, 4]              # mirrored (symmetric) at the top border
    assert list(idx[47]) == [91, 92, 93, 94, 95, 95, 94, 93]     # ... and at the bottom


def test_gaussian_window_sums_to_one_and_is_symmetric():
    w = R.gaussian_window()
    assert abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w.T) and np.array_equal(w, w[::-1])


def test_flat_block_gives_nan_features_and_nan_rows_leave_the_covariance():
    f, _ = R.block_features(np.zeros((96, 96)))
    assert np.all(np.isnan(f[1:2])) and np.isnan(f[5]) and f[0] == R.ALPHA[0]
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((50, 36))
    mu0, cov0 = R.nan_stats(rows)
    bad = rows.copy()
    bad = np.vstack([bad, np.full((1, 36), 7.0)])
    bad[-1, 4] = np.nan
    mu, cov = R.nan_stats(bad)
    assert np.array_equal(cov, cov0)
    keep = [c for c in range(36) if c != 4]
    assert np.allclose(mu[4], mu0[4], rtol=0, atol=1e-14)
    assert not np.allclose(mu[keep], mu0[keep])


def test_frame_without_a_whole_block_scores_nan():
    assert math.isnan(R.niqe(np.full((95, 300), 0.5, np.float32), np.zeros(36), np.eye(36)))


def _textures(n, seed, H=288, W=384):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.random((H, W))
        for _ in range(2):
            a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1)) / 3.0
        out.append(np.clip(0.2 + 0.6 * (a - a.min()) / (a.max() - a.min()), 0, 1).astype(np.float32))
    return out


def _blur(v, k=4):
    b = v.astype(np.float64)
    for _ in range(k):
        b = (b + np.roll(b, 1, 0) + np.roll(b, -1, 0) + np.roll(b, 1, 1) + np.roll(b, -1, 1)) / 5.0
    return b.astype(np.float32)


def test_pristine_fit_scores_its_own_frames_low_and_blurred_copies_higher():
    frames = _textures(5, 0)
    mu, cov = R.fit_pristine(frames)
    assert np.all(np.isfinite(mu)) and np.all(np.linalg.eigvalsh(cov) > 0)
    own = [R.niqe(v, mu, cov) for v in frames[:2]]
    blurred = [R.niqe(_blur(v), mu, cov) for v in frames[:2]]
    assert all(np.isfinite(own)) and max(own) < 10.0
    assert min(blurred) > max(own)


def test_pristine_fit_refuses_too_few_rows():
    with pytest.raises(ValueError):
        R.fit_pristine(_textures(1, 1, 96, 192))


def test_model_files_round_trip_and_a_non_spd_model_is_refused(tmp_path):
    from scipy.io import savemat
    from evreal_amd.nriqa import load_niqe_model, save_niqe_model
    rng = np.random.default_rng(5)
    a = rng.standard_normal((36, 36))
    cov = a @ a.T + 36 * np.eye(36)
    cov = (cov + cov.T) / 2
    mu = rng.standard_normal(36)
    savemat(str(tmp_path / 'm.mat'), {'mu_prisparam': mu[None, :], 'cov_prisparam': cov})
    m = load_niqe_model(str(tmp_path / 'm.mat'))
    assert np.array_equal(m['mu'], mu) and np.array_equal(m['cov'], cov)
    save_niqe_model(str(tmp_path / 'm.npz'), mu, cov, 'unit test')
    m = load_niqe_model(str(tmp_path / 'm.npz'))
    assert np.array_equal(m['mu'], mu) and np.array_equal(m['cov'], cov) and m['source'] == 'unit test'
    bad = cov.copy()
    bad[0, 0] = -1.0
    np.savez(str(tmp_path / 'bad.npz'), mu=mu, cov=bad, source=np.array('x'))
    with pytest.raises(ValueError):
        load_niqe_model(str(tmp_path / 'bad.npz'))
    np.savez(str(tmp_path / 'shape.npz'), mu=mu[:35], cov=cov, source=np.array('x'))
    with pytest.raises(ValueError):
        load_niqe_model(str(tmp_path / 'shape.npz'))


def test_tracker_without_a_model_file_keeps_niqe_unknown(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(em.NIQE_MODEL_ENV, raising=False)
    monkeypatch.setattr(em.EvalMetricsTracker, '_niqe_cache', [False, None])
    assert em.niqe_model_path() is None
    if 'niqe' in em.pyiqa_metric_factory().list_of_metrics:
        pytest.skip("pyiqa is installed: niqe goes to pyiqa without a model file")
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['niqe'], has_reference_frames=False)
    assert t.metrics == [] and 'Unknown metric niqe' in capsys.readouterr().out
    assert t.wants_precomputed() == []


def test_model_file_lookup_order(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(em.NIQE_MODEL_ENV, raising=False)
    os.makedirs('pretrained')
    open(os.path.join('pretrained', 'niqe_model.npz'), 'w').close()
    assert em.niqe_model_path() == os.path.join('pretrained', 'niqe_model.npz')
    open(os.path.join('pretrained', 'niqe_modelparameters.mat'), 'w').close()
    assert em.niqe_model_path() == os.path.join('pretrained', 'niqe_modelparameters.mat')
    open('mine.npz', 'w').close()
    monkeypatch.setenv(em.NIQE_MODEL_ENV, 'mine.npz')
    assert em.niqe_model_path() == 'mine.npz'


def test_queued_metric_books_like_the_reference_queue():
    from evreal_amd.eval_metrics import QueuedGpuMetric
    m = QueuedGpuMetric('niqe', no_ref=True)
    m.reset()
    nan = float('nan')
    lines = m.book([], [0, 1, 2], [1.0, 2.0, 3.0])
    assert lines == []
    lines = m.book([0, 1, 2], [3, 4, 5, 6, 7], [nan, 5.0, 6.0, 7.0, 8.0])
    # group 1 = frames 0..3 with one NaN: its 3 finite scores against the last 3 evaluated indices (1, 2, 3)
    assert lines == [(1, 1.0), (2, 2.0), (3, 3.0), (4, 5.0), (5, 6.0), (6, 7.0), (7, 8.0)]
    assert m.book(list(range(8)), [8, 9], [9.0, nan]) == []
    m.finish_queue()                     # the tail leaves as it is (utils/eval_metrics.py:136-140)
    assert m.updated == 2 and m.scores[-2] == 9.0 and math.isnan(m.scores[-1])


def test_header_declares_the_niqe_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'evreal_hip.h')).read()
    for name in ('evr_niqe_create', 'evr_niqe_destroy', 'evr_niqe_workspace_bytes', 'evr_niqe_score', 'evr_niqe_features'):
        assert name + '(' in hdr, name
