"""CPU checks of the PIQE oracle (tests/piqe_ref.py) against facts that do not depend on it, of the input set of
tests/test_gpu_piqe.py (every block class occurs; no deciding quantity sits on its threshold), and of the tracker's `piqe`
entry without a GPU."""
import os

import numpy as np
import pytest

from conftest import ROOT
import piqe_ref as P


def _u(H, W, seed):
    rng = np.random.default_rng(seed)
    return np.rint(255 * rng.random((H, W)))


def test_mu_and_sigma_are_a_correlation_with_a_replicate_border():
    from scipy.ndimage import correlate
    w = P.gaussian_window()
    u = _u(32, 48, 1)
    mu, sigma, m = P.mscn_parts(u)
    cmu = correlate(u, w, mode='nearest')
    np.testing.assert_allclose(mu, cmu, rtol=1e-13, atol=1e-11)
    csig = np.sqrt(np.abs(correlate(u * u, w, mode='nearest') - cmu * cmu))
    np.testing.assert_allclose(sigma, csig, rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(m, (u - cmu) / (csig + 1.0), rtol=1e-9, atol=1e-9)
    # replicate (not BRISQUE's zero padding): a constant image stays constant up to the border
    assert P.mscn_parts(np.full((16, 16), 100.0))[0][0, 0] == pytest.approx(100.0, rel=1e-14)


def test_block_variance_is_numpy_var_ddof_1():
    v = (_u(48, 64, 2) / 255).astype(np.float32)
    b = P.blocks(v)
    m = P.mscn_parts(P.quantize(v))[2]
    for by in range(3):
        for bx in range(4):
            blk = m[by * 16:(by + 1) * 16, bx * 16:(bx + 1) * 16]
            assert b['var'][by, bx] == pytest.approx(np.var(blk, ddof=1), rel=1e-13)
    assert np.array_equal((b['flags'] & P.ACTIVE) > 0, b['var'] > 0.1)


def test_segment_deviations_are_sliding_windows_of_the_four_edges():
    from numpy.lib.stride_tricks import sliding_window_view
    rng = np.random.default_rng(3)
    blk = rng.standard_normal((16, 16))
    got = P.segment_stds(blk)
    assert got.shape == (4, 11)
    for e, edge in enumerate((blk[0], blk[15], blk[:, 0], blk[:, 15])):
        np.testing.assert_allclose(got[e], np.std(sliding_window_view(edge, 6), axis=1, ddof=1), rtol=1e-13)


def test_noise_criterion_uses_the_two_central_columns():
    rng = np.random.default_rng(4)
    blk = rng.standard_normal((16, 16))
    var = np.var(blk, ddof=1)
    sg, beta = P.noise_quantities(blk, var)
    r = np.std(blk[:, 7:9], ddof=1) / np.std(np.delete(blk, (7, 8), axis=1), ddof=1)
    assert sg == pytest.approx(np.sqrt(var), rel=1e-15)
    assert beta == pytest.approx(abs(sg - r) / max(sg, r), rel=1e-12)
    # a flat centre in a flat surround: 0/0 -> 0, beta = 1
    assert P.noise_quantities(np.zeros((16, 16)), 1.0) == (1.0, 1.0)


def test_constant_frame_scores_exactly_100():
    for H, W in ((40, 40), (8, 8), (17, 33)):
        b = P.blocks(np.full((H, W), 0.4, np.float32))
        assert not b['flags'].any() and np.all(b['var'] == 0.0)
        assert P.score_blocks(b) == 100.0


def test_block_averaging_raises_the_score_and_flags_noticeable_artefacts():
    rng = np.random.default_rng(5)
    noisy = (P.texture(96, 128, 2) + 0.1 * rng.standard_normal((96, 128))).astype(np.float32)
    blocky = P.block_average(noisy).astype(np.float32)
    assert P.piqe(blocky) > P.piqe(noisy) + 10.0
    f = P.blocks(blocky)['flags']
    assert np.all(f & P.ACTIVE) and np.all(f & P.WHSA)
    assert not np.any(P.blocks(noisy)['flags'] & P.WHSA)


def test_padding_is_edge_replication_at_the_bottom_and_right():
    rng = np.random.default_rng(6)
    v = rng.random((17, 33)).astype(np.float32)
    padded = np.pad(v, ((0, 15), (0, 15)), mode='edge')
    assert padded.shape == (32, 48)
    a, b = P.blocks(v), P.blocks(padded)
    for k in ('var', 'flags', 'contribution'):
        assert a[k].shape == (2, 3) and np.array_equal(a[k], b[k]), k
    assert P.piqe(v) == P.piqe(padded)
    assert P.pad_post(np.zeros((16, 32))).shape == (16, 32)


def test_contribution_and_score_formula():
    b = dict(flags=np.array([[0, P.ACTIVE, P.ACTIVE | P.WHSA], [P.ACTIVE | P.WNC, P.ACTIVE | P.WHSA | P.WNC, 0]], np.uint8),
             contribution=np.array([[0.0, 0.0, 0.7], [0.4, 0.2, 0.0]]))
    assert P.score_blocks(b) == pytest.approx(100.0 * (1.3 + 1.0) / 5.0, rel=1e-15)
    assert list(P.block_class(b['flags']).ravel()) == [0, 1, 2, 3, 4, 0]


@pytest.fixture(scope='module')
def oracle_blocks():
    out = []
    for name, a in P.inputs():
        out.append((name, True, P.blocks(a, True)))
        if name in P.UNCLIPPED:
            out.append((name, False, P.blocks(P.unclipped(a), False)))
    return out


def test_gpu_input_set_covers_every_block_class(oracle_blocks):
    """inactive, active-unflagged, whsa only, wnc only, both"""
    seen = np.zeros(5, int)
    for _, _, b in oracle_blocks:
        seen += np.bincount(P.block_class(b['flags']).ravel(), minlength=5)
    assert np.all(seen > 0), seen
    shapes = {n: a.shape for n, a in P.inputs()}
    assert set(shapes.values()) == {(8, 8), (16, 16), (17, 33), (81, 113), (96, 128), (40, 40), (260, 346)}
    assert any(x.max() > 1.0 and x.min() < 0.0 for x in (P.unclipped(a) for n, a in P.inputs() if n in P.UNCLIPPED))


def test_gpu_input_set_keeps_every_deciding_quantity_off_its_threshold(oracle_blocks):
    """|var - 0.1|, |segstd - 0.1| and |sg - 2 beta| are >= 1e-6 everywhere: the GPU test leaves no block out of its flag
    comparison (its own exclusion rule, a margin below 1e-9, never applies)."""
    worst = min(float(b['margin'].min()) for _, _, b in oracle_blocks)
    print('worst margin', worst)
    assert worst >= 1e-6, worst


def test_tracker_takes_piqe_without_any_file_and_honours_the_switch(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(em.PIQE_ENV, raising=False)
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'a'), quan_eval_metric_names=['piqe'], has_reference_frames=False)
    assert [m.name for m in t.metrics] == ['piqe'] and isinstance(t.metrics[0], em.QueuedGpuMetric) and t.metrics[0].no_ref
    assert t.wants_precomputed() == ['piqe'] and 'Unknown metric' not in capsys.readouterr().out
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'b'), quan_eval_metric_names=['mse', 'piqe'], has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['mse', 'piqe']
    # a user's own registration wins
    monkeypatch.setitem(em._REGISTRY, 'piqe', lambda: em.BaseMetric('piqe', no_ref=True))
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'c'), quan_eval_metric_names=['piqe'], has_reference_frames=False)
    assert not isinstance(t.metrics[0], em.QueuedGpuMetric)
    monkeypatch.delitem(em._REGISTRY, 'piqe')
    monkeypatch.setenv(em.PIQE_ENV, '0')
    if 'piqe' in em.pyiqa_metric_factory().list_of_metrics:
        return                                                  # pyiqa is installed: the name goes there
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'd'), quan_eval_metric_names=['piqe'], has_reference_frames=False)
    assert t.metrics == [] and 'Unknown metric piqe' in capsys.readouterr().out


def test_header_and_bindings_declare_the_piqe_entry_points():
    from evreal_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'evreal_hip.h')).read()
    for name in ('evr_piqe_workspace_bytes', 'evr_piqe_score', 'evr_piqe_blocks'):
        assert name + '(' in hdr and name in lib.SYMBOLS, name


def test_refusals_need_no_gpu():
    from evreal_amd import build, lib
    build.build(verbose=False)
    l = lib.load()
    assert l.evr_piqe_workspace_bytes(2, 260, 346) >= 2 * 17 * 22 * 17
    assert l.evr_piqe_workspace_bytes(0, 260, 346) == 0 and l.evr_piqe_workspace_bytes(2, 0, 346) == 0
    assert l.evr_piqe_score(None, 1, 16, 16, 1, None, None, 0, None) == -1 and b'evr_piqe_score' in l.evr_last_error()
    assert l.evr_piqe_blocks(None, 1, 16, 16, 1, None, None, None, 0, None) == -1 and b'evr_piqe_blocks' in l.evr_last_error()
