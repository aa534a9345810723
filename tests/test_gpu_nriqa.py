"""NIQE on the GPU (evr_niqe_*, evreal_amd/nriqa.py) against the numpy oracle (tests/nriqa_ref.py), and the `-qm niqe` path
of the tracker and of evaluate() against the oracle fed through the reference's four-frame queue."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
import nriqa_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(260, 346), (180, 240), (480, 640), (624, 970)]


def _model(seed=11):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((36, 36)) * 0.05
    cov = a @ a.T + 0.01 * np.eye(36)
    cov = (cov + cov.T) / 2
    mu = np.abs(rng.standard_normal(36)) * 0.5 + 0.2
    return dict(mu=mu, cov=cov, source='test')


def _frame(H, W, seed, flat=False):
    """Smooth texture + noise, with values beyond [0,1] (the clip) and a flat patch."""
    rng = np.random.default_rng([seed, H, W])
    if flat:
        return np.full((H, W), 0.4, np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = 0.5 + 0.3 * np.sin(xx / (7 + seed % 5)) * np.cos(yy / 11.0) + 0.15 * rng.standard_normal((H, W))
    a[:40, :50] = 0.25                                   # a flat corner (a NaN feature row where it fills a block)
    a[H // 2, :] = 1.3
    return a.astype(np.float32)


@pytest.fixture(scope='module')
def niqe():
    from evreal_amd.nriqa import NIQE
    return NIQE(_model())


def test_features_match_the_oracle(niqe):
    for (H, W), seed in zip(SIZES, range(4)):
        v = _frame(H, W, seed)
        feat, sharp = niqe.features(torch.from_numpy(v[None]).cuda())
        feat, sharp = feat[0].cpu().numpy(), sharp[0].cpu().numpy()
        want, wsharp, dists = R.frame_features(v, with_dists=True)
        assert feat.shape == want.shape
        np.testing.assert_allclose(sharp, wsharp, rtol=1e-9, atol=1e-12)
        acols = [0] + [2 + 4 * i for i in range(4)]
        acols = acols + [18 + c for c in acols]
        keep = np.ones(want.shape[0], bool)
        for b in range(want.shape[0]):
            for j, c in enumerate(acols):
                if feat[b, c] != want[b, c]:
                    # one grid step only where the oracle's two squared distances are within 1e-12 relative (a tie up
                    # to the Gamma tables' last bits); that block's other features then follow another grid point
                    d = dists[b][j]
                    kg, kw = int(round((feat[b, c] - 0.2) / 0.001)), int(round((want[b, c] - 0.2) / 0.001))
                    assert abs(kg - kw) == 1 and abs(d[kg] - d[kw]) <= 1e-12 * abs(d[kw]), (H, W, b, c)
                    keep[b] = False
        assert keep.sum() >= len(keep) - 1
        np.testing.assert_allclose(feat[keep], want[keep], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=f'{H}x{W}')


def test_scores_match_the_oracle(niqe):
    m = _model()
    for (H, W), seed in zip(SIZES, range(4)):
        v = np.stack([_frame(H, W, seed), _frame(H, W, seed + 10)])
        got = niqe(torch.from_numpy(v).cuda()).cpu().numpy()
        want = np.array([R.niqe(x, m['mu'], m['cov']) for x in v])
        assert np.all(np.isfinite(want))
        np.testing.assert_allclose(got, want, rtol=1e-7, err_msg=f'{H}x{W}')
    for H, W in ((95, 300), (300, 95), (50, 50)):
        got = niqe(torch.from_numpy(np.stack([_frame(H, W, 0)] * 3)).cuda()).cpu().numpy()
        assert np.all(np.isnan(got)), (H, W)
    # a flat frame: every feature row has a NaN -> NaN
    assert math.isnan(float(niqe(torch.from_numpy(_frame(260, 346, 0, flat=True)[None]).cuda())[0]))


def test_bitwise_independent_of_batch_and_position(niqe):
    frames = torch.from_numpy(np.stack([_frame(260, 346, s) for s in range(64)])).cuda()
    full = niqe(frames).cpu().numpy()
    again = niqe(frames).cpu().numpy()
    assert np.array_equal(full.view(np.uint64), again.view(np.uint64))
    seven = np.concatenate([niqe(frames[i:i + 7]).cpu().numpy() for i in range(0, 64, 7)])
    ones = np.array([float(niqe(frames[i:i + 1])[0]) for i in range(0, 64, 9)])
    assert np.array_equal(seven.view(np.uint64), full.view(np.uint64))
    assert np.array_equal(ones.view(np.uint64), full[::9].view(np.uint64))
    perm = torch.arange(63, -1, -1, device='cuda')
    rev = niqe(frames[perm].contiguous()).cpu().numpy()[::-1]
    assert np.array_equal(np.ascontiguousarray(rev).view(np.uint64), full.view(np.uint64))
    f1, s1 = niqe.features(frames[5:6])
    f64, s64 = niqe.features(frames)
    assert torch.equal(f1[0].view(torch.int64), f64[5].view(torch.int64)) and torch.equal(s1[0], s64[5])


def test_workspace_and_argument_refusals(niqe):
    import ctypes
    from evreal_amd import lib as L
    lib = L.load()
    x = torch.from_numpy(np.stack([_frame(100, 200, s) for s in range(3)])).cuda()
    out = torch.empty(3, dtype=torch.float64, device='cuda')
    need = int(lib.evr_niqe_workspace_bytes(3, 100, 200))
    assert need > 0 and lib.evr_niqe_workspace_bytes(-1, 100, 200) == 0 and lib.evr_niqe_workspace_bytes(3, 0, 200) == 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    st = L.stream_ptr()
    assert lib.evr_niqe_score(niqe.handle, L.ptr(x), 3, 100, 200, 1, L.ptr(out), L.ptr(ws), need - 1, st) == -3
    assert lib.evr_niqe_score(niqe.handle, L.ptr(x), 3, 100, 200, 1, L.ptr(out), None, need, st) == -3
    assert lib.evr_niqe_score(niqe.handle, L.ptr(x), 3, 100, 200, 1, None, L.ptr(ws), need, st) == -1
    assert lib.evr_niqe_score(niqe.handle, L.ptr(x), 3, 0, 200, 1, L.ptr(out), L.ptr(ws), need, st) == -1
    assert lib.evr_niqe_score(None, L.ptr(x), 3, 100, 200, 1, L.ptr(out), L.ptr(ws), need, st) == -1
    assert lib.evr_niqe_score(niqe.handle, L.ptr(x), 3, 100, 200, 1, L.ptr(out), L.ptr(ws), need, st) == 0
    torch.cuda.synchronize()
    assert np.all(np.isfinite(out.cpu().numpy()))

    def create(mu, cov):
        mu, cov = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(cov, dtype=np.float64)
        h = ctypes.c_void_p()
        rc = lib.evr_niqe_create(mu.ctypes.data_as(ctypes.c_void_p), cov.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
        if rc == 0:
            lib.evr_niqe_destroy(h)
        return rc

    m = _model()
    assert create(m['mu'], m['cov']) == 0
    mu = m['mu'].copy()
    mu[7] = np.inf
    assert create(mu, m['cov']) == -1
    cov = m['cov'].copy()
    cov[2, 5] += 1e-6                                    # asymmetric
    assert create(m['mu'], cov) == -1
    shift = 2.0 * np.linalg.eigvalsh(m['cov'])[0]
    assert create(m['mu'], m['cov'] - shift * np.eye(36)) == -1                  # symmetric, its smallest eigenvalue < 0


def test_more_frames_than_one_grid_axis_holds(niqe):
    """Frames ride the grid's y axis, chunked at 65535: 65537 frames of one block against the first and the last 100 computed
    alone.  One block gives 36 finite features and no covariance: every score is NaN, from a score kernel of 65537 groups."""
    n = 65537
    x = torch.rand((n, 96, 96), generator=torch.Generator(device='cuda').manual_seed(65537), device='cuda')
    feat, sharp = niqe.features(x)
    assert feat.shape == (n, 1, 36) and sharp.shape == (n, 1)
    for sl in (slice(0, 100), slice(n - 100, n)):
        f, s = niqe.features(x[sl].contiguous())
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(s).all())
        assert torch.equal(f.view(torch.int64), feat[sl].view(torch.int64))
        assert torch.equal(s.view(torch.int64), sharp[sl].view(torch.int64))
    assert bool(torch.isnan(niqe(x)).all())


def test_score_counts_the_complete_rows_of_more_blocks_than_threads(niqe):
    """17 x 16 = 272 blocks: the score kernel's 256 threads walk the rows in two steps, the second a partial one, and flat
    blocks leave incomplete rows in both.  The score must be the oracle's from the kernel's own features: a wrong count of
    the complete rows scales the covariance by (m' - 1)/(m - 1) and moves the score far beyond 1e-7."""
    v = _frame(17 * 96, 16 * 96, 3)
    # flat beyond the blocks by 20 pixels: the 7x7 window and the resize taps of the half-size scale stay inside
    v[96 - 20:192 + 20, 96 - 20:384 + 20] = 0.3          # blocks 17 .. 19
    v[16 * 96 - 20:, 3 * 96 - 20:5 * 96 + 20] = 0.6      # blocks 259, 260: the second step
    x = torch.from_numpy(v[None]).cuda()
    feat, _ = niqe.features(x)
    rows = feat[0].cpu().numpy()
    incomplete = np.flatnonzero(np.isnan(rows).any(axis=1))
    assert rows.shape == (272, 36) and set(incomplete) >= {17, 18, 19, 259, 260}
    m = _model()
    want = R.score_features(rows, m['mu'], m['cov'])
    assert math.isfinite(want)
    np.testing.assert_allclose(float(niqe(x)[0]), want, rtol=1e-7)


def test_fit_on_gpu_matches_the_oracle_fit():
    from evreal_amd.nriqa import fit_niqe_model
    frames = [_frame(288, 384, s) for s in range(6)]
    got = fit_niqe_model(torch.from_numpy(np.stack(frames)).cuda())
    mu, cov = R.fit_pristine(frames)
    np.testing.assert_allclose(got['mu'], mu, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got['cov'], cov, rtol=1e-7, atol=1e-12)


def _queue_lines(indices, scores, batch=4):
    """utils/eval_metrics.py:44-53,119-147,217-223 for one queued metric: what its file receives."""
    hist, queue, lines, fmt = [], [], [], '{} {:.5f}\n'
    for i, s in zip(indices, scores):
        hist.append(i)
        queue.append(s)
        if len(queue) == batch:
            fin = [x for x in queue if math.isfinite(x)]
            queue = []
            if fin:
                lines += [fmt.format(a, b) for a, b in zip(hist[-len(fin):], fin)]
    if queue:
        lines += [fmt.format(a, b) for a, b in zip(hist[-len(queue):], queue)]
    return ''.join(lines)


@pytest.fixture()
def model_file(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    from evreal_amd.nriqa import save_niqe_model
    m = _model()
    path = str(tmp_path / 'niqe_model.npz')
    save_niqe_model(path, m['mu'], m['cov'], 'test')
    monkeypatch.setenv(em.NIQE_MODEL_ENV, path)
    monkeypatch.setattr(em.EvalMetricsTracker, '_niqe_cache', [False, None])
    return m


def test_tracker_books_niqe_like_the_reference_queue(tmp_path, model_file):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['niqe'], has_reference_frames=False)
    assert [m.name for m in t.metrics] == ['niqe'] and t.wants_precomputed() == ['niqe']
    frames = [_frame(260, 346, s, flat=(s == 2)) for s in range(11)]
    idx, k = list(range(11)), 0
    for n in (3, 5, 3):
        t.update_batch(idx[k:k + n], torch.from_numpy(np.stack(frames[k:k + n])).cuda(), None,
                       [0.01 * i for i in idx[k:k + n]], None)
        k += n
    t.finalize(idx[-1])
    want = _queue_lines(idx, [R.niqe(f, model_file['mu'], model_file['cov']) for f in frames])
    got = open(tmp_path / 'out' / 'niqe.txt').read()
    assert len(got.splitlines()) == 10 and want.splitlines()[0].startswith('1 ')    # frame 2 is flat: group 1 books 3 scores
    _compare_lines(got, want)


def _compare_lines(got, want):
    g, w = got.splitlines(), want.splitlines()
    assert [l.split()[0] for l in g] == [l.split()[0] for l in w]
    for a, b in zip(g, w):
        fa, fb = float(a.split()[1]), float(b.split()[1])
        assert a == b or abs(fa - fb) <= 1.01e-5, (a, b)      # (the last printed digit may round the other way)


def _write_tree(root, with_images, seeds):
    from evreal_amd import synth
    g = load_json('eval_loop.json')
    w = load_npz('firenet_weights.npz')
    for sub in ('eval', 'method', 'dataset'):
        os.makedirs(os.path.join(root, 'config', sub), exist_ok=True)
    cfg = dict(g['cfgs']['k3k'], save_images=True)
    json.dump(cfg, open(os.path.join(root, 'config', 'eval', 'k3k.json'), 'w'))
    ckpt = {'state_dict': {k: torch.from_numpy(w[k]) for k in w.files},
            'config': {'model': {'num_bins': 5, 'skip_type': 'no_skip', 'recurrent_block_type': 'convgru',
                                 'base_num_channels': 16, 'num_residual_blocks': 2,
                                 'recurrent_blocks': {'resblock': [0]}, 'kernel_size': 3,
                                 'final_activation': 'none', 'norm': 'none', 'BN_momentum': 0.01}}}
    torch.save(ckpt, os.path.join(root, 'firenet.pth'))
    json.dump({"model_name": "FireNet", "model_path": os.path.join(root, 'firenet.pth'), "event_tensor_normalization": True,
               "post_process_norm": "robust"}, open(os.path.join(root, 'config', 'method', 'FireNet.json'), 'w'))
    seqs = {}
    for k, seed in enumerate(seeds):
        name = 'seq%d' % k
        synth.write_sequence(os.path.join(root, 'data', 'NR', name), seed, 30000 + 3000 * k, 200000.0, 346, 260, 50.0,
                             with_images=with_images)
        seqs[name] = {}
    json.dump({"root_path": os.path.join(root, 'data', 'NR'), "sequences": seqs},
              open(os.path.join(root, 'config', 'dataset', 'NR.json'), 'w'))
    return list(seqs)


@pytest.mark.parametrize('batch_sequences', [1, 2])
def test_evaluate_without_frames_writes_the_queued_niqe_file(tmp_path, monkeypatch, model_file, batch_sequences):
    from PIL import Image
    from evreal_amd import eval as ev
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', str(batch_sequences))
    names = _write_tree(str(tmp_path), False, (81, 82))
    monkeypatch.chdir(tmp_path)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['niqe'])
    for name in names:
        out = tmp_path / 'outputs' / 'k3k' / 'NR' / name / 'FireNet'
        idx = [int(l.split()[0]) for l in open(out / 'timestamps.txt').read().splitlines()]
        assert len(idx) >= 8
        scores = []
        for i in idx:
            u8 = np.asarray(Image.open(out / 'frame_{:010d}.png'.format(i)), dtype=np.float32)
            scores.append(R.niqe(u8 / np.float32(255.0), model_file['mu'], model_file['cov']))
        _compare_lines(open(out / 'niqe.txt').read(), _queue_lines(idx, scores))


def test_niqe_next_to_mse_leaves_mse_unchanged(tmp_path, monkeypatch, model_file):
    from evreal_amd import eval as ev
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', '2')
    names = _write_tree(str(tmp_path), True, (91, 92))
    monkeypatch.chdir(tmp_path)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse'])
    before = {n: open(tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet' / 'mse.txt').read() for n in names}
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'niqe'])
    for n in names:
        out = tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet'
        assert open(out / 'mse.txt').read() == before[n] and before[n]
        assert open(out / 'niqe.txt').read().strip()
