"""BRISQUE on the GPU (evr_brisque_*, evreal_amd/nriqa.py) against the numpy oracle (tests/brisque_ref.py), and the
`-qm brisque` path of the tracker and of evaluate() against the oracle fed through the reference's four-frame queue."""
import ctypes
import math

import numpy as np
import pytest
import torch

import brisque_ref as B
from test_gpu_nriqa import _compare_lines, _model as _niqe_model, _queue_lines, _write_tree

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 13), (180, 240), (260, 346), (480, 640), (625, 970)]
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
KEYS = ('sv', 'coef', 'gamma', 'rho', 'fmin', 'fmax', 'lower', 'upper')


def _frame(H, W, seed, flat=False):
    """Smooth texture + noise, with values beyond [0,1] (the clip) and a flat patch."""
    if flat:
        return np.full((H, W), 0.4, np.float32)
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = 0.5 + 0.3 * np.sin(xx / (5 + seed % 5)) * np.cos(yy / 9.0) + 0.12 * rng.standard_normal((H, W))
    a[:H // 5, :W // 6] = 0.25
    a[H // 2, :] = 1.3
    a[:, W // 3] = -0.2
    return a.astype(np.float32)


def _model():
    """A synthetic SVR whose feature ranges come from real frames, with one feature svm-scale drops (min == max)."""
    feats = np.array([B.features(_frame(H, W, s)) for (H, W), s in zip(SIZES[2:], range(4))])
    fmin, fmax = feats.min(axis=0), feats.max(axis=0)
    fmin, fmax = fmin - 0.1 * (fmax - fmin) - 1e-3, fmax + 0.1 * (fmax - fmin) + 1e-3
    fmax[5] = fmin[5]
    rng = np.random.default_rng(17)
    return dict(sv=rng.uniform(-1, 1, (300, 36)), coef=rng.standard_normal(300), gamma=0.05, rho=-0.7, fmin=fmin,
                fmax=fmax, lower=-1.0, upper=1.0, source='test')


@pytest.fixture(scope='module')
def model():
    return _model()


@pytest.fixture(scope='module')
def brisque(model):
    from evreal_amd.nriqa import BRISQUE
    return BRISQUE(model)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('clip', [True, False])
def test_features_match_the_oracle(brisque, clip):
    for (H, W), seed in zip(SIZES, range(len(SIZES))):
        v = np.stack([_frame(H, W, seed), _frame(H, W, seed + 20)])
        got = brisque.features(_cuda(v), clip=clip).cpu().numpy()
        for g, x in zip(got, v):
            want = B.features(x, clip)
            assert np.array_equal(g[ALPHA_COLS], want[ALPHA_COLS]), (H, W, g[ALPHA_COLS], want[ALPHA_COLS])
            assert H < 100 or np.all(np.isfinite(want)), (H, W)        # (a tiny frame may have an empty AGGD side)
            np.testing.assert_allclose(g, want, rtol=1e-10, atol=1e-14, err_msg=f'{H}x{W} clip={clip}')


def test_scores_match_the_oracle(brisque, model):
    scores = []
    for (H, W), seed in zip(SIZES, range(len(SIZES))):
        v = np.stack([_frame(H, W, seed), _frame(H, W, seed + 30)])
        got = brisque(_cuda(v)).cpu().numpy()
        want = np.array([B.brisque(x, model) for x in v])
        assert H < 100 or np.all(np.isfinite(want))
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9, err_msg=f'{H}x{W}')
        scores += list(want)
    assert np.std(scores) > 1e-3                    # the synthetic model tells the frames apart
    got = brisque(_cuda(_frame(260, 346, 3)[None]), clip=False).cpu().numpy()[0]
    assert got == pytest.approx(B.brisque(_frame(260, 346, 3), model, clip=False), rel=1e-9, abs=1e-9)


def test_bitwise_independent_of_batch_and_position(brisque):
    x = _frame(260, 346, 5)
    alone = brisque(_cuda(x[None])).cpu().numpy()
    alone_f = brisque.features(_cuda(x[None])).cpu().numpy()
    frames = np.stack([_frame(260, 346, 100 + s) for s in range(37)])
    for pos in (0, 17, 36):
        batch = frames.copy()
        batch[pos] = x
        got = brisque(_cuda(batch)).cpu().numpy()
        assert got[pos:pos + 1].view(np.uint64) == alone.view(np.uint64), pos
        f = brisque.features(_cuda(batch)).cpu().numpy()
        assert np.array_equal(f[pos].view(np.uint64), alone_f[0].view(np.uint64)), pos
    full = brisque(_cuda(frames)).cpu().numpy()
    sevens = np.concatenate([brisque(_cuda(frames[i:i + 7])).cpu().numpy() for i in range(0, 37, 7)])
    assert np.array_equal(full.view(np.uint64), sevens.view(np.uint64))


def test_flat_frame_is_nan_and_leaves_its_neighbours_alone(brisque):
    frames = np.stack([_frame(180, 240, s, flat=(s == 3)) for s in range(6)])
    got = brisque(_cuda(frames)).cpu().numpy()
    assert math.isnan(got[3]) and np.all(np.isfinite(np.delete(got, 3)))
    for i in (2, 4):
        alone = brisque(_cuda(frames[i:i + 1])).cpu().numpy()
        assert got[i:i + 1].view(np.uint64) == alone.view(np.uint64)
    assert np.any(np.isnan(brisque.features(_cuda(frames[3:4])).cpu().numpy()))


def test_more_frames_than_one_grid_axis_holds(brisque):
    """Frames ride the grid's y axis, chunked at 65535: 65537 frames against the first and the last 100 computed alone."""
    n = 65537
    x = torch.rand((n, 16, 16), generator=torch.Generator(device='cuda').manual_seed(65537), device='cuda')
    full, full_f = brisque(x), brisque.features(x)
    for sl in (slice(0, 100), slice(n - 100, n)):
        alone, alone_f = brisque(x[sl].contiguous()), brisque.features(x[sl].contiguous())
        assert bool(torch.isfinite(alone).any())                    # the comparison does not pass on NaN alone
        assert torch.equal(alone.view(torch.int64), full[sl].view(torch.int64))
        assert torch.equal(alone_f.view(torch.int64), full_f[sl].view(torch.int64))


def test_workspace_and_argument_refusals(brisque, model):
    from evreal_amd import lib as L
    from evreal_amd.nriqa import BRISQUE, brisque_features
    lib = L.load()
    x = _cuda(np.stack([_frame(64, 80, 0)] * 3))
    out = torch.empty(3, dtype=torch.float64, device='cuda')
    need = int(lib.evr_brisque_workspace_bytes(3, 64, 80))
    assert need > 0 and lib.evr_brisque_workspace_bytes(-1, 64, 80) == 0 and lib.evr_brisque_workspace_bytes(3, 0, 80) == 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    st = L.stream_ptr()
    assert lib.evr_brisque_score(brisque.handle, L.ptr(x), 3, 64, 80, 1, L.ptr(out), L.ptr(ws), need - 1, st) == -3
    assert lib.evr_brisque_score(brisque.handle, L.ptr(x), 3, 64, 80, 1, L.ptr(out), None, need, st) == -3
    assert lib.evr_brisque_score(brisque.handle, L.ptr(x), 3, 64, 80, 1, None, L.ptr(ws), need, st) == -1
    assert lib.evr_brisque_score(brisque.handle, L.ptr(x), 3, 0, 80, 1, L.ptr(out), L.ptr(ws), need, st) == -1
    assert lib.evr_brisque_score(None, L.ptr(x), 3, 64, 80, 1, L.ptr(out), L.ptr(ws), need, st) == -1
    assert lib.evr_brisque_score(brisque.handle, L.ptr(x), 3, 64, 80, 1, L.ptr(out), L.ptr(ws), need, st) == 0
    torch.cuda.synchronize()
    assert np.all(np.isfinite(out.cpu().numpy()))

    def create(**kw):
        m = {k: np.ascontiguousarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v
             for k, v in dict(model, **kw).items()}
        nsv = kw.pop('nsv', len(m['coef']))
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        h = ctypes.c_void_p()
        rc = lib.evr_brisque_create(vp(m['sv']), vp(m['coef']), nsv, m['gamma'], m['rho'], vp(m['fmin']), vp(m['fmax']),
                                    m['lower'], m['upper'], ctypes.byref(h))
        if rc == 0:
            lib.evr_brisque_destroy(h)
        return rc

    assert create() == 0
    assert create(nsv=-1) == -1
    assert create(lower=1.0, upper=1.0) == -1
    assert create(gamma=float('nan')) == -1
    assert create(rho=float('inf')) == -1
    bad = model['fmin'].copy()
    bad[4] = model['fmax'][4] + 1.0
    assert create(fmin=bad) == -1
    sv = model['sv'].copy()
    sv[3, 3] = np.nan
    assert create(sv=sv) == -1
    # a features-only handle (no support vectors) gives features and refuses a score
    f = brisque_features(x)
    assert torch.equal(f.view(torch.int64), brisque.features(x).view(torch.int64))
    fo = BRISQUE(dict(model, sv=np.zeros((0, 36)), coef=np.zeros(0)))
    with pytest.raises(RuntimeError):
        fo(x)
    assert lib.evr_brisque_features(fo.handle, L.ptr(x), 3, 64, 80, 1, None, L.ptr(ws), need, st) == -1


@pytest.fixture()
def model_file(tmp_path, monkeypatch, model):
    from evreal_amd import eval_metrics as em
    from evreal_amd.nriqa import save_brisque_model
    path = str(tmp_path / 'brisque_model.npz')
    save_brisque_model(path, *(model[k] for k in KEYS), 'test')
    monkeypatch.setenv(em.BRISQUE_MODEL_ENV, path)
    monkeypatch.setattr(em.EvalMetricsTracker, '_brisque_cache', [False, None])
    return model


@pytest.fixture()
def niqe_file(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    from evreal_amd.nriqa import save_niqe_model
    m = _niqe_model()
    path = str(tmp_path / 'niqe_model.npz')
    save_niqe_model(path, m['mu'], m['cov'], 'test')
    monkeypatch.setenv(em.NIQE_MODEL_ENV, path)
    monkeypatch.setattr(em.EvalMetricsTracker, '_niqe_cache', [False, None])
    return m


def test_tracker_books_brisque_like_the_reference_queue(tmp_path, model_file, capsys):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['brisque'], has_reference_frames=False)
    assert [m.name for m in t.metrics] == ['brisque'] and t.wants_precomputed() == ['brisque']
    assert 'brisque: model' in capsys.readouterr().out
    frames = [_frame(260, 346, s, flat=(s == 2)) for s in range(11)]
    idx, k = list(range(11)), 0
    for n in (3, 5, 3):
        t.update_batch(idx[k:k + n], _cuda(np.stack(frames[k:k + n])), None, [0.01 * i for i in idx[k:k + n]], None)
        k += n
    t.finalize(idx[-1])
    want = _queue_lines(idx, [B.brisque(f, model_file) for f in frames])
    got = open(tmp_path / 'out' / 'brisque.txt').read()
    assert len(got.splitlines()) == 10 and want.splitlines()[0].startswith('1 ')    # frame 2 is flat: group 1 books 3 scores
    _compare_lines(got, want)


@pytest.mark.parametrize('batch_sequences', [1, 2])
def test_evaluate_without_frames_writes_brisque_next_to_niqe(tmp_path, monkeypatch, model_file, niqe_file, batch_sequences):
    from PIL import Image
    from evreal_amd import eval as ev
    import nriqa_ref as NR
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', str(batch_sequences))
    names = _write_tree(str(tmp_path), False, (81, 82))
    monkeypatch.chdir(tmp_path)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['niqe'])
    out = lambda name: tmp_path / 'outputs' / 'k3k' / 'NR' / name / 'FireNet'
    niqe_alone = {n: open(out(n) / 'niqe.txt').read() for n in names}
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['brisque', 'niqe'])
    for name in names:
        o = out(name)
        assert open(o / 'niqe.txt').read() == niqe_alone[name] and niqe_alone[name]
        idx = [int(l.split()[0]) for l in open(o / 'timestamps.txt').read().splitlines()]
        assert len(idx) >= 8
        bq, nq = [], []
        for i in idx:
            u8 = np.asarray(Image.open(o / 'frame_{:010d}.png'.format(i)), dtype=np.float32) / np.float32(255.0)
            bq.append(B.brisque(u8, model_file))
            nq.append(NR.niqe(u8, niqe_file['mu'], niqe_file['cov']))
        _compare_lines(open(o / 'brisque.txt').read(), _queue_lines(idx, bq))
        _compare_lines(open(o / 'niqe.txt').read(), _queue_lines(idx, nq))


def test_brisque_next_to_mse_leaves_mse_unchanged(tmp_path, monkeypatch, model_file):
    from evreal_amd import eval as ev
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', '2')
    names = _write_tree(str(tmp_path), True, (91, 92))
    monkeypatch.chdir(tmp_path)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse'])
    before = {n: open(tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet' / 'mse.txt').read() for n in names}
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'brisque'])
    for n in names:
        out = tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet'
        assert open(out / 'mse.txt').read() == before[n] and before[n]
        assert open(out / 'brisque.txt').read().strip()
