"""GMSD on the GPU (evr_gmsd, evreal_amd.prepost.GMSD) against the numpy oracle (tests/gmsd_ref.py), and the `-qm gmsd` path of
the tracker and of evaluate() against the oracle fed through the reference's four-frame queue."""
import json

import numpy as np
import pytest
import torch

import gmsd_ref as G
from test_gpu_frmetrics import _pair as _textured_pair
from test_gpu_nriqa import _compare_lines, _queue_lines, _write_tree
from thirdparty_refs import image_pairs

pytestmark = pytest.mark.gpu

TH, TW = 16, 32         # the kernel's tile, in pooled pixels (csrc/gmsd.hip)
# pooled sides one below, at and one above a multiple of the tile in each direction (even and odd source sides), two tiles too
TILE_EDGE = [(2 * TH - 2, 2 * TW + 2), (2 * TH, 2 * TW), (2 * TH + 2, 2 * TW - 2), (2 * TH + 3, 2 * TW + 3), (2 * TH - 1, 2 * TW - 1),
             (4 * TH + 2, 4 * TW - 2), (4 * TH - 2, 4 * TW + 3)]
SMALL = [(2, 4), (4, 4), (5, 7), (33, 65)] + TILE_EDGE
LARGE = [(97, 131), (260, 346), (625, 970)]
FLOOR = 1e-3            # scores at least this far from 0: the square root does not amplify the variance's error beyond 1e-9


def _random_pair(H, W, seed):
    """Uniform noise, as the `noise` pair of image_pairs(): scores far from 0."""
    rng = np.random.default_rng([seed, H, W])
    return rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


@pytest.fixture(scope='module')
def gm():
    from evreal_amd.prepost import GMSD
    return GMSD()


def _check(gm, imgs, refs, clip, floor, tag, worst):
    stats, maps = gm.map(_cuda(np.stack(imgs)), _cuda(np.stack(refs)), clip=clip)
    stats, maps = stats.cpu().numpy(), maps.cpu().numpy()
    for k, (img, ref) in enumerate(zip(imgs, refs)):
        q = G.gms_map(img, ref, clip)
        want, mean = G.gmsd(img, ref, clip), G.mean_gms(img, ref, clip)
        assert maps[k].shape == q.shape
        d_map = np.abs(maps[k] - q).max()
        d_mean = abs(stats[k, 1] - mean)
        d_var = abs(stats[k, 0] ** 2 - want ** 2)
        d_score = abs(stats[k, 0] - want)
        print(f'{tag} clip={clip} frame {k}: score {want:.6f}, map {d_map:.2e}, mean {d_mean:.2e}, variance {d_var:.2e}, '
              f'score {d_score:.2e}')
        for key, d in (('map', d_map), ('mean', d_mean), ('var', d_var), ('score', d_score)):
            worst[key] = max(worst.get(key, 0.0), d)
        assert d_map <= 1e-12, (tag, clip, k, d_map)
        assert d_mean <= 1e-12, (tag, clip, k, d_mean)
        assert d_var <= 1e-12, (tag, clip, k, d_var)
        if floor:
            assert want >= FLOOR, (tag, clip, k, want)
        if want >= FLOOR:
            assert d_score <= 1e-9, (tag, clip, k, d_score)


@pytest.mark.parametrize('clip', [True, False])
def test_map_and_scores_match_the_oracle(gm, clip):
    """Bounds (derived, not tuned): the map 1e-12 absolute -- g <= 170, every operation a correctly rounded fp64 one on
    operands with relative error below 1e-15, q <= 1; the mean GMS 1e-12; the variance |s^2 - s_ref^2| <= 1e-12 -- sums of at
    most 1.5e5 terms of magnitude at most 1; the score additionally |s - s_ref| <= 1e-9 wherever the oracle's score is at
    least 1e-3, which is asserted to hold for every random pair and every pair from 33 x 65 upward.
    Measured on an MI355X over all shapes, clipped and unclipped: map 0 (every pixel bit for bit), mean GMS <= 1.11e-16,
    variance <= 2.08e-17, score <= 5.55e-17."""
    worst = {}
    for (H, W), seed in zip(SMALL, range(len(SMALL))):
        pairs = [_random_pair(H, W, seed), _random_pair(H, W, seed + 100)]
        _check(gm, [p[0] for p in pairs], [p[1] for p in pairs], clip, True, f'{H}x{W}', worst)
    for (H, W), seed in zip(LARGE, range(len(LARGE))):
        pairs = [_textured_pair(H, W, seed)] + ([_textured_pair(H, W, seed + 10)] if H < 625 else [])
        _check(gm, [p[0] for p in pairs], [p[1] for p in pairs], clip, True, f'{H}x{W}', worst)
    for name, img, ref in image_pairs():
        _check(gm, [img, ref], [ref, img], clip, False, name, worst)
    print('largest distances:', {k: f'{v:.2e}' for k, v in worst.items()})


def test_identical_frames_and_swapped_arguments(gm):
    for H, W in ((5, 7), (97, 131), (260, 346)):
        img, ref = _textured_pair(H, W, 4)
        a, b = _cuda(np.stack([img, ref])), _cuda(np.stack([ref, img]))
        same, _ = gm.map(a, a)
        assert np.array_equal(same.cpu().numpy(), [[0.0, 1.0], [0.0, 1.0]]), (H, W)
        s1, m1 = gm.map(a, b)
        s2, m2 = gm.map(b, a)
        assert np.array_equal(_bits(s1), _bits(s2)) and np.array_equal(_bits(m1), _bits(m2)), (H, W)
        assert np.array_equal(_bits(s1)[0], _bits(s1)[1]) and np.array_equal(_bits(m1)[0], _bits(m1)[1]), (H, W)
        assert np.array_equal(_bits(gm(a, b)), _bits(s1)[:, 0]) and np.array_equal(_bits(gm.stats(a, b)), _bits(s1))


def test_one_pooled_pixel_is_nan_and_a_side_of_one_is_refused(gm):
    from evreal_amd import lib as L
    img, ref = _random_pair(3, 3, 1)
    got = gm.stats(_cuda(img[None]), _cuda(ref[None])).cpu().numpy()
    assert np.isnan(got[0, 0]) and abs(got[0, 1] - G.mean_gms(img, ref)) <= 1e-12
    for H, W in ((1, 8), (8, 1)):
        x = _cuda(np.zeros((2, H, W), np.float32))
        with pytest.raises(ValueError, match=f'{H}x{W}'):
            gm(x, x)
    lib = L.load()
    x = _cuda(np.zeros((1, 1, 346), np.float32))
    out = torch.full((1, 2), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    rc = lib.evr_gmsd(L.ptr(x), L.ptr(x), 1, 1, 346, 1, L.ptr(out), None, L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == -1 and b'1 x 346' in lib.evr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), [[7.0, 7.0]])         # nothing was launched


def test_bitwise_independent_of_batch_and_position(gm):
    rng = np.random.default_rng(64)
    imgs, refs = _cuda(rng.random((64, 260, 346), dtype=np.float32)), _cuda(rng.random((64, 260, 346), dtype=np.float32))
    full, full_map = (_bits(t) for t in gm.map(imgs, refs))
    again, again_map = (_bits(t) for t in gm.map(imgs, refs))
    assert np.array_equal(full, again) and np.array_equal(full_map, again_map)
    sevens = [tuple(_bits(t) for t in gm.map(imgs[i:i + 7], refs[i:i + 7])) for i in range(0, 64, 7)]
    assert np.array_equal(np.concatenate([a for a, _ in sevens]), full)
    assert np.array_equal(np.concatenate([b for _, b in sevens]), full_map)
    for i in range(0, 64, 9):
        a, b = (_bits(t) for t in gm.map(imgs[i:i + 1], refs[i:i + 1]))
        assert np.array_equal(a[0], full[i]) and np.array_equal(b[0], full_map[i]), i
    perm = torch.arange(63, -1, -1, device='cuda')
    a, b = (_bits(t) for t in gm.map(imgs[perm].contiguous(), refs[perm].contiguous()))
    assert np.array_equal(a[::-1], full) and np.array_equal(b[::-1], full_map)
    assert np.array_equal(_bits(gm.stats(imgs, refs)), full)        # without the map
    assert abs(np.ascontiguousarray(full[:, 0]).view(np.float64)[0] - G.gmsd(imgs[0].cpu().numpy(), refs[0].cpu().numpy())) <= 1e-9


def test_more_frames_than_one_grid_axis_holds(gm):
    """Frames ride the grid's z axis, chunked at 65535: 65537 pairs against the first and the last 100 computed alone."""
    n = 65537
    rng = np.random.default_rng(65537)
    imgs, refs = _cuda(rng.random((n, 4, 6), dtype=np.float32)), _cuda(rng.random((n, 4, 6), dtype=np.float32))
    full, full_map = (_bits(t) for t in gm.map(imgs, refs))
    for sl in (slice(0, 100), slice(n - 100, n)):
        a, b = (_bits(t) for t in gm.map(imgs[sl].contiguous(), refs[sl].contiguous()))
        assert np.array_equal(a, full[sl]) and np.array_equal(b, full_map[sl])
    k = n - 1
    want = G.gmsd(imgs[k].cpu().numpy(), refs[k].cpu().numpy())
    assert abs(np.ascontiguousarray(full[k]).view(np.float64)[0] - want) <= 1e-9 and want >= FLOOR


def test_existing_metrics_are_untouched(gm):
    from evreal_amd.prepost import FullRefMetrics, Metrics
    pairs = [_textured_pair(260, 346, s) for s in range(5)]
    imgs, refs = _cuda(np.stack([p[0] for p in pairs])), _cuda(np.stack([p[1] for p in pairs]))
    m, fr = Metrics(), FullRefMetrics()
    before, before_fr = _bits(m(imgs, refs)), _bits(fr(imgs, refs))
    keep_i, keep_r = imgs.clone(), refs.clone()
    got = gm(imgs, refs).cpu().numpy()
    assert np.isfinite(got).all() and (got > 0).all()
    assert torch.equal(imgs, keep_i) and torch.equal(refs, keep_r)       # the inputs are read only
    assert np.array_equal(_bits(m(imgs, refs)), before) and np.array_equal(_bits(fr(imgs, refs)), before_fr)


def _feed(t, frames, refs):
    idx, k = list(range(len(frames))), 0
    for n in (3, 5, 3):
        t.update_batch(idx[k:k + n], _cuda(np.stack(frames[k:k + n])), _cuda(np.stack(refs[k:k + n])),
                       [0.01 * i for i in idx[k:k + n]], None)
        k += n
    t.finalize(idx[-1])
    return idx


@pytest.mark.parametrize('hist_eq', ['none', 'global'])
def test_tracker_books_like_the_reference_queue(tmp_path, hist_eq):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    from evreal_amd.prepost import histogram_equalization
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'gmsd'],
                           has_reference_frames=True, hist_eq=hist_eq)
    assert [m.name for m in t.metrics] == ['mse', 'gmsd']
    assert t.wants_precomputed() == (['mse', 'gmsd'] if hist_eq == 'none' else [])
    pairs = [_textured_pair(260, 346, s) for s in range(11)]
    frames, refs = [p[0] for p in pairs], [p[1] for p in pairs]
    idx = _feed(t, frames, refs)
    if hist_eq != 'none':       # the oracle sees the frames the tracker's equalisation hands to the metrics
        eq = lambda a: histogram_equalization(torch.clamp(_cuda(np.stack(a)), 0.0, 1.0).contiguous(), hist_eq).cpu().numpy()
        frames, refs = list(eq(frames)), list(eq(refs))
    got = open(tmp_path / 'out' / 'gmsd.txt').read()
    assert len(got.splitlines()) == 11
    _compare_lines(got, _queue_lines(idx, [G.gmsd(a, b) for a, b in zip(frames, refs)]))
    assert len(open(tmp_path / 'out' / 'mse.txt').read().splitlines()) == 11
    assert 0 < t.get_mean_scores()['gmsd'] < 1


def test_evaluate_writes_the_same_files_one_sequence_at_a_time_and_batched(tmp_path, monkeypatch):
    from evreal_amd import eval as ev
    from evreal_amd.eval_metrics import EvalMetricsTracker
    names = _write_tree(str(tmp_path), True, (91, 92))
    monkeypatch.chdir(tmp_path)
    # (with the tree's 3 ms tolerance only two windows of a sequence end near a frame: every window is scored here, so that the
    # queue releases full groups as well as a tail)
    cfg_path = tmp_path / 'config' / 'eval' / 'k3k.json'
    cfg_path.write_text(json.dumps(dict(json.loads(cfg_path.read_text()), ts_tol_ms=1e6)))
    out = lambda n: tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet'
    read = lambda n, files: {f: open(out(n) / (f + '.txt')).read() for f in files}
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', '2')
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim'])
    plain = {n: read(n, ('mse', 'ssim')) for n in names}

    seen = {}
    real = EvalMetricsTracker.update_batch

    def spy(self, indices, imgs, refs, img_ts, ref_ts, scores=None, u8=None):
        rec = seen.setdefault(self.output_dir, [])
        rec += [(i, a, b) for i, a, b in zip(indices, imgs.detach().cpu().numpy().copy(), refs.detach().cpu().numpy().copy())]
        return real(self, indices, imgs, refs, img_ts, ref_ts, scores=scores, u8=u8)

    runs = {}
    for S in (1, 2):
        monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', str(S))
        seen.clear()
        monkeypatch.setattr(EvalMetricsTracker, 'update_batch', spy)
        ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim', 'gmsd'])
        monkeypatch.setattr(EvalMetricsTracker, 'update_batch', real)
        runs[S] = {n: read(n, ('mse', 'ssim', 'gmsd')) for n in names}
    assert runs[1] == runs[2]
    for n in names:
        assert runs[2][n]['mse'] == plain[n]['mse'] and runs[2][n]['ssim'] == plain[n]['ssim'] and plain[n]['mse']
        rec = [v for k, v in seen.items() if k.replace('\\', '/').endswith(f'/{n}/FireNet')][0]
        evaluated = [int(l.split()[0]) for l in runs[2][n]['mse'].splitlines()]
        rec = [r for r in rec if r[0] in set(evaluated)]
        assert [r[0] for r in rec] == evaluated and len(evaluated) >= 8
        assert len(runs[2][n]['gmsd'].splitlines()) == len(evaluated)
        _compare_lines(runs[2][n]['gmsd'], _queue_lines(evaluated, [G.gmsd(a, b) for _, a, b in rec]))
