"""PSNR / MS-SSIM on the GPU (evr_fr_metrics, evreal_amd.prepost.FullRefMetrics) against the numpy oracle
(tests/frmetrics_ref.py), and the `-qm psnr ms_ssim` path of the tracker and of evaluate() against the oracle fed through
the reference's four-frame queue."""
import json

import numpy as np
import pytest
import torch

import frmetrics_ref as FR
from test_gpu_brisque import _frame
from test_gpu_nriqa import _compare_lines, _queue_lines, _write_tree
from thirdparty_refs import image_pairs

pytestmark = pytest.mark.gpu

SIZES = [(161, 161), (180, 240), (260, 346), (480, 640), (625, 970)]


def _pair(H, W, seed):
    """A reference built like the BRISQUE test frames (values beyond [0, 1], a flat patch) and an image 6 % of noise away."""
    ref = _frame(H, W, seed)
    rng = np.random.default_rng([seed, H, W, 7])
    return (ref + np.float32(0.06) * rng.standard_normal((H, W)).astype(np.float32)).astype(np.float32), ref


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def fr():
    from evreal_amd.prepost import FullRefMetrics
    return FullRefMetrics()


def _check(fr, imgs, refs, clip, floor, tag, worst):
    scores, scales = fr.per_scale(_cuda(np.stack(imgs)), _cuda(np.stack(refs)), clip=clip)
    scores, scales = scores.cpu().numpy(), scales.cpu().numpy()
    for k, (img, ref) in enumerate(zip(imgs, refs)):
        want, per = FR.ms_ssim(img, ref, clip)
        row = FR.scales_row(per)
        assert np.abs(row).min() >= floor, (tag, row)         # away from 0: the clamp cannot flip
        d_scale = np.abs(scales[k] - row).max()
        d_comb = abs(scores[k, 1] - FR.combine(scales[k])) / FR.combine(scales[k])
        d_psnr = abs(scores[k, 0] - FR.psnr(img, ref, clip))
        d_score = abs(scores[k, 1] - want)
        print(f'{tag} clip={clip} frame {k}: per-scale {d_scale:.2e}, score vs own scales (rel) {d_comb:.2e}, '
              f'score vs oracle {d_score:.2e}, psnr {d_psnr:.2e} dB')
        for key, d in (('scale', d_scale), ('comb', d_comb), ('psnr', d_psnr), ('score', d_score)):
            worst[key] = max(worst.get(key, 0.0), d)
        assert d_scale <= 1e-9, (tag, clip, k, d_scale)
        assert d_comb <= 1e-13, (tag, clip, k, d_comb)
        assert d_psnr <= 1e-9, (tag, clip, k, d_psnr)


@pytest.mark.parametrize('clip', [True, False])
def test_kernels_match_the_oracle(fr, clip):
    """Bounds (derived, not tuned): per-scale CS_l / S_l 1e-9 absolute -- each moment is two 11-term fp64 sums of values of
    at most 1 (1.3 unclipped), error <= 2.4e-15, variances <= 7e-15, divided by denominators of at least C2 = 9e-4 and
    C1 = 1e-4: <= 2e-10 (6e-10 unclipped) on the maps and their means; the score against the product formula on the
    kernel's own ten outputs 1e-13 relative; PSNR 1e-9 dB (fp64 sums of <= 6.1e5 terms: <= 3e-10 dB).
    Measured on an MI355X over all sizes, clipped and unclipped: per-scale <= 4.5e-16, score against the product formula
    <= 2.3e-16 relative, score against the oracle <= 2.3e-16, PSNR <= 7.2e-15 dB."""
    worst = {}
    for (H, W), seed in zip(SIZES, range(len(SIZES))):
        pairs = [_pair(H, W, seed), _pair(H, W, seed + 10)]
        _check(fr, [p[0] for p in pairs], [p[1] for p in pairs], clip, 0.8, f'{H}x{W}', worst)
    for name, img, ref in image_pairs():
        if min(img.shape) >= 161:
            _check(fr, [img, ref], [ref, img], clip, 1e-3, name, worst)
    print('largest distances:', {k: f'{v:.2e}' for k, v in worst.items()})


def test_psnr_alone_takes_any_size_and_ms_ssim_refuses_small_frames(fr):
    from evreal_amd import lib as L
    for H, W in ((1, 1), (7, 300), (96, 128), (160, 346)):
        img, ref = _pair(H, W, 3)
        got = fr(_cuda(img[None]), _cuda(ref[None]), ms_ssim=False).cpu().numpy()
        assert abs(got[0, 0] - FR.psnr(img, ref)) <= 1e-9 and got[0, 1] == 0.0, (H, W)
        with pytest.raises(ValueError, match='161'):
            fr(_cuda(img[None]), _cuda(ref[None]))
    lib = L.load()
    x = _cuda(np.zeros((1, 96, 128), np.float32))
    out = torch.empty((1, 2), dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    rc = lib.evr_fr_metrics(L.ptr(x), L.ptr(x), 1, 96, 128, 2, 1, L.ptr(out), None, L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == -1 and b'161' in lib.evr_last_error()
    ident = fr(_cuda(_pair(260, 346, 1)[1][None]), _cuda(_pair(260, 346, 1)[1][None])).cpu().numpy()
    assert ident[0, 1] == 1.0 and abs(ident[0, 0] - 80.0) <= 1e-12


def test_bitwise_independent_of_batch_and_position(fr):
    pairs = [_pair(260, 346, s) for s in range(64)]
    imgs, refs = _cuda(np.stack([p[0] for p in pairs])), _cuda(np.stack([p[1] for p in pairs]))
    bits = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)
    full, full_sc = fr.per_scale(imgs, refs)
    full, full_sc = bits(full), bits(full_sc)
    again, again_sc = fr.per_scale(imgs, refs)
    assert np.array_equal(full, bits(again)) and np.array_equal(full_sc, bits(again_sc))
    sevens = [fr.per_scale(imgs[i:i + 7], refs[i:i + 7]) for i in range(0, 64, 7)]
    sevens = [(bits(a), bits(b)) for a, b in sevens]
    assert np.array_equal(np.concatenate([a for a, _ in sevens]), full)
    assert np.array_equal(np.concatenate([b for _, b in sevens]), full_sc)
    for i in range(0, 64, 9):
        a, b = fr.per_scale(imgs[i:i + 1], refs[i:i + 1])
        assert np.array_equal(bits(a)[0], full[i]) and np.array_equal(bits(b)[0], full_sc[i]), i
    perm = torch.arange(63, -1, -1, device='cuda')
    a, b = fr.per_scale(imgs[perm].contiguous(), refs[perm].contiguous())
    assert np.array_equal(bits(a)[::-1], full) and np.array_equal(bits(b)[::-1], full_sc)
    only = bits(fr(imgs, refs, psnr=False))
    assert np.array_equal(only[:, 1], full[:, 1]) and not only[:, 0].any()


def test_more_frames_than_one_grid_axis_holds(fr):
    """Frames ride the grid's z axis, chunked at 65535: 65537 pairs of 2 x 2 with PSNR alone (65537 frames of the 161 x 161
    MS-SSIM needs do not fit; the chunk loop is the same code) against the first and the last 100 computed alone, bit for bit,
    and the last pair against the oracle within the 1e-9 dB of test_kernels_match_the_oracle."""
    n = 65537
    g = torch.Generator(device='cuda').manual_seed(65537)
    imgs = torch.rand((n, 2, 2), device='cuda', generator=g)
    refs = torch.rand((n, 2, 2), device='cuda', generator=g)
    bits = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)
    full = fr(imgs, refs, ms_ssim=False)
    for sl in (slice(0, 100), slice(n - 100, n)):
        assert np.array_equal(bits(fr(imgs[sl].contiguous(), refs[sl].contiguous(), ms_ssim=False)), bits(full[sl]))
    k = n - 1
    got, want = full[k].cpu().numpy(), FR.psnr(imgs[k].cpu().numpy(), refs[k].cpu().numpy())
    print(f'last pair: psnr {got[0]!r} vs {want!r}')
    assert abs(got[0] - want) <= 1e-9 and got[1] == 0.0


def test_existing_metrics_are_untouched(fr):
    from evreal_amd.prepost import Metrics
    pairs = [_pair(260, 346, s) for s in range(5)]
    imgs, refs = _cuda(np.stack([p[0] for p in pairs])), _cuda(np.stack([p[1] for p in pairs]))
    m = Metrics()
    before = m(imgs, refs).cpu().numpy()
    new = fr(imgs, refs).cpu().numpy()
    after = m(imgs, refs).cpu().numpy()
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    # the squared error is summed over the same tiles in the same order as evr_metrics: the same mse, to the last bit
    want = 10.0 * np.log10(1.0 / (before[:, 0] + 1e-8))
    np.testing.assert_allclose(new[:, 0], want, rtol=0, atol=1e-12)


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
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'psnr', 'ms_ssim'],
                           has_reference_frames=True, hist_eq=hist_eq)
    assert [m.name for m in t.metrics] == ['mse', 'psnr', 'ms_ssim']
    assert t.wants_precomputed() == (['mse', 'psnr', 'ms_ssim'] if hist_eq == 'none' else [])
    pairs = [_pair(260, 346, s) for s in range(11)]
    frames, refs = [p[0] for p in pairs], [p[1] for p in pairs]
    idx = _feed(t, frames, refs)
    if hist_eq != 'none':       # the oracle sees the frames the tracker's equalisation hands to the metrics
        eq = lambda a: histogram_equalization(torch.clamp(_cuda(np.stack(a)), 0.0, 1.0).contiguous(), hist_eq).cpu().numpy()
        frames, refs = list(eq(frames)), list(eq(refs))
    for name, fn in (('psnr', FR.psnr), ('ms_ssim', lambda a, b: FR.ms_ssim(a, b)[0])):
        got = open(tmp_path / 'out' / (name + '.txt')).read()
        assert len(got.splitlines()) == 11
        _compare_lines(got, _queue_lines(idx, [fn(a, b) for a, b in zip(frames, refs)]))
    assert len(open(tmp_path / 'out' / 'mse.txt').read().splitlines()) == 11
    means = t.get_mean_scores()
    assert 0.9 < means['ms_ssim'] <= 1.0 or hist_eq != 'none'
    assert means['psnr'] > 0


def test_too_small_frames_leave_ms_ssim_empty(tmp_path, capsys):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'psnr', 'ms_ssim'],
                           has_reference_frames=True)
    pairs = [_pair(96, 128, s) for s in range(11)]
    idx = _feed(t, [p[0] for p in pairs], [p[1] for p in pairs])
    out = capsys.readouterr().out
    assert out.count('Exception in metric ms_ssim: ') == 1 and '161' in out
    assert open(tmp_path / 'out' / 'ms_ssim.txt').read() == ''
    means = t.get_mean_scores()
    assert means['ms_ssim'] == -1 and means['psnr'] > 0 and means['mse'] > 0
    _compare_lines(open(tmp_path / 'out' / 'psnr.txt').read(), _queue_lines(idx, [FR.psnr(a, b) for a, b in pairs]))
    assert len(open(tmp_path / 'out' / 'mse.txt').read().splitlines()) == 11


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
        ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim', 'psnr', 'ms_ssim'])
        monkeypatch.setattr(EvalMetricsTracker, 'update_batch', real)
        runs[S] = {n: read(n, ('mse', 'ssim', 'psnr', 'ms_ssim')) for n in names}
    assert runs[1] == runs[2]
    for n in names:
        assert runs[2][n]['mse'] == plain[n]['mse'] and runs[2][n]['ssim'] == plain[n]['ssim'] and plain[n]['mse']
        rec = [v for k, v in seen.items() if k.replace('\\', '/').endswith(f'/{n}/FireNet')][0]
        evaluated = [int(l.split()[0]) for l in runs[2][n]['mse'].splitlines()]
        rec = [r for r in rec if r[0] in set(evaluated)]
        assert [r[0] for r in rec] == evaluated and len(evaluated) >= 8
        _compare_lines(runs[2][n]['psnr'], _queue_lines(evaluated, [FR.psnr(a, b) for _, a, b in rec]))
        _compare_lines(runs[2][n]['ms_ssim'], _queue_lines(evaluated, [FR.ms_ssim(a, b)[0] for _, a, b in rec]))
