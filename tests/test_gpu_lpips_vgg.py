"""LPIPS-VGG on the GPU (evr_lpips_vgg_*, evreal_amd.lpips.LPIPSVGG) against the torch-CPU restatement (tests/lpips_vgg_ref.py) with
deterministic synthetic weights, and the `-qm lpips-vgg` path of the tracker and of evaluate().  Parity with pyiqa itself is
unpinned (tests/test_lpips_vgg_pins.py)."""
import json
import os

import numpy as np
import pytest
import torch

import lpips_vgg_ref as R
from test_gpu_nriqa import _compare_lines, _queue_lines, _write_tree
from vgg_metric_common import _bound, _cuda, _feed, _frames, BATCHES, run_child, write_weights_file

pytestmark = pytest.mark.gpu

# 16x16: every pool ends at one pixel; 37x53: a pool drops a row or a column on three of the four levels; 64x80: several tiles,
# and cout = 64 and cout >= 128 both reach their kernels
SHAPES = [(16, 16), (37, 53), (64, 80)]
_REF = {}


@pytest.fixture(scope='module')
def sd():
    from evreal_amd import weights
    return weights.synth_lpips_vgg_state_dict(seed=3)


def _reference(sd, H, W):
    """(img, ref, (total64, layers64), (total32, layers32)) of the test frames at H x W: computed once per shape, never modified."""
    if (H, W) not in _REF:
        img, ref = R.frame_pairs(H, W)
        _REF[(H, W)] = (img, ref, R.lpips_vgg(sd, img, ref, torch.float64), R.lpips_vgg(sd, img, ref, torch.float32))
    return _REF[(H, W)]


def _assert_within(got_total, got_layers, ref, tag, scale=1.0):
    _, _, (t64, l64), (t32, l32) = ref
    worst = 0.0
    for name, got, w64, w32 in (('total', got_total, t64, t32), ('layers', got_layers, l64, l32)):
        ratio = np.abs(got - w64) / _bound(w64, w32, scale)
        print(f'{tag} {name}: error / bound (worst {ratio.max():.3f})\n{ratio}')
        worst = max(worst, float(ratio.max()))
    for name, got, w64, w32 in (('total', got_total, t64, t32), ('layers', got_layers, l64, l32)):
        assert (np.abs(got - w64) <= _bound(w64, w32, scale)).all(), (tag, name, got, w64)
    return worst


@pytest.mark.parametrize('shape', SHAPES)
def test_totals_and_layers_vs_oracle(sd, shape):
    """Pair 0 is identical (exactly 0), pair 3 is zeros against ones (conv1_1's padding term).  For the totals and each of the five
    layers |got - want64| <= max(2e-4 |want64| + 1e-7, 8 |want32 - want64|).
    Worst measured error / bound on an MI355X (default h3 arithmetic), all three shapes: totals below 0.0005, layers 0.002."""
    from evreal_amd.lpips import LPIPSVGG
    H, W = shape
    ref = _reference(sd, H, W)
    m = LPIPSVGG(sd)
    img, rf = _cuda(ref[0]), _cuda(ref[1])
    total = m(img, rf).cpu().numpy()
    layers = m.layers(img, rf).cpu().numpy()
    assert total.shape == (4,) and layers.shape == (4, 5)
    assert total[0] == 0.0 and np.array_equal(layers[0], np.zeros(5))
    _assert_within(total, layers, ref, f'{H}x{W}')
    assert m.saturation() == 0
    assert m.flops() > 0


def test_passes_determinism_and_a_handle_that_changes_shape(sd):
    """n = 5 with max_pairs = 2 (passes of 2, 2 and 1 pairs) against one pass, at the bound test_lpips_handle_serves_changing_pair_counts
    uses between pair counts (split-K may reorder sums); the same call twice is equal bit for bit; a changing n and a changing frame
    size on one handle give exactly what a fresh handle gives."""
    from evreal_amd.lpips import LPIPSVGG
    H, W = 37, 53
    rng = np.random.default_rng(5)
    ref = rng.random((5, H, W), dtype=np.float32)
    img = np.clip(ref + 0.1 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    d_img, d_ref = _cuda(img), _cuda(ref)
    one = LPIPSVGG(sd)
    want, want_l = one(d_img, d_ref).cpu().numpy(), one.layers(d_img, d_ref).cpu().numpy()
    np.testing.assert_allclose(want[:2], R.lpips_vgg(sd, img[:2], ref[:2])[0], rtol=2e-4, atol=1e-7)
    chunked = LPIPSVGG(sd, max_pairs=2)
    np.testing.assert_allclose(chunked(d_img, d_ref).cpu().numpy(), want, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(chunked.layers(d_img, d_ref).cpu().numpy(), want_l, rtol=1e-6, atol=1e-9)
    assert np.array_equal(one(d_img, d_ref).cpu().numpy(), want)
    assert np.array_equal(chunked(d_img, d_ref).cpu().numpy(), chunked(d_img, d_ref).cpu().numpy())
    fresh = {}
    for n in (3, 5, 1, 2, 5, 3):
        o = int(rng.integers(0, 5 - n + 1))
        if n not in fresh:
            fresh[n] = LPIPSVGG(sd)
        got = one(d_img[o:o + n], d_ref[o:o + n]).cpu().numpy()
        np.testing.assert_array_equal(got, fresh[n](d_img[o:o + n], d_ref[o:o + n]).cpu().numpy(), err_msg=f'n={n}')
        np.testing.assert_allclose(got, want[o:o + n], rtol=1e-6, atol=1e-9, err_msg=f'n={n}')
    small_i, small_r = d_img[:2, :16, :24].contiguous(), d_ref[:2, :16, :24].contiguous()
    a = one(d_img[:2], d_ref[:2]).cpu().numpy()
    b = one(small_i, small_r).cpu().numpy()
    c = one(d_img[:2], d_ref[:2]).cpu().numpy()
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(b, LPIPSVGG(sd)(small_i, small_r).cpu().numpy())
    np.testing.assert_allclose(b, R.lpips_vgg(sd, img[:2, :16, :24], ref[:2, :16, :24])[0], rtol=2e-4, atol=1e-7)
    assert one.saturation() == 0 and chunked.saturation() == 0


def test_a_side_below_16_is_refused(sd):
    from evreal_amd import lib as L
    from evreal_amd.lpips import LPIPSVGG
    m = LPIPSVGG(sd)
    x = _cuda(np.zeros((2, 15, 40), np.float32))
    with pytest.raises(ValueError, match='15x40'):
        m(x, x)
    out = torch.full((2,), 7.0, dtype=torch.float64, device='cuda')      # the C entry point refuses it too, before any launch
    rc = m.lib.evr_lpips_vgg_forward(m.handle, L.ptr(x), L.ptr(x), 2, 15, 40, 1, L.ptr(out), None, L.stream_ptr())
    assert rc == -1 and b'too small' in m.lib.evr_last_error()
    rc = m.lib.evr_lpips_vgg_forward(m.handle, L.ptr(x), L.ptr(x), 1, 2048, 2048, 1, L.ptr(out), None, L.stream_ptr())      # H * W = 2^22
    assert rc == -1 and b'too large' in m.lib.evr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), [7.0, 7.0])


@pytest.mark.parametrize('clip', [True, False])
def test_clip_of_the_input(sd, clip):
    """Frames that leave [0,1]: with clip the kernels score clip(x, 0, 1), without it x as it is -- against the oracle, which never
    clips, on the input prepared accordingly (the gate of test_totals_and_layers_vs_oracle)."""
    from evreal_amd.lpips import LPIPSVGG
    H, W = 37, 53
    _, ref = R.frame_pairs(H, W, n=2)
    rng = np.random.default_rng(23)
    img = (ref + 0.4 * rng.standard_normal(ref.shape)).astype(np.float32)
    assert (img < 0).mean() > 0.02 and (img > 1).mean() > 0.02
    seen = np.clip(img, 0, 1) if clip else img
    want = (img, ref, R.lpips_vgg(sd, seen, ref, torch.float64), R.lpips_vgg(sd, seen, ref, torch.float32))
    other = R.lpips_vgg(sd, img if clip else np.clip(img, 0, 1), ref, torch.float64)[0]
    # the two readings are more than two bounds apart on every pair: a kernel that took the other one cannot pass
    assert (np.abs(other - want[2][0]) > 2 * _bound(want[2][0], want[3][0])).all()
    m = LPIPSVGG(sd)
    total = m(_cuda(img), _cuda(ref), clip=clip).cpu().numpy()
    layers = m.layers(_cuda(img), _cuda(ref), clip=clip).cpu().numpy()
    _assert_within(total, layers, want, f'clip={clip}')


_CHILD = r'''
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np, torch
import lpips_vgg_ref as R
from evreal_amd import weights
from evreal_amd.lpips import LPIPSVGG
sd = weights.synth_lpips_vgg_state_dict(seed=3)
img, ref = R.frame_pairs(37, 53, n=2)
m = LPIPSVGG(sd)
a, b = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
print('RESULT ' + json.dumps({'total': m(a, b).cpu().numpy().tolist(), 'layers': m.layers(a, b).cpu().numpy().tolist(),
                              'sat': m.saturation()}))
'''


@pytest.mark.parametrize('mode,scale', [('fp32', 1.0), ('mx', 10.0), ('mx6', 10.0)])
def test_arithmetic_modes(sd, mode, scale):
    """One fresh child process per mode (the library reads EVR_ARITH once), 37 x 53 with 3 pairs.  fp32 takes the bound of
    test_totals_and_layers_vs_oracle; mx and mx6 (which LPIPS runs as mx) ten times that bound: the ratio between this project's
    image gates for those modes and for h3 (1e-4 against 1e-5).
    Worst measured error / bound on an MI355X: fp32 totals below 0.0005, layers 0.002; mx and mx6 (of their ten-fold bound)
    totals 0.001, layers 0.007."""
    got = run_child(_CHILD, mode)
    img, ref = R.frame_pairs(37, 53, n=2)
    ref4 = (img, ref, R.lpips_vgg(sd, img, ref, torch.float64), R.lpips_vgg(sd, img, ref, torch.float32))
    total, layers = np.array(got['total']), np.array(got['layers'])
    assert total[0] == 0.0
    _assert_within(total, layers, ref4, mode, scale)
    assert got['sat'] == 0


@pytest.fixture()
def weights_file(tmp_path, monkeypatch, sd):
    from evreal_amd import eval_metrics as em
    return write_weights_file(tmp_path, monkeypatch, sd, 'lpips_vgg.pth', em.LPIPS_VGG_WEIGHTS_ENV, '_lpips_vgg_cache')


def test_tracker_books_like_the_reference_queue(tmp_path, weights_file, sd):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    from evreal_amd.lpips import LPIPSVGG
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'lpips-vgg'], has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['mse', 'lpips-vgg'] and t.wants_precomputed() == ['mse', 'lpips-vgg']
    frames, refs = _frames(32, 40, 10)
    idx = _feed(t, frames, refs)
    m, scores, k = LPIPSVGG(sd), [], 0
    for n in BATCHES:      # the handle's own scores, in the tracker's batches
        scores += m(_cuda(np.stack(frames[k:k + n])), _cuda(np.stack(refs[k:k + n])), clip=True).cpu().numpy().tolist()
        k += n
    got = open(tmp_path / 'out' / 'lpips-vgg.txt').read()
    assert len(got.splitlines()) == 10 and got == _queue_lines(idx, scores)
    assert min(scores) > 1e-3
    assert abs(t.get_mean_scores()['lpips-vgg'] - np.mean(scores)) <= 1e-12
    plain = EvalMetricsTracker(output_dir=str(tmp_path / 'plain'), quan_eval_metric_names=['mse'], has_reference_frames=True)
    _feed(plain, frames, refs)
    with open(tmp_path / 'out' / 'mse.txt', 'rb') as a, open(tmp_path / 'plain' / 'mse.txt', 'rb') as b:
        mse = a.read()
        assert mse == b.read() and len(mse.splitlines()) == 10


def test_tracker_without_a_weights_file_reports_the_name_as_unknown(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.setenv(em.LPIPS_VGG_WEIGHTS_ENV, str(tmp_path / 'nowhere.pth'))
    monkeypatch.setattr(em.EvalMetricsTracker, '_lpips_vgg_cache', [False, None])
    monkeypatch.setattr(em, '_pyiqa_factory', type('NoPyiqa', (), {'list_of_metrics': []})())      # (as on a machine without pyiqa)
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'lpips-vgg'], has_reference_frames=True)
    out = capsys.readouterr().out
    assert [m.name for m in t.metrics] == ['mse']
    assert 'Unknown metric lpips-vgg' in out and out.count('lpips-vgg: no weights at') == 1
    assert not os.path.exists(tmp_path / 'out' / 'lpips-vgg.txt')
    t.finalize(0)


def test_tracker_refuses_frames_with_a_side_below_16(tmp_path, weights_file, capsys):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'lpips-vgg'], has_reference_frames=True)
    frames, refs = _frames(8, 40, 10)
    _feed(t, frames, refs)
    out = capsys.readouterr().out
    assert out.count('Exception in metric lpips-vgg: ') == 1 and '8x40' in out
    assert open(tmp_path / 'out' / 'lpips-vgg.txt').read() == ''
    assert t.get_mean_scores()['lpips-vgg'] == -1
    assert len(open(tmp_path / 'out' / 'mse.txt').read().splitlines()) == 10


def test_evaluate_writes_the_file_and_leaves_the_others_alone(tmp_path, monkeypatch, weights_file):
    from evreal_amd import eval as ev
    from evreal_amd.eval_metrics import EvalMetricsTracker
    names = _write_tree(str(tmp_path), True, (91, 92))
    monkeypatch.chdir(tmp_path)
    # (with the tree's 3 ms tolerance only two windows of a sequence end near a frame: every window is scored here, so that the
    # queue releases full groups as well as a tail)
    cfg_path = tmp_path / 'config' / 'eval' / 'k3k.json'
    cfg_path.write_text(json.dumps(dict(json.loads(cfg_path.read_text()), ts_tol_ms=1e6)))
    out = lambda n: tmp_path / 'outputs' / 'k3k' / 'NR' / n / 'FireNet'
    read = lambda n, files: {f: open(out(n) / (f + '.txt'), 'rb').read() for f in files}
    monkeypatch.setenv('EVREAL_BATCH_SEQUENCES', '2')
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim'])
    plain = {n: read(n, ('mse', 'ssim')) for n in names}

    seen, precomputed = {}, []
    real = EvalMetricsTracker.update_batch

    def spy(self, indices, imgs, refs, img_ts, ref_ts, scores=None, u8=None):
        rec = seen.setdefault(self.output_dir, [])
        rec += [(i, a, b, ts) for i, a, b, ts in zip(indices, imgs.detach().cpu().numpy().copy(), refs.detach().cpu().numpy().copy(), img_ts)]
        precomputed.append(scores is not None and 'lpips-vgg' in scores and 'mse' in scores)
        return real(self, indices, imgs, refs, img_ts, ref_ts, scores=scores, u8=u8)

    monkeypatch.setattr(EvalMetricsTracker, 'update_batch', spy)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim', 'lpips-vgg'])
    monkeypatch.setattr(EvalMetricsTracker, 'update_batch', real)
    assert precomputed and all(precomputed)      # the chunk loop computed the new name itself: mse / ssim stay on the fast path
    for n in names:
        got = read(n, ('mse', 'ssim', 'lpips-vgg'))
        assert got['mse'] == plain[n]['mse'] and got['ssim'] == plain[n]['ssim'] and plain[n]['mse']
        rec = [v for k, v in seen.items() if k.replace('\\', '/').endswith(f'/{n}/FireNet')][0]
        evaluated = [int(l.split()[0]) for l in got['mse'].decode().splitlines()]
        rec = [r for r in rec if r[0] in set(evaluated)]
        assert [r[0] for r in rec] == evaluated
        assert len(got['lpips-vgg'].splitlines()) == len(evaluated) >= 8
        # the tracker-only path on the same frames
        t = EvalMetricsTracker(output_dir=str(tmp_path / 'again' / n), quan_eval_metric_names=['lpips-vgg'], has_reference_frames=True)
        for k in range(0, len(rec), 4):
            part = rec[k:k + 4]
            t.update_batch([r[0] for r in part], _cuda(np.stack([r[1] for r in part])), _cuda(np.stack([r[2] for r in part])),
                           [r[3] for r in part], None)
        t.finalize(rec[-1][0])
        _compare_lines(got['lpips-vgg'].decode(), open(tmp_path / 'again' / n / 'lpips-vgg.txt').read())
