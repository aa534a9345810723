"""DISTS on the GPU (evr_dists_*, evreal_amd.lpips.DISTS) against the torch-CPU restatement (tests/dists_ref.py) with deterministic
synthetic weights, and the `-qm dists` path of the tracker and of evaluate().  Parity with pyiqa itself is unpinned
(tests/test_dists_pins.py)."""
import json

import numpy as np
import pytest
import torch

import dists_ref as R
from test_gpu_nriqa import _compare_lines, _queue_lines, _write_tree
from vgg_metric_common import _bound, _cuda, _feed, _frames, BATCHES, run_child, write_weights_file

pytestmark = pytest.mark.gpu

# 16x16: the four pools end at one pixel; 37x53: the ceil-mode pool gains a row or a column on several levels (19x27, 10x14, 5x7,
# 3x4); 64x80: several tiles, and cout = 64 and cout >= 128 both reach their kernels
SHAPES = [(16, 16), (37, 53), (64, 80)]
_REF = {}


@pytest.fixture(scope='module')
def sd():
    from evreal_amd import weights
    return weights.synth_dists_state_dict(seed=3)


def _reference(sd, H, W):
    """(img, ref, (total64, stages64), (total32, stages32)) of the test frames at H x W: computed once per shape, never modified."""
    if (H, W) not in _REF:
        img, ref = R.frame_pairs(H, W)
        _REF[(H, W)] = (img, ref, R.dists(sd, img, ref, torch.float64), R.dists(sd, img, ref, torch.float32))
    return _REF[(H, W)]


def _assert_within(got_total, got_stages, ref, tag, scale=1.0):
    _, _, (t64, s64), (t32, s32) = ref
    terms = (('total', got_total, t64, t32), ('stages', got_stages, s64, s32))
    worst = 0.0
    for name, got, w64, w32 in terms:
        ratio = np.abs(got - w64) / _bound(w64, w32, scale)
        print(f'{tag} {name}: error / bound (worst {ratio.max():.3f})\n{ratio}')
        worst = max(worst, float(ratio.max()))
    for name, got, w64, w32 in terms:
        assert (np.abs(got - w64) <= _bound(w64, w32, scale)).all(), (tag, name, got, w64)
    return worst


def _assert_construction_zeros(total, stages, H, W):
    """Pair 0 is identical; pair 3 is a constant against a constant (no texture in the input's feature set); a 1x1 map has no
    variance (relu5_3 of a 16x16 frame): an fp32 value squared is exact in fp64, so the kernels' sum(f^2)/N - mean^2 cancels."""
    assert abs(total[0]) <= 1e-12 and np.abs(stages[0]).max() <= 1e-12
    assert stages[3, 0, 1] == 0.0
    if (H, W) == (16, 16):
        assert np.array_equal(stages[:, 5, 1], np.zeros(len(stages)))


@pytest.mark.parametrize('shape', SHAPES)
def test_totals_and_stages_vs_oracle(sd, shape):
    """For the totals and each of the twelve stage distances |got - want64| <= max(2e-4 |want64| + 1e-7, 8 |want32 - want64|); the
    distances that are zero by construction are exactly zero; the stage distances add up to the score.
    Worst measured error / bound on an MI355X (default h3 arithmetic), all three shapes: totals 0.002, stage distances 0.010."""
    from evreal_amd.lpips import DISTS
    H, W = shape
    ref = _reference(sd, H, W)
    m = DISTS(sd)
    img, rf = _cuda(ref[0]), _cuda(ref[1])
    total = m(img, rf).cpu().numpy()
    stages = m.stages(img, rf).cpu().numpy()
    assert total.shape == (4,) and stages.shape == (4, 6, 2)
    _assert_construction_zeros(total, stages, H, W)
    _assert_construction_zeros(*ref[2], H, W)
    _assert_within(total, stages, ref, f'{H}x{W}')
    np.testing.assert_allclose(stages.sum(axis=(1, 2)), total, rtol=0, atol=1e-12)
    assert m.saturation() == 0
    assert m.flops() > 0


def test_passes_determinism_and_a_handle_that_changes_shape(sd):
    """n = 5 with max_pairs = 2 (passes of 2, 2 and 1 pairs) against one pass within rtol 1e-6, atol 1e-9 (split-K may reorder the
    convolutions' sums); the same call twice is equal bit for bit; a changing n and a changing frame size on one handle give
    exactly what a fresh handle gives."""
    from evreal_amd.lpips import DISTS
    H, W = 37, 53
    rng = np.random.default_rng(5)
    ref = rng.random((5, H, W), dtype=np.float32)
    img = np.clip(ref + 0.1 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    d_img, d_ref = _cuda(img), _cuda(ref)
    one = DISTS(sd)
    want, want_s = one(d_img, d_ref).cpu().numpy(), one.stages(d_img, d_ref).cpu().numpy()
    np.testing.assert_allclose(want[:2], R.dists(sd, img[:2], ref[:2])[0], rtol=2e-4, atol=1e-7)
    chunked = DISTS(sd, max_pairs=2)
    np.testing.assert_allclose(chunked(d_img, d_ref).cpu().numpy(), want, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(chunked.stages(d_img, d_ref).cpu().numpy(), want_s, rtol=1e-6, atol=1e-9)
    assert np.array_equal(one(d_img, d_ref).cpu().numpy(), want)
    assert np.array_equal(chunked(d_img, d_ref).cpu().numpy(), chunked(d_img, d_ref).cpu().numpy())
    fresh = {}
    for n in (3, 5, 1, 2, 5, 3):
        o = int(rng.integers(0, 5 - n + 1))
        if n not in fresh:
            fresh[n] = DISTS(sd)
        got = one(d_img[o:o + n], d_ref[o:o + n]).cpu().numpy()
        np.testing.assert_array_equal(got, fresh[n](d_img[o:o + n], d_ref[o:o + n]).cpu().numpy(), err_msg=f'n={n}')
        np.testing.assert_allclose(got, want[o:o + n], rtol=1e-6, atol=1e-9, err_msg=f'n={n}')
    small_i, small_r = d_img[:2, :16, :24].contiguous(), d_ref[:2, :16, :24].contiguous()
    a = one(d_img[:2], d_ref[:2]).cpu().numpy()
    b = one(small_i, small_r).cpu().numpy()
    c = one(d_img[:2], d_ref[:2]).cpu().numpy()
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(b, DISTS(sd)(small_i, small_r).cpu().numpy())
    np.testing.assert_allclose(b, R.dists(sd, img[:2, :16, :24], ref[:2, :16, :24])[0], rtol=2e-4, atol=1e-7)
    assert one.saturation() == 0 and chunked.saturation() == 0


def test_handles_of_both_trunk_metrics_in_one_process_keep_their_state_apart(sd):
    """An LPIPSVGG and a DISTS handle hold the same trunk code (csrc/vgg_trunk.h): a static, or a plan cached without its handle, would
    show where they alternate call by call on one stream and change shape.  37x53 is the smallest frame whose floor- and ceil-mode
    level sizes differ on several levels, 16x24 the smallest where they still agree; five pairs at max_pairs = 2 run in three passes.
    Every result equals, bit for bit, that of a fresh handle of the same kind given the same call."""
    from evreal_amd import weights
    from evreal_amd.lpips import DISTS, LPIPSVGG
    kinds = ((LPIPSVGG, weights.synth_lpips_vgg_state_dict(seed=3)), (DISTS, sd))
    big = [_cuda(a) for a in R.frame_pairs(37, 53)]
    small = [_cuda(a[1:3]) for a in R.frame_pairs(16, 24)]
    five = [_cuda(a[[0, 1, 2, 3, 1]]) for a in R.frame_pairs(37, 53)]
    handles = []
    for max_pairs, calls in ((0, (big, small, big)), (2, (five,))):
        pair = [cls(w, max_pairs=max_pairs) for cls, w in kinds]
        got = [m(img, ref) for img, ref in calls for m in pair]      # alternating; nothing waits for a result in between
        want = []
        for img, ref in calls:
            fresh = [cls(w, max_pairs=max_pairs) for cls, w in kinds]
            want += [m(img, ref) for m in fresh]
            handles += fresh
        for k, (g, w) in enumerate(zip(got, want)):
            g, w = g.cpu().numpy(), w.cpu().numpy()
            assert g.max() > 1e-3, (max_pairs, k, g)
            np.testing.assert_array_equal(g, w, err_msg=f'max_pairs={max_pairs} call {k // 2} {kinds[k % 2][0].__name__}')
        handles += pair
    assert [m.saturation() for m in handles] == [0] * len(handles)


def test_a_side_below_16_and_a_frame_too_large_are_refused(sd):
    from evreal_amd import lib as L
    from evreal_amd.lpips import DISTS
    m = DISTS(sd)
    x = _cuda(np.zeros((2, 15, 40), np.float32))
    with pytest.raises(ValueError, match='15x40'):
        m(x, x)
    out = torch.full((2,), 7.0, dtype=torch.float64, device='cuda')      # the C entry point refuses it too, before any launch
    rc = m.lib.evr_dists_forward(m.handle, L.ptr(x), L.ptr(x), 2, 15, 40, 1, L.ptr(out), None, L.stream_ptr())
    assert rc == -1 and b'too small' in m.lib.evr_last_error() and b'40x15' in m.lib.evr_last_error()
    rc = m.lib.evr_dists_forward(m.handle, L.ptr(x), L.ptr(x), 1, 2048, 2048, 1, L.ptr(out), None, L.stream_ptr())      # H * W = 2^22
    assert rc == -1 and b'too large' in m.lib.evr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), [7.0, 7.0])


@pytest.mark.parametrize('clip', [True, False])
def test_clip_of_the_input(sd, clip):
    """Frames that leave [0,1]: with clip the kernels score clip(x, 0, 1), without it x as it is -- against the oracle, which never
    clips, on the input prepared accordingly (the gate of test_totals_and_stages_vs_oracle)."""
    from evreal_amd.lpips import DISTS
    H, W = 37, 53
    ref = R.frame_pairs(H, W)[1][1:3]
    rng = np.random.default_rng(23)
    img = (ref + 0.4 * rng.standard_normal(ref.shape)).astype(np.float32)
    assert (img < 0).mean() > 0.02 and (img > 1).mean() > 0.02
    seen = np.clip(img, 0, 1) if clip else img
    want = (img, ref, R.dists(sd, seen, ref, torch.float64), R.dists(sd, seen, ref, torch.float32))
    other = R.dists(sd, img if clip else np.clip(img, 0, 1), ref, torch.float64)[0]
    # the two readings are more than two bounds apart on every pair: a kernel that took the other one cannot pass
    assert (np.abs(other - want[2][0]) > 2 * _bound(want[2][0], want[3][0])).all()
    m = DISTS(sd)
    total = m(_cuda(img), _cuda(ref), clip=clip).cpu().numpy()
    stages = m.stages(_cuda(img), _cuda(ref), clip=clip).cpu().numpy()
    _assert_within(total, stages, want, f'clip={clip}')


_CHILD = r'''
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np, torch
import dists_ref as R
from evreal_amd import weights
from evreal_amd.lpips import DISTS
sd = weights.synth_dists_state_dict(seed=3)
img, ref = R.frame_pairs(37, 53)
m = DISTS(sd)
a, b = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
print('RESULT ' + json.dumps({'total': m(a, b).cpu().numpy().tolist(), 'stages': m.stages(a, b).cpu().numpy().tolist(),
                              'sat': m.saturation()}))
'''


@pytest.mark.parametrize('mode,scale', [('fp32', 1.0), ('mx', 10.0), ('mx6', 10.0)])
def test_arithmetic_modes(sd, mode, scale):
    """One fresh child process per mode (the library reads EVR_ARITH once), 37 x 53 with the four pairs.  fp32 takes the bound of
    test_totals_and_stages_vs_oracle; mx and mx6 (which the backbone runs as mx) ten times that bound: the ratio between this
    project's image gates for those modes and for h3 (1e-4 against 1e-5).
    Worst measured error / bound on an MI355X: fp32 totals 0.002, stage distances 0.010; mx and mx6 (of their ten-fold bound)
    totals 0.006, stage distances 0.025."""
    got = run_child(_CHILD, mode)
    total, stages = np.array(got['total']), np.array(got['stages'])
    _assert_construction_zeros(total, stages, 37, 53)
    _assert_within(total, stages, _reference(sd, 37, 53), mode, scale)
    assert got['sat'] == 0


@pytest.fixture()
def weights_file(tmp_path, monkeypatch, sd):
    from evreal_amd import eval_metrics as em
    return write_weights_file(tmp_path, monkeypatch, sd, 'dists.pth', em.DISTS_WEIGHTS_ENV, '_dists_cache')


def test_tracker_books_like_the_reference_queue(tmp_path, weights_file, sd):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    from evreal_amd.lpips import DISTS
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'dists'], has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['mse', 'dists'] and t.wants_precomputed() == ['mse', 'dists']
    frames, refs = _frames(32, 40, 10)
    idx = _feed(t, frames, refs)
    m, scores, k = DISTS(sd), [], 0
    for n in BATCHES:      # the handle's own scores, in the tracker's batches
        scores += m(_cuda(np.stack(frames[k:k + n])), _cuda(np.stack(refs[k:k + n])), clip=True).cpu().numpy().tolist()
        k += n
    got = open(tmp_path / 'out' / 'dists.txt').read()
    assert len(got.splitlines()) == 10 and got == _queue_lines(idx, scores)
    assert min(scores) > 1e-3
    assert abs(t.get_mean_scores()['dists'] - np.mean(scores)) <= 1e-12
    plain = EvalMetricsTracker(output_dir=str(tmp_path / 'plain'), quan_eval_metric_names=['mse'], has_reference_frames=True)
    _feed(plain, frames, refs)
    with open(tmp_path / 'out' / 'mse.txt', 'rb') as a, open(tmp_path / 'plain' / 'mse.txt', 'rb') as b:
        mse = a.read()
        assert mse == b.read() and len(mse.splitlines()) == 10


def test_tracker_refuses_frames_with_a_side_below_16(tmp_path, weights_file, capsys):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'dists'], has_reference_frames=True)
    frames, refs = _frames(8, 40, 10)
    _feed(t, frames, refs)
    out = capsys.readouterr().out
    assert out.count('Exception in metric dists: ') == 1 and '8x40' in out
    assert open(tmp_path / 'out' / 'dists.txt').read() == ''
    assert t.get_mean_scores()['dists'] == -1
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
        precomputed.append(scores is not None and 'dists' in scores and 'mse' in scores)
        return real(self, indices, imgs, refs, img_ts, ref_ts, scores=scores, u8=u8)

    monkeypatch.setattr(EvalMetricsTracker, 'update_batch', spy)
    ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim', 'dists'])
    monkeypatch.setattr(EvalMetricsTracker, 'update_batch', real)
    assert precomputed and all(precomputed)      # the chunk loop computed the new name itself: mse / ssim stay on the fast path
    for n in names:
        got = read(n, ('mse', 'ssim', 'dists'))
        assert got['mse'] == plain[n]['mse'] and got['ssim'] == plain[n]['ssim'] and plain[n]['mse']
        rec = [v for k, v in seen.items() if k.replace('\\', '/').endswith(f'/{n}/FireNet')][0]
        evaluated = [int(l.split()[0]) for l in got['mse'].decode().splitlines()]
        rec = [r for r in rec if r[0] in set(evaluated)]
        assert [r[0] for r in rec] == evaluated
        assert len(got['dists'].splitlines()) == len(evaluated) >= 8
        # the tracker-only path on the same frames
        t = EvalMetricsTracker(output_dir=str(tmp_path / 'again' / n), quan_eval_metric_names=['dists'], has_reference_frames=True)
        for k in range(0, len(rec), 4):
            part = rec[k:k + 4]
            t.update_batch([r[0] for r in part], _cuda(np.stack([r[1] for r in part])), _cuda(np.stack([r[2] for r in part])),
                           [r[3] for r in part], None)
        t.finalize(rec[-1][0])
        _compare_lines(got['dists'].decode(), open(tmp_path / 'again' / n / 'dists.txt').read())
