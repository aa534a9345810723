"""VIFp on the GPU (evr_vifp, evreal_amd.prepost.VIFP) against the numpy oracle (tests/vifp_ref.py) fed the library's own taps
(evr_vifp_taps), and the `-qm vifp` path of the tracker and of evaluate() against the oracle fed through the reference's
four-frame queue."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import vifp_ref as V
from test_gpu_frmetrics import _pair as _textured_pair
from test_gpu_nriqa import _compare_lines, _queue_lines, _write_tree
from thirdparty_refs import image_pairs

pytestmark = pytest.mark.gpu

TH, TW = 16, 32         # the kernel's tile, in window anchors (csrc/vifp.hip)
# A scale's grid covers the anchors of the next scale's window (side - N' + 1) and masks its own moments to side - N + 1.  Sides
# that put either count one below, at and one above a multiple of the tile: at scale 1 (N = 17, N' = 9) H - 8 and H - 16 around
# 48 and 32, W - 8 and W - 16 around 64; at scale 2 (side ceil((H - 8) / 2), N = 9, N' = 5) the side minus 4 and minus 8 around 16
# (rows) and 32 (columns).  Every one of them spans more than one tile in at least one direction.
EDGE_H = [55, 56, 57, 47, 48, 49, 46, 50, 54, 58, 56]
EDGE_W = [71, 72, 73, 79, 80, 81, 78, 82, 86, 88, 90]
SMALL = [(41, 41), (41, 48), (42, 43), (43, 42)] + list(zip(EDGE_H, EDGE_W))
LARGE = [(57, 73), (97, 131), (260, 346)]
REL_TERM, REL_SCORE = 1e-10, 3e-10


def _noise_pair(H, W, seed):
    rng = np.random.default_rng([seed, H, W])
    return rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32)


def _wide_pair(H, W, seed):
    """Values from about -1.3 to 2.3: with clip, whole regions saturate into flat 0 or 1 in either frame or in both (the EPS
    branches: s1 < EPS, s2 < EPS, sv <= EPS), without it nothing does."""
    a, b = _noise_pair(H, W, seed)
    yy, xx = np.mgrid[0:H, 0:W]
    bump = np.float32(0.5) + (1.5 * np.sin(xx / 12.0) * np.cos(yy / 10.0)).astype(np.float32)
    return ((bump + np.float32(0.3) * (a - np.float32(0.5))).astype(np.float32),
            (np.float32(0.8) * bump + np.float32(0.3) * (b - np.float32(0.5))).astype(np.float32))


def _piecewise_pair(H, W, seed):
    """Constant blocks of 24 x 40 pixels (wider than every window), the image's levels a gain and an offset away from the
    reference's, one block inverted (a negative gain) and one flattened."""
    rng = np.random.default_rng([seed, H, W, 3])
    levels = rng.random(((H + 23) // 24, (W + 39) // 40), dtype=np.float32)
    ref = np.ascontiguousarray(np.kron(levels, np.ones((24, 40), np.float32))[:H, :W].astype(np.float32))
    img = (np.float32(0.8) * ref + np.float32(0.05)).astype(np.float32)
    img[:30, :50] = np.float32(1.0) - img[:30, :50]
    img[30:, 50:] = np.float32(0.4)
    return img, ref


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


@pytest.fixture(scope='module')
def vf():
    from evreal_amd.prepost import VIFP
    return VIFP()


@pytest.fixture(scope='module')
def taps():
    from evreal_amd import lib as L
    lib, out = L.load(), []
    for s in (1, 2, 3, 4):
        buf = (ctypes.c_double * (2 ** (5 - s) + 1))()
        assert lib.evr_vifp_taps(s, ctypes.cast(buf, ctypes.c_void_p)) == 0
        out.append(np.array(buf[:]))
    return out


def _check(vf, taps, imgs, refs, clip, tag, worst):
    rows = vf.stats(_cuda(np.stack(imgs)), _cuda(np.stack(refs)), clip=clip).cpu().numpy()
    assert rows.shape == (len(imgs), 9)
    for k, (img, ref) in enumerate(zip(imgs, refs)):
        want = V.scales(img, ref, clip, taps)
        score = V.vifp(img, ref, clip, taps)
        got = np.stack([rows[k, 1:5], rows[k, 5:9]], axis=1)
        rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
        d_score = abs(rows[k, 0] - score) / abs(score) if math.isfinite(score) and score != 0 else 0.0
        print(f'{tag} clip={clip} frame {k}: score {score:.9f}, terms {rel.max():.2e}, score {d_score:.2e}')
        worst['term'] = max(worst.get('term', 0.0), rel.max())
        worst['score'] = max(worst.get('score', 0.0), d_score)
        assert (want >= 0).all() and (got >= 0).all()
        assert (got[want == 0] == 0).all(), (tag, clip, k)
        assert (np.abs(got - want) <= REL_TERM * want).all(), (tag, clip, k, rel.max())
        if math.isnan(score):
            assert math.isnan(rows[k, 0]), (tag, clip, k)
        elif score == 0:
            assert rows[k, 0] == 0, (tag, clip, k)
        else:
            assert abs(rows[k, 0] - score) <= REL_SCORE * abs(score), (tag, clip, k, d_score)


@pytest.mark.parametrize('clip', [True, False])
def test_scales_and_scores_match_the_oracle(vf, taps, clip):
    """Gates (derived, not tuned): every num_s and den_s within 1e-10 relative, an exact 0 where the oracle's is 0 -- the terms
    are non-negative, the arguments of log10 are bit-identical by construction (the same taps, the same operation order, no
    fused multiply-add on either side), log10 is within an ulp or two, and a sum of at most 6.1e5 terms in another order moves
    by at most n * 2^-53 = 6.7e-11 relative; the score within 3e-10 relative.
    Measured on an MI355X over all shapes and kinds, clipped and unclipped: terms <= 4.40e-16 relative, score <= 4.08e-16."""
    worst = {}
    for k, (H, W) in enumerate(SMALL):
        pairs = [_noise_pair(H, W, k), _wide_pair(H, W, k + 100)]
        _check(vf, taps, [p[0] for p in pairs], [p[1] for p in pairs], clip, f'{H}x{W}', worst)
    for k, (H, W) in enumerate(LARGE):
        pairs = [_textured_pair(H, W, k), _piecewise_pair(H, W, k), _wide_pair(H, W, k + 10)]
        _check(vf, taps, [p[0] for p in pairs], [p[1] for p in pairs], clip, f'{H}x{W}', worst)
    _check(vf, taps, [_textured_pair(625, 970, 7)[0]], [_textured_pair(625, 970, 7)[1]], clip, '625x970', worst)
    for name, img, ref in image_pairs():
        _check(vf, taps, [img, ref], [ref, img], clip, name, worst)
    print('largest relative distances:', {k: f'{v:.2e}' for k, v in worst.items()})


def test_identical_constant_and_swapped_frames(vf, taps):
    for H, W in ((41, 41), (97, 131), (260, 346)):
        img, ref = _textured_pair(H, W, 4)
        same = vf(_cuda(ref[None]), _cuda(ref[None])).cpu().numpy()[0]
        assert same < 1.0 and 1.0 - same <= 1e-9, (H, W, same)         # the +EPS of g: not exactly 1
        flat, other = np.full((H, W), 0.3, np.float32), np.full((H, W), 0.7, np.float32)
        tex = _noise_pair(H, W, 5)[0]
        got = vf.stats(_cuda(np.stack([flat, flat, tex])), _cuda(np.stack([tex, other, flat]))).cpu().numpy()
        assert got[0, 0] == 0.0 and (got[0, 1:5] == 0.0).all() and (got[0, 5:9] > 0.0).all()     # a constant image against texture
        assert math.isnan(got[1, 0]) and (got[1, 1:] == 0.0).all()                               # two constant frames: 0 / 0
        assert math.isnan(got[2, 0]) and (got[2, 1:] == 0.0).all()                               # a flat reference
        ab = vf(_cuda(img[None]), _cuda(ref[None])).cpu().numpy()[0]
        ba = vf(_cuda(ref[None]), _cuda(img[None])).cpu().numpy()[0]
        want_ab, want_ba = V.vifp(img, ref, True, taps), V.vifp(ref, img, True, taps)
        assert abs(want_ab - want_ba) > 1e-3 * want_ab                  # the metric is not symmetric
        assert abs(ab - want_ab) <= REL_SCORE * want_ab and abs(ba - want_ba) <= REL_SCORE * want_ba


def test_a_side_of_40_is_refused_before_any_launch(vf):
    from evreal_amd import lib as L
    for H, W in ((40, 64), (64, 40)):
        x = _cuda(np.zeros((2, H, W), np.float32))
        with pytest.raises(ValueError, match=f'{H}x{W}'):
            vf(x, x)
    lib = L.load()
    x = _cuda(np.zeros((1, 40, 346), np.float32))
    out = torch.full((1, 9), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    rc = lib.evr_vifp(L.ptr(x), L.ptr(x), 1, 40, 346, 1, L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == -1 and b'40 x 346' in lib.evr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.full((1, 9), 7.0))      # nothing was launched


def test_bitwise_independent_of_batch_and_position(vf, taps):
    rng = np.random.default_rng(16)
    imgs, refs = _cuda(rng.random((16, 97, 131), dtype=np.float32)), _cuda(rng.random((16, 97, 131), dtype=np.float32))
    full = _bits(vf.stats(imgs, refs))
    assert np.array_equal(_bits(vf.stats(imgs, refs)), full)
    fives = [_bits(vf.stats(imgs[i:i + 5], refs[i:i + 5])) for i in range(0, 16, 5)]
    assert np.array_equal(np.concatenate(fives), full)
    for i in range(16):
        assert np.array_equal(_bits(vf.stats(imgs[i:i + 1], refs[i:i + 1]))[0], full[i]), i
    perm = torch.arange(15, -1, -1, device='cuda')
    assert np.array_equal(_bits(vf.stats(imgs[perm].contiguous(), refs[perm].contiguous()))[::-1], full)
    assert np.array_equal(_bits(vf(imgs, refs)), full[:, 0])
    sc = _bits(vf.scales(imgs, refs))
    assert sc.shape == (16, 4, 2) and np.array_equal(sc[:, :, 0], full[:, 1:5]) and np.array_equal(sc[:, :, 1], full[:, 5:9])
    out = torch.zeros((16, 9), dtype=torch.float64, device='cuda')
    col = vf(imgs, refs, out=out)
    assert np.array_equal(_bits(out), full) and col.data_ptr() == out.data_ptr() and np.array_equal(_bits(col), full[:, 0])
    want = V.vifp(imgs[3].cpu().numpy(), refs[3].cpu().numpy(), True, taps)
    assert abs(np.ascontiguousarray(full[3]).view(np.float64)[0] - want) <= REL_SCORE * want


def test_more_frames_than_one_grid_axis_holds(vf, taps):
    """Frames ride the grid's z axis, chunked at 65535: 65537 pairs against the first and the last 100 computed alone."""
    n = 65537
    g = torch.Generator(device='cuda').manual_seed(65537)
    imgs = torch.rand((n, 41, 41), device='cuda', generator=g)
    refs = torch.rand((n, 41, 41), device='cuda', generator=g)
    full = _bits(vf.stats(imgs, refs))
    for sl in (slice(0, 100), slice(n - 100, n)):
        assert np.array_equal(_bits(vf.stats(imgs[sl].contiguous(), refs[sl].contiguous())), full[sl])
    k = n - 1
    want = V.vifp(imgs[k].cpu().numpy(), refs[k].cpu().numpy(), True, taps)
    assert abs(np.ascontiguousarray(full[k]).view(np.float64)[0] - want) <= REL_SCORE * abs(want)


def test_existing_metrics_are_untouched(vf):
    from evreal_amd.prepost import GMSD, FullRefMetrics, Metrics
    pairs = [_textured_pair(260, 346, s) for s in range(5)]
    imgs, refs = _cuda(np.stack([p[0] for p in pairs])), _cuda(np.stack([p[1] for p in pairs]))
    m, fr, gm = Metrics(), FullRefMetrics(), GMSD()
    before = [_bits(m(imgs, refs)), _bits(fr(imgs, refs)), _bits(gm.stats(imgs, refs))]
    keep_i, keep_r = imgs.clone(), refs.clone()
    got = vf(imgs, refs).cpu().numpy()
    assert np.isfinite(got).all() and (got > 0).all()
    assert torch.equal(imgs, keep_i) and torch.equal(refs, keep_r)       # the inputs are read only
    after = [_bits(m(imgs, refs)), _bits(fr(imgs, refs)), _bits(gm.stats(imgs, refs))]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def _feed(t, frames, refs):
    idx, k = list(range(len(frames))), 0
    for n in (3, 5, 3):
        t.update_batch(idx[k:k + n], _cuda(np.stack(frames[k:k + n])), _cuda(np.stack(refs[k:k + n])),
                       [0.01 * i for i in idx[k:k + n]], None)
        k += n
    t.finalize(idx[-1])
    return idx


@pytest.mark.parametrize('hist_eq', ['none', 'global'])
def test_tracker_books_like_the_reference_queue(tmp_path, taps, hist_eq):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    from evreal_amd.prepost import histogram_equalization
    t = EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['mse', 'vifp'],
                           has_reference_frames=True, hist_eq=hist_eq)
    assert [m.name for m in t.metrics] == ['mse', 'vifp']
    assert t.wants_precomputed() == (['mse', 'vifp'] if hist_eq == 'none' else [])
    pairs = [_textured_pair(260, 346, s) for s in range(11)]
    frames, refs = [p[0] for p in pairs], [p[1] for p in pairs]
    idx = _feed(t, frames, refs)
    if hist_eq != 'none':       # the oracle sees the frames the tracker's equalisation hands to the metrics
        eq = lambda a: histogram_equalization(torch.clamp(_cuda(np.stack(a)), 0.0, 1.0).contiguous(), hist_eq).cpu().numpy()
        frames, refs = list(eq(frames)), list(eq(refs))
    got = open(tmp_path / 'out' / 'vifp.txt').read()
    assert len(got.splitlines()) == 11
    _compare_lines(got, _queue_lines(idx, [V.vifp(a, b, True, taps) for a, b in zip(frames, refs)]))
    assert len(open(tmp_path / 'out' / 'mse.txt').read().splitlines()) == 11
    assert 0 < t.get_mean_scores()['vifp'] < 1


def test_evaluate_writes_the_same_files_one_sequence_at_a_time_and_batched(tmp_path, monkeypatch, taps):
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
        ev.evaluate(['FireNet'], ['k3k'], ['NR'], ['mse', 'ssim', 'vifp'])
        monkeypatch.setattr(EvalMetricsTracker, 'update_batch', real)
        runs[S] = {n: read(n, ('mse', 'ssim', 'vifp')) for n in names}
    assert runs[1] == runs[2]
    for n in names:
        assert runs[2][n]['mse'] == plain[n]['mse'] and runs[2][n]['ssim'] == plain[n]['ssim'] and plain[n]['mse']
        rec = [v for k, v in seen.items() if k.replace('\\', '/').endswith(f'/{n}/FireNet')][0]
        evaluated = [int(l.split()[0]) for l in runs[2][n]['mse'].splitlines()]
        rec = [r for r in rec if r[0] in set(evaluated)]
        assert [r[0] for r in rec] == evaluated and len(evaluated) >= 8
        assert len(runs[2][n]['vifp'].splitlines()) == len(evaluated)
        _compare_lines(runs[2][n]['vifp'], _queue_lines(evaluated, [V.vifp(a, b, True, taps) for _, a, b in rec]))
