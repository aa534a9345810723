"""VIFp without a GPU: the numpy oracle (tests/vifp_ref.py) against facts independent of it -- scipy's correlate2d with the
two-dimensional window, the properties of the metric -- and the library's taps, the C entry's handling of its arguments, and the
tracker's handling of the name and the shape."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vifp_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(41, 41), (41, 48), (57, 73), (64, 80), (97, 131)]


def _pair(H, W, seed):
    rng = np.random.default_rng([seed, H, W])
    return rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32)


def _texture(H, W, seed=5):
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.mgrid[0:H, 0:W]
    return np.clip(0.5 + 0.25 * np.sin(xx / 5.0) * np.cos(yy / 6.0) + 0.1 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)


def _filt2d(a, w):
    from scipy.signal import correlate2d
    return correlate2d(a, np.outer(w, w), mode='valid')


@pytest.mark.parametrize('H,W', SIZES)
def test_separable_restatement_equals_correlate2d_with_the_2d_window(H, W):
    """Another filter routine, another summation order: 1e-12 on the scores, on pairs that keep every window's variance at least
    1e-3 away from the thresholds (asserted first), so that no branch can fall the other way."""
    img, ref = _pair(H, W, 1)
    v1, v2 = V.min_variances(img, ref)
    assert v1 >= 1e-3 and v2 >= 1e-3, (v1, v2)
    a, b = V.vifp(img, ref), V.vifp(img, ref, filt=_filt2d)
    print(f'{H}x{W}: {a:.12f}, difference {abs(a - b):.2e}, smallest variances {v1:.3g} {v2:.3g}')
    assert abs(a - b) <= 1e-12
    assert np.abs(V.scales(img, ref) - V.scales(img, ref, filt=_filt2d)).max() <= 1e-12 * V.scales(img, ref).max()


def test_properties_of_the_metric():
    from scipy.ndimage import gaussian_filter
    ref = _texture(97, 131)
    same = V.vifp(ref, ref)
    assert same < 1.0 and 1.0 - same <= 1e-9                    # the +EPS of g: not exactly 1
    blur = V.vifp(gaussian_filter(ref, 1.5), ref)
    assert 0.0 < blur < 0.9
    stretched = (np.float32(0.5) + np.float32(1.5) * (ref - np.float32(0.5))).astype(np.float32)
    assert V.vifp(stretched, ref, clip=False) > 1.05            # a gain above 1 carries more than the reference's information
    rng = np.random.default_rng(3)
    noisy = np.clip(ref + 0.1 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    assert 0.0 < V.vifp(noisy, ref) < blur + 0.9
    flat = np.full_like(ref, 0.3)
    assert V.vifp(flat, ref) == 0.0                             # exactly: every g is 0
    assert math.isnan(V.vifp(flat, flat)) and math.isnan(V.vifp(ref, flat))     # 0 / 0: a flat reference
    assert V.vifp(noisy, ref) != V.vifp(ref, noisy)             # not symmetric


def test_size_limit_and_the_pyramid_sides():
    img, ref = _pair(64, 64, 2)
    for H, W in ((40, 64), (64, 40)):
        with pytest.raises(ValueError, match=f'{H}x{W}'):
            V.vifp(img[:H, :W], ref[:H, :W])
    t = V.terms(img[:41, :41], ref[:41, :41])
    assert [m[0].shape for m in t] == [(25, 25), (9, 9), (3, 3), (1, 1)]
    t = V.terms(img[:42, :43], ref[:42, :43])
    assert [m[0].shape for m in t] == [(26, 27), (9, 10), (3, 3), (1, 1)]
    assert math.isfinite(V.vifp(img[:41, :41], ref[:41, :41]))


def test_clip_matters_and_nothing_is_quantised():
    img, ref = _pair(48, 48, 4)
    wide = (np.float32(1.6) * img - np.float32(0.3)).astype(np.float32)
    assert V.vifp(wide, ref, clip=True) != V.vifp(wide, ref, clip=False)
    assert V.vifp(wide, ref, clip=True) == V.vifp(np.clip(wide, 0, 1), ref, clip=False)
    fine = (img + np.float32(1e-4)).astype(np.float32)          # far below a grey level of 1 / 255
    assert V.vifp(fine, ref) != V.vifp(img, ref)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from evreal_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _taps(lib, s):
    N = 2 ** (5 - s) + 1
    buf = (ctypes.c_double * (N + 1))()
    buf[N] = 7.0
    assert lib.evr_vifp_taps(s, ctypes.cast(buf, ctypes.c_void_p)) == 0
    assert buf[N] == 7.0                                        # N_s doubles and no more
    return np.array(buf[:N])


def test_the_library_hands_out_its_taps(lib):
    for s, N in zip((1, 2, 3, 4), (17, 9, 5, 3)):
        got, want = _taps(lib, s), V.window(s)
        assert got.shape == want.shape == (N,)
        assert (np.abs(got - want) <= 2 * np.spacing(want)).all(), s
        assert abs(math.fsum(got) - 1.0) <= N * 2.0 ** -53, s
        assert np.array_equal(got, got[::-1]) or np.abs(got - got[::-1]).max() <= 2 * np.spacing(got.max())
    buf = (ctypes.c_double * 17)()
    for s in (0, 5):
        assert lib.evr_vifp_taps(s, ctypes.cast(buf, ctypes.c_void_p)) == -1 and b'evr_vifp_taps' in lib.evr_last_error()
    assert lib.evr_vifp_taps(1, None) == -1
    # the oracle fed these taps is the oracle
    img, ref = _pair(57, 73, 6)
    assert abs(V.vifp(img, ref, taps=[_taps(lib, s) for s in (1, 2, 3, 4)]) - V.vifp(img, ref)) <= 1e-12


def test_argument_validation_without_gpu(lib):
    assert lib.evr_vifp_workspace_bytes(-1, 260, 346) == 0 and lib.evr_vifp_workspace_bytes(2, 40, 346) == 0
    assert lib.evr_vifp_workspace_bytes(2, 346, 40) == 0
    one, two = lib.evr_vifp_workspace_bytes(1, 260, 346), lib.evr_vifp_workspace_bytes(2, 260, 346)
    # the three lower levels of both planes in fp64 (126x169, 61x83, 30x41) and a pair of doubles per tile
    levels = 2 * 8 * (126 * 169 + 61 * 83 + 30 * 41)
    assert levels <= two - one <= levels + 3 * 256 + 16 * 512
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)           # a non-null HOST address: every call below must return before it is used
    call = lambda img, ref, n, H, W, out: lib.evr_vifp(img, ref, n, H, W, 1, out, p, 1 << 30, None)
    assert call(p, p, -1, 260, 346, p) == -1 and b'evr_vifp' in lib.evr_last_error()
    assert call(p, p, 1, 0, 346, p) == -1
    assert call(p, p, 1, 40, 346, p) == -1 and b'40 x 346' in lib.evr_last_error()
    assert call(p, p, 1, 260, 40, p) == -1 and b'260 x 40' in lib.evr_last_error()
    assert call(p, p, 0, 40, 346, p) == -1          # the size limit does not wait for a frame
    assert call(p, p, 0, 260, 346, p) == 0          # n == 0 launches nothing
    assert call(None, p, 1, 260, 346, p) == -1 and b'null' in lib.evr_last_error()
    assert call(p, None, 1, 260, 346, p) == -1 and call(p, p, 1, 260, 346, None) == -1
    assert lib.evr_vifp(p, p, 1, 260, 346, 1, p, None, 0, None) == -1 and b'workspace' in lib.evr_last_error()
    assert lib.evr_vifp(p, p, 1, 260, 346, 1, p, p, one - 1, None) == -1 and b'workspace' in lib.evr_last_error()
    assert lib.evr_version() == 1005


def test_header_declares_the_entry_points():
    from evreal_amd import lib as L
    hdr = open(os.path.join(ROOT, 'include', 'evreal_hip.h')).read()
    for name in ('evr_vifp_workspace_bytes', 'evr_vifp', 'evr_vifp_taps'):
        assert name + '(' in hdr and name in L.SYMBOLS, name
    assert L.SYMBOLS['evr_vifp_workspace_bytes'][0] is ctypes.c_size_t and len(L.SYMBOLS['evr_vifp'][1]) == 10


def test_vifp_object_needs_no_gpu_to_exist():
    from evreal_amd.prepost import VIFP
    m = VIFP()
    assert m.ws is None and m.lib is None and VIFP.MIN_SIDE == 41
    assert m.too_small(41, 41) is None and m.too_small(260, 346) is None
    assert '40x346' in m.too_small(40, 346) and '260x40' in m.too_small(260, 40)


# ---- tracker: routing with a CPU stand-in (the manner of tests/test_metric_table_cpu.py) --------------------------------------------
UNUSED = 1e6        # the num / den columns: no file may hold them


class _StandIn:
    def __init__(self, *bases, returns_first=False):
        self.bases, self.returns_first, self.calls = bases, returns_first, 0

    def __call__(self, img, ref=None, clip=True, out=None, **flags):
        assert clip is True
        self.calls += 1
        n = img.shape[0]
        rows = torch.stack([b + torch.arange(n, dtype=torch.float64) for b in self.bases], dim=1)
        if out is not None:
            out.copy_(rows)
            rows = out
        return rows[:, 0] if self.returns_first else rows       # (GMSD and VIFP write whole rows and return the first column)


BATCHES = (3, 2, 1)
IN_BATCH = [j for n in BATCHES for j in range(n)]


def _tracker(tmp_path, monkeypatch, names, sub='out'):
    from evreal_amd import eval_metrics as em
    for env in (em.GMSD_ENV, em.VIFP_ENV):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(em, '_pyiqa_factory', SimpleNamespace(list_of_metrics=[]))     # pyiqa not installed
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / sub), quan_eval_metric_names=list(names), has_reference_frames=True)
    stand = dict(gpu=_StandIn(10, 20), gmsd=_StandIn(50, UNUSED, returns_first=True),
                 vifp=_StandIn(*([70] + [UNUSED] * 8), returns_first=True))
    t._gpu, t._gmsd, t._vifp = stand['gpu'], stand['gmsd'], stand['vifp']
    return t, stand


def _feed(t, H, W):
    k = 0
    for n in BATCHES:
        idx = list(range(k, k + n))
        t.update_batch(idx, torch.zeros((n, H, W)), torch.zeros((n, H, W)), [0.01 * i for i in idx], None)
        k += n
    t.finalize(k - 1)


def _lines(t, name):
    return open(f'{t.output_dir}/{name}.txt').read().splitlines()


def test_only_the_score_column_reaches_the_file(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    t, stand = _tracker(tmp_path, monkeypatch, ['mse', 'vifp', 'gmsd'])
    assert [m.name for m in t.metrics] == ['mse', 'vifp', 'gmsd'] and t.wants_precomputed() == ['mse', 'vifp', 'gmsd']
    assert isinstance(t.metrics[1], em.QueuedGpuMetric) and t.metrics[1].no_ref is False
    _feed(t, 200, 200)
    for name, base in (('mse', 10), ('vifp', 70), ('gmsd', 50)):
        assert _lines(t, name) == ['{} {:.5f}'.format(i, base + j) for i, j in enumerate(IN_BATCH)], name
    assert t.get_mean_scores()['vifp'] == pytest.approx(70 + np.mean(IN_BATCH), abs=1e-12)
    assert stand['vifp'].calls == len(BATCHES)
    out = capsys.readouterr().out
    assert 'Exception in metric' not in out and 'Unknown metric' not in out


def test_frames_below_41_are_refused_by_shape_with_one_line(tmp_path, monkeypatch, capsys):
    t, stand = _tracker(tmp_path, monkeypatch, ['mse', 'vifp', 'gmsd'])
    _feed(t, 40, 200)
    out = capsys.readouterr().out
    assert out.count('Exception in metric vifp: ') == 1 and '40x200' in out and out.count('Exception in metric') == 1
    assert _lines(t, 'vifp') == [] and t.get_mean_scores()['vifp'] == -1
    assert stand['vifp'].calls == 0                             # decided from the shape: never launched
    for name, base in (('mse', 10), ('gmsd', 50)):
        assert _lines(t, name) == ['{} {:.5f}'.format(i, base + j) for i, j in enumerate(IN_BATCH)], name
    assert t.get_num_quan_evaluations() == 6


def test_the_name_without_reference_frames_and_under_equalisation(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    monkeypatch.delenv(em.VIFP_ENV, raising=False)
    T = lambda **kw: em.EvalMetricsTracker(output_dir=str(tmp_path / 'o'), quan_eval_metric_names=['vifp'], **kw)
    t = T(has_reference_frames=True)
    assert os.path.exists(tmp_path / 'o' / 'vifp.txt') and t.get_mean_scores() == {'vifp': -1}
    assert T(has_reference_frames=True, hist_eq='global').wants_precomputed() == []
    t = T(has_reference_frames=False)
    assert t.metrics == [] and t.wants_precomputed() == []


def test_opt_out_sends_the_name_down_the_old_path(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.setenv(em.VIFP_ENV, '0')
    assert em.VIFP_ENV == 'EVREAL_GPU_VIFP' and not em.gpu_vifp_enabled()
    monkeypatch.setattr(em, '_pyiqa_factory', SimpleNamespace(list_of_metrics=[]))     # pyiqa not installed
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'o'), quan_eval_metric_names=['vifp'], has_reference_frames=True)
    assert t.metrics == [] and 'Unknown metric vifp' in capsys.readouterr().out


def test_a_registered_plug_in_takes_precedence(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em

    class Mine(em.BaseMetric):
        def __init__(self):
            super().__init__('vifp')

    monkeypatch.setitem(em._REGISTRY, 'vifp', Mine)
    t, _ = _tracker(tmp_path, monkeypatch, ['vifp'])
    assert isinstance(t.metrics[0], Mine)


def test_vif_is_still_not_ours(tmp_path, monkeypatch, capsys):
    """pyiqa's `vif` is the wavelet-domain form: the name keeps going to pyiqa, or to nobody."""
    t, _ = _tracker(tmp_path, monkeypatch, ['vif', 'vifp'])
    assert [m.name for m in t.metrics] == ['vifp'] and 'Unknown metric vif\n' in capsys.readouterr().out
