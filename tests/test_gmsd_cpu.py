"""GMSD without a GPU: the numpy oracle (tests/gmsd_ref.py) against facts independent of it -- a composition of torch's conv2d
and std in float64, scipy's correlate, digits computed by a separate restatement of the five steps -- and the tracker's,
the Python class's and the C entry's handling of the name, the shape and the arguments."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmsd_ref as G
from thirdparty_refs import image_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(4, 4), (5, 7), (97, 131), (260, 346)]
# scores of image_pairs(), from a separate restatement of the five steps (other summation orders move them by < 1e-12)
DIGITS = {'davis346': 0.078025991552, 'davis240': 0.075607922765, 'vga': 0.078042191307, 'odd': 0.074945364337,
          'noise': 0.206525682963}


def _pair(H, W, seed):
    rng = np.random.default_rng([seed, H, W])
    return rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32)


def _torch_gradients(v):
    """-> (pooled, gx, gy, magnitude) from conv2d in float64."""
    u = torch.from_numpy(G.luminance(v))[None, None]
    p = F.conv2d(u, torch.full((1, 1, 2, 2), 0.25, dtype=torch.float64), stride=2)
    kx = torch.tensor([[1., 0., -1.]] * 3, dtype=torch.float64)[None, None] / 3.0
    g = F.conv2d(p, torch.cat([kx, kx.transpose(2, 3)]), padding=1)
    return p[0, 0], g[0, 0], g[0, 1], torch.sqrt((g ** 2).sum(1) + 1e-12)[0]


def _torch_gmsd(img, ref):
    ga, gb = _torch_gradients(img)[3], _torch_gradients(ref)[3]
    q = (2 * ga * gb + 170.0) / (ga ** 2 + gb ** 2 + 170.0)
    return q.numpy(), float(torch.std(q))


@pytest.mark.parametrize('H,W', SIZES)
def test_oracle_equals_a_composition_of_conv2d_and_std(H, W):
    img, ref = _pair(H, W, 1)
    q, s = _torch_gmsd(img, ref)
    got = G.gms_map(img, ref)
    assert got.shape == (H // 2, W // 2) and got.dtype == np.float64
    assert np.abs(got - q).max() <= 1e-12
    assert abs(G.gmsd(img, ref) - s) <= 1e-12
    assert abs(G.mean_gms(img, ref) - q.mean()) <= 1e-12
    assert 0.0 < got.min() and got.max() <= 1.0


@pytest.mark.parametrize('H,W', SIZES)
def test_gradients_equal_scipy_correlate_with_constant_padding(H, W):
    from scipy.ndimage import correlate
    img, _ = _pair(H, W, 2)
    p, gx, gy, mag = _torch_gradients(img)
    p = p.numpy()
    assert np.array_equal(p, G.pool(G.luminance(img)))
    kx = np.array([[1., 0., -1.]] * 3) / 3.0
    sx, sy = correlate(p, kx, mode='constant', cval=0.0), correlate(p, kx.T, mode='constant', cval=0.0)
    assert np.abs(sx - gx.numpy()).max() <= 1e-12 and np.abs(sy - gy.numpy()).max() <= 1e-12
    assert np.abs(np.sqrt(sx * sx + sy * sy + 1e-12) - G.gradient_magnitude(p)).max() <= 1e-12


def test_oracle_reproduces_the_recorded_digits():
    pairs = {name: (img, ref) for name, img, ref in image_pairs()}
    for name, want in DIGITS.items():
        got = G.gmsd(*pairs[name])
        assert abs(got - want) <= 1e-9, (name, got, want)
    flat = pairs['constant']
    assert G.gmsd(*flat) == 0.0 and G.mean_gms(*flat) == 1.0
    # the rounding of step 1 shows in the fourth digit: the unrounded luminance gives 0.078077 on davis346
    img, ref = pairs['davis346']
    raw = lambda v: G.gradient_magnitude(G.pool(255.0 * v.astype(np.float64)))
    ga, gb = raw(img), raw(ref)
    unrounded = np.std(((2.0 * ga) * gb + 170.0) / ((ga * ga + gb * gb) + 170.0), ddof=1)
    assert abs(unrounded - 0.078077) <= 1e-6 and abs(G.gmsd(img, ref) - 0.078026) <= 1e-6


def test_symmetry_identity_and_the_moment_form():
    for name, img, ref in image_pairs():
        a, b = G.gms_map(img, ref), G.gms_map(ref, img)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name
        assert np.float64(G.gmsd(img, ref)).view(np.uint64) == np.float64(G.gmsd(ref, img)).view(np.uint64), name
        assert G.gmsd(ref, ref) == 0.0 and G.mean_gms(ref, ref) == 1.0, name
    # the kernel's form -- the moments of d = 1 - q -- on a pair that differs in one pixel: the two-pass value
    _, ref = _pair(260, 346, 3)
    ref = (np.rint(ref * 255) / 255).astype(np.float32)
    img = ref.copy()
    img[100, 100] = np.float32(1.0) - img[100, 100]
    d = 1.0 - G.gms_map(img, ref)
    N = d.size
    moments = np.sqrt(max((np.sum(d * d) - np.sum(d) ** 2 / N) / (N - 1), 0.0))
    two_pass = G.gmsd(img, ref)
    assert two_pass > 0 and abs(moments - two_pass) <= 1e-9 * two_pass      # (few non-zero d: no cancellation)


def test_the_dropped_odd_row_and_column_do_not_reach_the_score():
    img, ref = _pair(97, 131, 4)
    a = G.gms_map(img, ref)
    img2, ref2 = img.copy(), ref.copy()
    img2[-1, :] = 1.0; ref2[-1, :] = 0.0; img2[:, -1] = 0.0; ref2[:, -1] = 1.0
    b = G.gms_map(img2, ref2)
    assert np.array_equal(a, b) and G.gmsd(img, ref) == G.gmsd(img2, ref2)
    assert np.array_equal(a, G.gms_map(img[:96, :130], ref[:96, :130]))


def test_the_zero_padding_reaches_the_score():
    """A frame with a bright border, against its interior alone: the border pixels of the pooled plane see the zeros."""
    H, W = 40, 56
    img, ref = np.full((H, W), 0.9, np.float32), np.full((H, W), 0.8, np.float32)
    rng = np.random.default_rng(5)
    img[8:-8, 8:-8] = rng.random((H - 16, W - 16), dtype=np.float32)
    ref[8:-8, 8:-8] = rng.random((H - 16, W - 16), dtype=np.float32)
    q = G.gms_map(img, ref)
    assert q[0, 0] < 1.0 and q[0, W // 4] < 1.0          # corner and edge: gradients against the padding, unequal in img and ref
    assert q[2, 2] == 1.0                                # flat, away from the edge: both gradients vanish
    assert abs(G.gmsd(img, ref) - G.gmsd(img[8:-8, 8:-8], ref[8:-8, 8:-8])) > 1e-3


def test_one_pooled_pixel_is_nan_and_a_side_of_one_raises():
    img, ref = _pair(3, 3, 6)
    assert G.gms_map(img, ref).shape == (1, 1) and np.isnan(G.gmsd(img, ref))
    assert np.isnan(float(torch.std(torch.tensor([0.5], dtype=torch.float64))))
    for shape in ((1, 8), (8, 1), (1, 1)):
        with pytest.raises(ValueError, match='%dx%d' % shape):
            G.gmsd(np.zeros(shape, np.float32), np.zeros(shape, np.float32))


def test_clip_off_keeps_the_rounding():
    v = np.array([[-0.2, 0.5, 1.3, 0.25]], np.float32)
    assert np.array_equal(G.luminance(v, clip=True), [[0.0, 128.0, 255.0, 64.0]])      # 127.5 -> 128, 63.75 -> 64
    assert np.array_equal(G.luminance(v, clip=False), [[-51.0, 128.0, 332.0, 64.0]])
    assert np.array_equal(G.luminance(np.array([[2.5 / 255, 3.5 / 255]], np.float32)), [[2.0, 4.0]])   # half to even


# ---- tracker -----------------------------------------------------------------------------------------------------------------------
def _tracker(tmp_path, **kw):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    return EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['gmsd'], **kw)


def test_tracker_knows_gmsd(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.delenv('EVREAL_GPU_GMSD', raising=False)
    t = _tracker(tmp_path, has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['gmsd']
    assert isinstance(t.metrics[0], em.QueuedGpuMetric) and t.metrics[0].no_ref is False
    assert 'Unknown metric' not in capsys.readouterr().out
    assert t.wants_precomputed() == ['gmsd']
    assert os.path.exists(tmp_path / 'out' / 'gmsd.txt')
    assert t.get_mean_scores() == {'gmsd': -1}
    t = _tracker(tmp_path, has_reference_frames=True, hist_eq='global')
    assert [m.name for m in t.metrics] == ['gmsd'] and t.wants_precomputed() == []
    t = _tracker(tmp_path, has_reference_frames=False)
    assert t.metrics == [] and t.wants_precomputed() == []


def test_gmsd_sits_after_the_user_registry(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em

    class Mine(em.BaseMetric):
        def __init__(self):
            super().__init__('gmsd')

    monkeypatch.setitem(em._REGISTRY, 'gmsd', Mine)
    t = _tracker(tmp_path, has_reference_frames=True)
    assert isinstance(t.metrics[0], Mine)


def test_opt_out_sends_the_name_down_the_old_path(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.setenv('EVREAL_GPU_GMSD', '0')
    monkeypatch.setattr(em, '_pyiqa_factory', SimpleNamespace(list_of_metrics=[]))     # pyiqa not installed
    t = _tracker(tmp_path, has_reference_frames=True)
    assert t.metrics == [] and 'Unknown metric gmsd' in capsys.readouterr().out


def test_default_metric_list_is_unchanged(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    monkeypatch.setattr(em.EvalMetricsTracker, '_lpips_model', classmethod(lambda cls: object()))
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['mse', 'ssim', 'lpips']


def test_gmsd_object_needs_no_gpu_to_exist():
    from evreal_amd.prepost import GMSD
    m = GMSD()
    assert m.ws is None and m.lib is None
    assert m.too_small(2, 2) is None and m.too_small(260, 346) is None
    assert '1x346' in m.too_small(1, 346) and '260x1' in m.too_small(260, 1)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from evreal_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_argument_validation_without_gpu(lib):
    import ctypes
    assert lib.evr_gmsd_workspace_bytes(-1, 260, 346) == 0 and lib.evr_gmsd_workspace_bytes(2, 1, 346) == 0
    assert lib.evr_gmsd_workspace_bytes(2, 346, 1) == 0
    one, two = lib.evr_gmsd_workspace_bytes(1, 260, 346), lib.evr_gmsd_workspace_bytes(2, 260, 346)
    assert 16 <= two - one < 2 * 260 * 346          # a pair of doubles per tile, far below the frames themselves
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)           # a non-null HOST address: every call below must return before it is used
    call = lambda img, ref, n, H, W, out: lib.evr_gmsd(img, ref, n, H, W, 1, out, None, p, 1 << 30, None)
    assert call(p, p, -1, 260, 346, p) == -1 and b'evr_gmsd' in lib.evr_last_error()
    assert call(p, p, 1, 0, 346, p) == -1
    assert call(p, p, 1, 1, 346, p) == -1 and b'1 x 346' in lib.evr_last_error()
    assert call(p, p, 1, 260, 1, p) == -1 and b'260 x 1' in lib.evr_last_error()
    assert call(p, p, 0, 1, 346, p) == -1           # the size limit does not wait for a frame
    assert call(p, p, 0, 260, 346, p) == 0          # n == 0 launches nothing
    assert call(None, p, 1, 260, 346, p) == -1 and b'null' in lib.evr_last_error()
    assert call(p, None, 1, 260, 346, p) == -1 and call(p, p, 1, 260, 346, None) == -1
    assert lib.evr_gmsd(p, p, 1, 260, 346, 1, p, None, None, 0, None) == -3       # workspace
    assert lib.evr_gmsd(p, p, 1, 260, 346, 1, p, None, p, one - 1, None) == -3
    assert lib.evr_version() == 1005


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'evreal_hip.h')).read()
    for name in ('evr_gmsd_workspace_bytes', 'evr_gmsd'):
        assert name + '(' in hdr, name


def test_a_side_of_one_is_refused_by_shape_with_one_line(tmp_path, capsys):
    """Decided from the shape, before any launch: no GPU is needed to see it."""
    t = _tracker(tmp_path, has_reference_frames=True)
    idx = list(range(6))
    for k in (0, 3):
        t.update_batch(idx[k:k + 3], torch.zeros((3, 1, 8)), torch.zeros((3, 1, 8)), [0.01 * i for i in idx[k:k + 3]], None)
    t.finalize(idx[-1])
    out = capsys.readouterr().out
    assert out.count('Exception in metric gmsd: ') == 1 and '1x8' in out
    assert open(tmp_path / 'out' / 'gmsd.txt').read() == ''
    assert t.get_mean_scores() == {'gmsd': -1} and t.get_num_quan_evaluations() == 6
