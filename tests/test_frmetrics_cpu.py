"""PSNR / MS-SSIM without a GPU: the numpy oracle (tests/frmetrics_ref.py) against an independent float64 restatement built
from torch's conv2d / avg_pool2d, against scikit-image's SSIM at scale 1, known values and cross-check digits; the tracker's
handling of the two names; the argument checks of evr_fr_metrics (which come before any HIP call)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_json
import frmetrics_ref as FR
from thirdparty_refs import image_pairs

LARGE = ('davis346', 'davis240', 'vga', 'noise')


def _pairs():
    return [(n, i, r) for n, i, r in image_pairs() if n in LARGE]


def _textured_pair(H, W, seed):
    """Smooth texture + noise with values beyond [0, 1] and a flat patch; the image is the reference plus 6 % noise."""
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ref = 0.5 + 0.3 * np.sin(xx / (5 + seed % 5)) * np.cos(yy / 9.0) + 0.12 * rng.standard_normal((H, W))
    ref[:H // 5, :W // 6] = 0.25
    ref[H // 2, :] = 1.3
    ref[:, W // 3] = -0.2
    img = ref + 0.06 * rng.standard_normal((H, W))
    return img.astype(np.float32), ref.astype(np.float32)


def _torch_ms_ssim(img, ref, clip=True):
    """pytorch-msssim's algorithm restated with conv2d / avg_pool2d in float64 -> (score, [(S_l, CS_l)])."""
    X = torch.from_numpy(np.asarray(ref, np.float64))[None, None]
    Y = torch.from_numpy(np.asarray(img, np.float64))[None, None]
    if clip:
        X, Y = X.clamp(0, 1), Y.clamp(0, 1)
    r = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(r ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()

    def filt(a):
        return F.conv2d(F.conv2d(a, g.view(1, 1, 11, 1)), g.view(1, 1, 1, 11))

    C1, C2, per = 0.01 ** 2, 0.03 ** 2, []
    for l in range(5):
        ux, uy = filt(X), filt(Y)
        vx, vy, vxy = filt(X * X) - ux * ux, filt(Y * Y) - uy * uy, filt(X * Y) - ux * uy
        cs = (2 * vxy + C2) / (vx + vy + C2)
        s = (2 * ux * uy + C1) / (ux * ux + uy * uy + C1) * cs
        per.append((float(s.mean()), float(cs.mean())))
        if l < 4:
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    v = torch.tensor([p[1] for p in per[:4]] + [per[4][0]], dtype=torch.float64).clamp(min=0)
    w = torch.tensor(FR.W5)
    return float(torch.prod(v ** w)), per


def test_oracle_matches_the_torch_restatement():
    cases = [(n, i, r, True) for n, i, r in _pairs()]
    for (H, W), seed in (((161, 161), 1), ((625, 970), 2)):
        img, ref = _textured_pair(H, W, seed)
        cases += [(f'{H}x{W}', img, ref, True), (f'{H}x{W} unclipped', img, ref, False)]
    worst = 0.0
    for name, img, ref, clip in cases:
        got, per = FR.ms_ssim(img, ref, clip)
        want, wper = _torch_ms_ssim(img, ref, clip)
        d = max(abs(got - want), np.abs(np.array(per) - np.array(wper)).max())
        print(f'{name}: score {got:.12f}, distance to the torch restatement {d:.2e}')
        worst = max(worst, d)
        assert d <= 1e-12, (name, d)
    print(f'largest distance {worst:.2e}')


def test_scale_one_matches_scikit_image_and_psnr_the_fixture_mse():
    from oracle import metrics as OM
    rows = {r['name']: r for r in load_json('thirdparty_metrics.json')['rows']}
    for name, img, ref in _pairs():
        _, per = FR.ms_ssim(img, ref)
        s1 = per[0][0]
        d_oracle, d_fixture = abs(s1 - OM.ssim(img, ref)), abs(s1 - rows[name]['ssim'])
        print(f'{name}: S_1 {s1:.10f}, to oracle.metrics.ssim {d_oracle:.2e}, to scikit-image 0.18.3 {d_fixture:.2e}')
        assert d_oracle <= 1e-6 and d_fixture <= 1e-6, (name, d_oracle, d_fixture)
        want = 10.0 * math.log10(1.0 / (rows[name]['mse'] + 1e-8))
        assert abs(FR.psnr(img, ref) - want) <= 1e-9, (name, FR.psnr(img, ref), want)


def test_known_values():
    img, ref = _textured_pair(180, 240, 3)
    score, per = FR.ms_ssim(ref, ref)
    assert score == 1.0 and all(p == (1.0, 1.0) for p in per)
    assert abs(FR.psnr(ref, ref) - 80.0) <= 1e-12
    rng = np.random.default_rng(9)
    ref = rng.random((260, 346), dtype=np.float32)
    score, per = FR.ms_ssim(np.float32(1) - ref, ref)
    assert score == 0.0
    assert all(-0.999 < p[1] < -0.4 for p in per[:4]), per       # far from 0: the clamp, not a rounding, gives the zero
    assert FR.level_sizes(260, 346) == [(260, 346), (130, 173), (65, 87), (33, 44), (17, 22)]
    assert [s[0] for s in FR.level_sizes(625, 970)] == [625, 313, 157, 79, 40]
    assert [s[0] for s in FR.level_sizes(161, 161)] == [161, 81, 41, 21, 11]
    with pytest.raises(ValueError):
        FR.ms_ssim(np.zeros((160, 400), np.float32), np.zeros((160, 400), np.float32))


def test_cross_check_digits():
    want = {'davis346': 0.904978729879, 'davis240': 0.904073890246, 'vga': 0.904854702187, 'noise': 0.075936766249}
    for name, img, ref in _pairs():
        assert abs(FR.ms_ssim(img, ref)[0] - want[name]) <= 1e-9, (name, FR.ms_ssim(img, ref)[0])
        if name == 'davis346':
            assert abs(FR.psnr(img, ref) - 22.011401) <= 5e-7
    row = FR.scales_row(FR.ms_ssim(*_pairs()[0][1:])[1])
    assert FR.combine(row) == FR.ms_ssim(*_pairs()[0][1:])[0]


# ---- tracker -----------------------------------------------------------------------------------------------------------------------
def _tracker(tmp_path, **kw):
    from evreal_amd.eval_metrics import EvalMetricsTracker
    return EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['psnr', 'ms_ssim'], **kw)


def test_tracker_knows_psnr_and_ms_ssim(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.delenv(em.FR_METRICS_ENV, raising=False)
    t = _tracker(tmp_path, has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['psnr', 'ms_ssim']
    assert all(isinstance(m, em.QueuedGpuMetric) and m.no_ref is False for m in t.metrics)
    assert 'Unknown metric' not in capsys.readouterr().out
    assert t.wants_precomputed() == ['psnr', 'ms_ssim']
    assert os.path.exists(tmp_path / 'out' / 'psnr.txt') and os.path.exists(tmp_path / 'out' / 'ms_ssim.txt')
    assert t.get_mean_scores() == {'psnr': -1, 'ms_ssim': -1}
    t = _tracker(tmp_path, has_reference_frames=True, hist_eq='global')
    assert t.wants_precomputed() == []
    t = _tracker(tmp_path, has_reference_frames=False)
    assert t.metrics == [] and t.wants_precomputed() == []


def test_default_metric_list_is_unchanged(tmp_path, monkeypatch):
    from evreal_amd import eval_metrics as em
    monkeypatch.setattr(em.EvalMetricsTracker, '_lpips_model', classmethod(lambda cls: object()))
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['mse', 'ssim', 'lpips']


def test_opt_out_sends_the_names_down_the_old_path(tmp_path, monkeypatch, capsys):
    from evreal_amd import eval_metrics as em
    monkeypatch.setenv(em.FR_METRICS_ENV, '0')
    if {'psnr', 'ms_ssim'} & set(em.pyiqa_metric_factory().list_of_metrics):
        pytest.skip("pyiqa is installed: the names go to pyiqa")
    t = _tracker(tmp_path, has_reference_frames=True)
    out = capsys.readouterr().out
    assert t.metrics == [] and 'Unknown metric psnr' in out and 'Unknown metric ms_ssim' in out


def test_full_ref_metrics_object_needs_no_gpu_to_exist():
    from evreal_amd.prepost import FullRefMetrics
    m = FullRefMetrics()
    assert m.ws is None and m.MIN_SIDE == 161
    assert m.too_small(161, 161) is None and m.too_small(260, 346) is None
    assert '161' in m.too_small(160, 346) and '96x128' in m.too_small(96, 128)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from evreal_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_argument_validation_without_gpu(lib):
    import ctypes
    assert lib.evr_fr_metrics_workspace_bytes(2, 260, 346) > 0
    assert lib.evr_fr_metrics_workspace_bytes(-1, 260, 346) == 0 and lib.evr_fr_metrics_workspace_bytes(2, 0, 346) == 0
    # five pooled fp64 levels of both images + the per-tile partials
    lv = FR.level_sizes(260, 346)[1:]
    assert lib.evr_fr_metrics_workspace_bytes(2, 260, 346) >= 2 * 2 * 8 * sum(h * w for h, w in lv)
    assert lib.evr_fr_metrics_workspace_bytes(2, 96, 128) < 2 * 96 * 128      # psnr alone: partials only
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # a non-null HOST address: every call below must return before it is used
    call = lambda img, ref, n, H, W, which, out: lib.evr_fr_metrics(img, ref, n, H, W, which, 1, out, None, p, 1 << 30, None)
    assert call(p, p, -1, 260, 346, 3, p) == -1 and b'evr_fr_metrics' in lib.evr_last_error()
    assert call(p, p, 1, 0, 346, 3, p) == -1
    assert call(None, p, 1, 260, 346, 3, p) == -1 and b'null' in lib.evr_last_error()
    assert call(p, None, 1, 260, 346, 1, p) == -1
    assert call(p, p, 1, 260, 346, 1, None) == -1
    assert call(p, p, 1, 260, 346, 0, p) == -1 and call(p, p, 1, 260, 346, 4, p) == -1
    assert call(p, p, 1, 160, 346, 2, p) == -1 and b'161' in lib.evr_last_error()
    assert call(p, p, 1, 346, 160, 3, p) == -1 and b'161' in lib.evr_last_error()
    assert call(p, p, 0, 160, 346, 3, p) == -1              # the size limit does not wait for a frame
    assert call(p, p, 0, 160, 346, 1, p) == 0               # psnr alone takes any size; n == 0 launches nothing
    assert lib.evr_fr_metrics(p, p, 1, 260, 346, 3, 1, p, None, None, 0, None) == -3      # workspace


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'evreal_hip.h')).read()
    for name in ('evr_fr_metrics_workspace_bytes', 'evr_fr_metrics'):
        assert name + '(' in hdr, name
