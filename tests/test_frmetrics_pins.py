"""PSNR / MS-SSIM pinned to pyiqa (the reference's `-qm psnr ms_ssim`, utils/eval_metrics.py:110-147) where pyiqa is
importable: the oracle (CPU) and the kernels (`-m gpu`) against pyiqa.create_metric('psnr') / ('ms_ssim') called as the
reference calls them (a gray frame replicated to three channels, eval_utils.py:46-54).  Skips where pyiqa is missing.
A convention it contradicts (a luma conversion, a scaling to 255, a rounding, another eps) is fixed in tests/frmetrics_ref.py
and csrc/frmetrics.hip together.

Bounds: pyiqa computes in float32.  Its mse carries a relative error of about 1e-6 (fp32 squares, fp32 summation in
blocks), which is 4e-6 dB: 1e-4 dB is held.  Its SSIM moments carry about 11 * 6e-8 each, over denominators that are
typically 1e-2 or more on textured frames: the map means move by about 1e-5; 1e-4 absolute is held."""
import numpy as np
import pytest

import frmetrics_ref as FR

PSNR_TOL_DB, MS_SSIM_TOL = 1e-4, 1e-4


def _setup():
    pyiqa = pytest.importorskip('pyiqa')
    import torch
    return torch, pyiqa.create_metric('psnr', device='cpu'), pyiqa.create_metric('ms_ssim', device='cpu')


def _pairs():
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:260, 0:346].astype(np.float64)
    out = []
    for k in range(3):
        ref = np.clip(0.5 + 0.3 * np.sin(xx / (6.0 + k)) * np.cos(yy / 9.0) + 0.1 * rng.standard_normal((260, 346)), 0, 1)
        img = np.clip(ref + 0.05 * (k + 1) * rng.standard_normal((260, 346)), 0, 1)
        out.append((img.astype(np.float32), ref.astype(np.float32)))
    return out


def _pyiqa(torch, metric, img, ref):
    t = lambda v: torch.from_numpy(v)[None].repeat(3, 1, 1)[None]
    return float(metric(t(img), t(ref)).squeeze())


def test_oracle_matches_pyiqa():
    torch, psnr, ms = _setup()
    for img, ref in _pairs():
        assert abs(FR.psnr(img, ref) - _pyiqa(torch, psnr, img, ref)) <= PSNR_TOL_DB
        assert abs(FR.ms_ssim(img, ref)[0] - _pyiqa(torch, ms, img, ref)) <= MS_SSIM_TOL


@pytest.mark.gpu
def test_kernels_match_pyiqa():
    torch, psnr, ms = _setup()
    from evreal_amd.prepost import FullRefMetrics
    pairs = _pairs()
    got = FullRefMetrics()(torch.from_numpy(np.stack([p[0] for p in pairs])).cuda(),
                           torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()).cpu().numpy()
    for g, (img, ref) in zip(got, pairs):
        assert abs(g[0] - _pyiqa(torch, psnr, img, ref)) <= PSNR_TOL_DB
        assert abs(g[1] - _pyiqa(torch, ms, img, ref)) <= MS_SSIM_TOL
