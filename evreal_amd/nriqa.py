"""No-reference image quality on the GPU: NIQE (Mittal, Soundararajan, Bovik 2013), the `-qm niqe` of the reference's
no-reference datasets (utils/eval_metrics.py:100-156, 205-208 -> pyiqa), through evr_niqe_* (csrc/nriqa.hip).

The pristine model is a 36-vector and a 36x36 covariance.  Offline it comes from a file:
  * the published MATLAB release's (or pyiqa's cached) `niqe_modelparameters.mat`: keys mu_prisparam, cov_prisparam;
  * an `.npz` with mu, cov and source, e.g. one fitted on sharp frames by

        python -m evreal_amd.nriqa fit --out model.npz SEQ_DIR [SEQ_DIR ...]

    (estimatemodelparam.m on the sequences' images.npy frames).  Scores from a self-fitted model are NOT comparable with
    published NIQE figures.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

from . import lib as _lib

NUM_FEATURES = 36
BLOCK = 96
SHARPNESS_THRESHOLD = 0.75      # estimatemodelparam.m: blocks sharper than 0.75 x the frame's sharpest


def _as_frames(img):
    assert img.is_cuda and img.dtype == torch.float32, "NIQE takes cuda fp32 frames"
    v = img if img.dim() == 3 else img.reshape(-1, img.shape[-2], img.shape[-1])
    return v.contiguous()


def check_model(mu, cov):
    """(mu [36], cov [36,36]) as fp64 arrays; raises ValueError unless cov is symmetric positive definite."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    cov = np.asarray(cov, dtype=np.float64)
    if mu.shape != (NUM_FEATURES,) or cov.shape != (NUM_FEATURES, NUM_FEATURES):
        raise ValueError(f"NIQE model: mu {mu.shape} / cov {cov.shape}, expected (36,) / (36, 36)")
    if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(cov))):
        raise ValueError("NIQE model: non-finite values")
    if np.max(np.abs(cov - cov.T)) > 1e-12 * np.max(np.abs(cov)):
        raise ValueError("NIQE model: cov is not symmetric")
    cov = (cov + cov.T) / 2.0           # (a covariance written by MATLAB or numpy may differ from its transpose in the last bit)
    try:
        np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError("NIQE model: cov is not positive definite") from None
    return np.ascontiguousarray(mu), np.ascontiguousarray(cov)


def load_niqe_model(path):
    """-> dict(mu, cov, source, path) from a MATLAB .mat (mu_prisparam, cov_prisparam) or an .npz (mu, cov, source)."""
    if path.lower().endswith('.mat'):
        from scipy.io import loadmat
        d = loadmat(path)
        mu, cov, source = d['mu_prisparam'], d['cov_prisparam'], 'MATLAB model file ' + os.path.basename(path)
    else:
        with np.load(path, allow_pickle=False) as d:
            mu, cov = d['mu'], d['cov']
            source = str(d['source']) if 'source' in d.files else 'unknown'
    mu, cov = check_model(mu, cov)
    return dict(mu=mu, cov=cov, source=source, path=path)


def save_niqe_model(path, mu, cov, source):
    mu, cov = check_model(mu, cov)
    np.savez(path, mu=mu, cov=cov, source=np.array(source))


class NIQE:
    """NIQE scores of cuda fp32 frames [n,H,W] -> cuda fp64 [n] (NaN for a frame without a whole 96x96 block).
    `model`: a dict with mu / cov (load_niqe_model) or a path.  The workspace is kept between calls."""

    def __init__(self, model):
        _lib.require_gpu()
        self.lib = _lib.load()
        if isinstance(model, (str, os.PathLike)):
            model = load_niqe_model(os.fspath(model))
        self.mu, self.cov = check_model(model['mu'], model['cov'])
        self.source, self.path = model.get('source', 'unknown'), model.get('path')
        h = ctypes.c_void_p()
        _lib.check(self.lib.evr_niqe_create(self.mu.ctypes.data_as(ctypes.c_void_p), self.cov.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.byref(h)), 'evr_niqe_create')
        self.handle = h
        self.ws = None

    def _workspace(self, n, H, W, device):
        need = int(self.lib.evr_niqe_workspace_bytes(n, H, W))
        if self.ws is None or self.ws.numel() < need or self.ws.device != device:
            self.ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self.ws

    def __call__(self, img, clip=True, out=None):
        v = _as_frames(img)
        n, H, W = v.shape
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=v.device)
        ws = self._workspace(n, H, W, v.device)
        _lib.check(self.lib.evr_niqe_score(self.handle, _lib.ptr(v), n, H, W, 1 if clip else 0, _lib.ptr(out), _lib.ptr(ws),
                                           ws.numel(), _lib.stream_ptr()), 'evr_niqe_score')
        return out

    def features(self, img, clip=True):
        """-> (feat cuda fp64 [n, nb, 36], sharpness cuda fp64 [n, nb]); blocks in raster order."""
        v = _as_frames(img)
        n, H, W = v.shape
        nb = (H // BLOCK) * (W // BLOCK)
        feat = torch.empty((n, nb, NUM_FEATURES), dtype=torch.float64, device=v.device)
        sharp = torch.empty((n, nb), dtype=torch.float64, device=v.device)
        ws = self._workspace(n, H, W, v.device)
        _lib.check(self.lib.evr_niqe_features(self.handle, _lib.ptr(v), n, H, W, 1 if clip else 0, _lib.ptr(feat), _lib.ptr(sharp),
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'evr_niqe_features')
        return feat, sharp

    def __del__(self):
        try:
            if self.handle is not None:
                self.lib.evr_niqe_destroy(self.handle); self.handle = None
        except Exception:
            pass


_feature_handle = []


def niqe_features(img, clip=True):
    """NIQE block features of cuda fp32 frames [n,H,W] -> (feat [n, nb, 36], sharpness [n, nb]) on the device.  The
    features do not depend on a model (a placeholder one is used)."""
    if not _feature_handle:
        _feature_handle.append(NIQE(dict(mu=np.zeros(NUM_FEATURES), cov=np.eye(NUM_FEATURES), source='features only')))
    return _feature_handle[0].features(img, clip)


def nan_mean_cov(rows):
    """(column-wise NaN-ignoring mean, unbiased covariance of the NaN-free rows; NaN with fewer than 2) -- nanmean / nancov."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, NUM_FEATURES)
    cnt = (~np.isnan(rows)).sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        mu = np.where(np.isnan(rows), 0.0, rows).sum(axis=0) / cnt
    ok = rows[~np.isnan(rows).any(axis=1)]
    cov = np.cov(ok, rowvar=False) if len(ok) >= 2 else np.full((NUM_FEATURES, NUM_FEATURES), np.nan)
    return mu, cov


def fit_niqe_model(frames, clip=True, threshold=SHARPNESS_THRESHOLD, source='fit'):
    """estimatemodelparam.m: from each frame keep the blocks with sharpness > threshold x the frame's maximum, pool their
    36-vectors and take the NaN-aware mean and covariance.  frames: a cuda fp32 tensor [n,H,W] or an iterable of them (one
    batch each).  Refuses a fit with fewer than 37 complete rows.  -> dict(mu, cov, source)."""
    if isinstance(frames, torch.Tensor):
        frames = [frames]
    rows = []
    for chunk in frames:
        feat, sharp = niqe_features(chunk, clip)
        feat, sharp = feat.cpu().numpy(), sharp.cpu().numpy()
        for f, s in zip(feat, sharp):
            if len(s):
                rows.append(f[s > threshold * s.max()])
    rows = np.concatenate(rows) if rows else np.zeros((0, NUM_FEATURES))
    complete = int((~np.isnan(rows).any(axis=1)).sum())
    if complete < NUM_FEATURES + 1:
        raise ValueError(f"NIQE fit: {complete} complete block rows, at least {NUM_FEATURES + 1} are needed")
    mu, cov = check_model(*nan_mean_cov(rows))
    return dict(mu=mu, cov=cov, source=source)


def _sequence_frames(path, device, chunk=64):
    """The frames of one sequence's images.npy as the frame loop reads them (images[i][:,:,0] / 255 in fp32)."""
    imgs = np.load(os.path.join(path, 'images.npy'), mmap_mode='r')
    d255 = torch.tensor(255.0, dtype=torch.float32, device=device)
    for i in range(0, len(imgs), chunk):
        a = torch.from_numpy(np.ascontiguousarray(imgs[i:i + chunk, :, :, 0])).to(device)
        yield (a.to(torch.float32) / d255).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m evreal_amd.nriqa', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    f = sub.add_parser('fit', help="fit a pristine NIQE model on the sequences' own images.npy frames")
    f.add_argument('--out', required=True, help='output .npz (mu, cov, source)')
    f.add_argument('sequences', nargs='+', help='sequence directories holding images.npy')
    a = ap.parse_args(argv)
    _lib.require_gpu()
    seqs = [os.path.abspath(s) for s in a.sequences]
    source = 'self-fitted (estimatemodelparam, sharpness > 0.75 max) on images.npy of: ' + ', '.join(os.path.basename(s) for s in seqs)
    frames = (c for s in seqs for c in _sequence_frames(s, torch.device('cuda')))
    model = fit_niqe_model(frames, source=source)
    save_niqe_model(a.out, model['mu'], model['cov'], source)
    print(f"wrote {a.out}: {source}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
