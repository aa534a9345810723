"""No-reference image quality on the GPU: NIQE (Mittal, Soundararajan, Bovik 2013), BRISQUE (Mittal, Moorthy, Bovik
2012) and PIQE (Venkatanath et al. 2015), the `-qm niqe` / `-qm brisque` / `-qm piqe` of the reference's no-reference
datasets (utils/eval_metrics.py:100-156, 205-208 -> pyiqa), through evr_niqe_*, evr_brisque_* and evr_piqe_*
(csrc/nriqa.hip).  PIQE is training-free: it needs no file.

The pristine model is a 36-vector and a 36x36 covariance.  Offline it comes from a file:
  * the published MATLAB release's (or pyiqa's cached) `niqe_modelparameters.mat`: keys mu_prisparam, cov_prisparam;
  * an `.npz` with mu, cov and source, e.g. one fitted on sharp frames by

        python -m evreal_amd.nriqa fit --out model.npz SEQ_DIR [SEQ_DIR ...]

    (estimatemodelparam.m on the sequences' images.npy frames).  Scores from a self-fitted model are NOT comparable with
    published NIQE figures.

The BRISQUE model is an RBF support-vector regression plus the svm-scale ranges of its 36 features.  It comes from:
  * a libsvm text model (e.g. the MATLAB release's `allmodel`) with its svm-scale range file (`allrange`), or
  * an `.npz` with sv, coef, gamma, rho, fmin, fmax, lower, upper and source, e.g. one converted by

        python -m evreal_amd.nriqa brisque-convert --model allmodel --range allrange --out brisque_model.npz

pyiqa's `brisque_svm_weights.pth` holds the support vectors but not the feature ranges (those live in pyiqa's source), so
that file alone is refused.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

from . import lib as _lib
from .prepost import Workspace

NUM_FEATURES = 36
BLOCK = 96
SHARPNESS_THRESHOLD = 0.75      # estimatemodelparam.m: blocks sharper than 0.75 x the frame's sharpest


def _as_frames(img):
    assert img.is_cuda and img.dtype == torch.float32, "NIQE takes cuda fp32 frames"
    v = img if img.dim() == 3 else img.reshape(-1, img.shape[-2], img.shape[-1])
    return v.contiguous()


def _new(v, *shape, dtype=torch.float64):
    """An output of one entry [*shape] per frame of v."""
    return torch.empty((v.shape[0],) + shape, dtype=dtype, device=v.device)


class NoRefMetric(Workspace):
    """What the no-reference metrics share: the library, the handle where the metric has one (`_destroy` names the entry
    point that frees it), the workspace kept between calls, and one checked call of a named entry point:
    entry([handle,] frames, n, H, W, clip, *outs, workspace, bytes, stream)."""
    _score = None               # the scoring entry point's name
    _destroy = None
    handle = None

    def __init__(self):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.ws = None

    def _run(self, entry, v, clip, *outs):
        n, H, W = v.shape
        ws = self._workspace(n, H, W, v.device)
        head = (self.handle,) if self._destroy else ()
        _lib.check(getattr(self.lib, entry)(*head, _lib.ptr(v), n, H, W, 1 if clip else 0, *map(_lib.ptr, outs), _lib.ptr(ws),
                                            ws.numel(), _lib.stream_ptr()), entry)
        return outs[0] if len(outs) == 1 else outs

    def __call__(self, img, clip=True, out=None):
        v = _as_frames(img)
        return self._run(self._score, v, clip, _new(v) if out is None else out)

    def __del__(self):
        try:
            if self._destroy and self.handle is not None:
                getattr(self.lib, self._destroy)(self.handle); self.handle = None
        except Exception:
            pass


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


class NIQE(NoRefMetric):
    """NIQE scores of cuda fp32 frames [n,H,W] -> cuda fp64 [n] (NaN for a frame without a whole 96x96 block).
    `model`: a dict with mu / cov (load_niqe_model) or a path.  The workspace is kept between calls."""
    _workspace_bytes, _score, _destroy = 'evr_niqe_workspace_bytes', 'evr_niqe_score', 'evr_niqe_destroy'

    def __init__(self, model):
        super().__init__()
        if isinstance(model, (str, os.PathLike)):
            model = load_niqe_model(os.fspath(model))
        self.mu, self.cov = check_model(model['mu'], model['cov'])
        self.source, self.path = model.get('source', 'unknown'), model.get('path')
        h = ctypes.c_void_p()
        _lib.check(self.lib.evr_niqe_create(self.mu.ctypes.data_as(ctypes.c_void_p), self.cov.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.byref(h)), 'evr_niqe_create')
        self.handle = h

    def features(self, img, clip=True):
        """-> (feat cuda fp64 [n, nb, 36], sharpness cuda fp64 [n, nb]); blocks in raster order."""
        v = _as_frames(img)
        nb = (v.shape[1] // BLOCK) * (v.shape[2] // BLOCK)
        return self._run('evr_niqe_features', v, clip, _new(v, nb, NUM_FEATURES), _new(v, nb))


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


BRISQUE_SVM_TYPES = ('epsilon_svr', 'nu_svr')
# libsvm model header lines a BRISQUE model may carry without needing them
_LIBSVM_IGNORED = ('nr_class', 'total_sv', 'probA', 'probB', 'label', 'nr_sv', 'degree', 'coef0')


def check_brisque_model(sv, coef, gamma, rho, fmin, fmax, lower, upper):
    """-> dict of fp64 arrays / floats; raises ValueError unless the model is one evr_brisque_create accepts (nsv = 0: a
    features-only model)."""
    sv = np.ascontiguousarray(np.asarray(sv, dtype=np.float64).reshape(-1, NUM_FEATURES))
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(-1))
    fmin = np.ascontiguousarray(np.asarray(fmin, dtype=np.float64).reshape(-1))
    fmax = np.ascontiguousarray(np.asarray(fmax, dtype=np.float64).reshape(-1))
    gamma, rho, lower, upper = float(gamma), float(rho), float(lower), float(upper)
    if sv.shape[0] != coef.shape[0]:
        raise ValueError(f"BRISQUE model: {sv.shape[0]} support vectors but {coef.shape[0]} coefficients")
    if fmin.shape != (NUM_FEATURES,) or fmax.shape != (NUM_FEATURES,):
        raise ValueError(f"BRISQUE model: feature ranges {fmin.shape} / {fmax.shape}, expected (36,) / (36,)")
    if not all(np.all(np.isfinite(a)) for a in (sv, coef, fmin, fmax, [gamma, rho, lower, upper])):
        raise ValueError("BRISQUE model: non-finite values")
    if not lower < upper:
        raise ValueError(f"BRISQUE model: scaling interval lower {lower} >= upper {upper}")
    if np.any(fmin > fmax):
        raise ValueError(f"BRISQUE model: feature {int(np.argmax(fmin > fmax)) + 1} has min > max")
    return dict(sv=sv, coef=coef, gamma=gamma, rho=rho, fmin=fmin, fmax=fmax, lower=lower, upper=upper)


def _libsvm_index(tok, what, path):
    i, _, v = tok.partition(':')
    try:
        i, v = int(i), float(v)
    except ValueError:
        raise ValueError(f"{path}: cannot read '{tok}' in {what}") from None
    if not 1 <= i <= NUM_FEATURES:
        raise ValueError(f"{path}: feature index {i} in {what} is outside 1..{NUM_FEATURES}")
    return i, v


def read_libsvm_model(path):
    """A libsvm text model (svm-train's output) of an epsilon- or nu-SVR with an RBF kernel over at most 36 features ->
    (sv [nsv, 36], coef [nsv], gamma, rho).  Sparse `index:value` lines; a missing index is 0."""
    head, sv, coef = {}, [], []
    with open(path) as f:
        lines = iter(f.read().splitlines())
    for line in lines:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'SV':
            break
        if tok[0] in ('svm_type', 'kernel_type', 'gamma', 'rho'):
            head[tok[0]] = tok[1:]
        elif tok[0] not in _LIBSVM_IGNORED:
            raise ValueError(f"{path}: unknown libsvm model line '{line.strip()}'")
    else:
        raise ValueError(f"{path}: no SV section (not a libsvm model)")
    svm_type = (head.get('svm_type') or ['?'])[0]
    if svm_type not in BRISQUE_SVM_TYPES:
        raise ValueError(f"{path}: svm_type {svm_type}, BRISQUE needs a regression ({' or '.join(BRISQUE_SVM_TYPES)})")
    kernel = (head.get('kernel_type') or ['?'])[0]
    if kernel != 'rbf':
        raise ValueError(f"{path}: kernel_type {kernel}, only rbf is supported")
    if 'gamma' not in head or 'rho' not in head or len(head['rho']) != 1:
        raise ValueError(f"{path}: gamma and one rho are required")
    for n, line in enumerate(lines):
        tok = line.split()
        if not tok:
            continue
        row = np.zeros(NUM_FEATURES)
        for t in tok[1:]:
            i, v = _libsvm_index(t, f'support vector {n + 1}', path)
            row[i - 1] = v
        coef.append(float(tok[0]))
        sv.append(row)
    return np.array(sv).reshape(-1, NUM_FEATURES), np.array(coef), float(head['gamma'][0]), float(head['rho'][0])


def read_svm_scale_range(path):
    """An svm-scale range file (`svm-scale -s`) with an x section over all 36 features -> (fmin [36], fmax [36], lower,
    upper).  A y section (target scaling) is refused: BRISQUE's release scales features only."""
    with open(path) as f:
        lines = [l.split() for l in f.read().splitlines() if l.strip()]
    if not lines or lines[0][0] == 'y':
        raise ValueError(f"{path}: a range file with a y section is not supported" if lines else f"{path}: empty range file")
    if lines[0] != ['x'] or len(lines) < 2 or len(lines[1]) != 2:
        raise ValueError(f"{path}: not an svm-scale range file (expected 'x', then 'lower upper')")
    lower, upper = float(lines[1][0]), float(lines[1][1])
    fmin, fmax = np.full(NUM_FEATURES, np.nan), np.full(NUM_FEATURES, np.nan)
    for tok in lines[2:]:
        if tok[0] == 'y':
            raise ValueError(f"{path}: a range file with a y section is not supported")
        if len(tok) != 3:
            raise ValueError(f"{path}: cannot read range line '{' '.join(tok)}'")
        i = int(tok[0])
        if not 1 <= i <= NUM_FEATURES:
            raise ValueError(f"{path}: feature index {i} is outside 1..{NUM_FEATURES}")
        fmin[i - 1], fmax[i - 1] = float(tok[1]), float(tok[2])
    missing = [k + 1 for k in range(NUM_FEATURES) if np.isnan(fmin[k])]
    if missing:
        raise ValueError(f"{path}: no range for feature(s) {missing}; all 36 are needed")
    return fmin, fmax, lower, upper


def load_brisque_model(path, range_path=None):
    """-> dict(sv, coef, gamma, rho, fmin, fmax, lower, upper, source, path) from an .npz, or from a libsvm text model and
    its svm-scale range file (`range_path`, default `allrange` beside the model)."""
    if path.lower().endswith('.pth'):
        raise ValueError(f"{path}: pyiqa's BRISQUE weights hold no feature ranges (they live in pyiqa's source); give a "
                         "libsvm model with its range file, or an .npz")
    if path.lower().endswith('.npz'):
        with np.load(path, allow_pickle=False) as d:
            m = check_brisque_model(*(d[k] for k in ('sv', 'coef', 'gamma', 'rho', 'fmin', 'fmax', 'lower', 'upper')))
            source = str(d['source']) if 'source' in d.files else 'unknown'
    else:
        if range_path is None:
            range_path = os.path.join(os.path.dirname(path), 'allrange')
        sv, coef, gamma, rho = read_libsvm_model(path)
        fmin, fmax, lower, upper = read_svm_scale_range(range_path)
        m = check_brisque_model(sv, coef, gamma, rho, fmin, fmax, lower, upper)
        source = f'libsvm model {os.path.basename(path)} + range {os.path.basename(range_path)}'
    return dict(m, source=source, path=path)


def save_brisque_model(path, sv, coef, gamma, rho, fmin, fmax, lower, upper, source):
    m = check_brisque_model(sv, coef, gamma, rho, fmin, fmax, lower, upper)
    np.savez(path, **m, source=np.array(source))


class BRISQUE(NoRefMetric):
    """BRISQUE scores of cuda fp32 frames [n,H,W] -> cuda fp64 [n] (NaN for a frame with a NaN feature, e.g. a flat one).
    `model`: a dict as load_brisque_model returns, or a path.  A model without support vectors gives features only.  The
    workspace is kept between calls."""
    _workspace_bytes, _score, _destroy = 'evr_brisque_workspace_bytes', 'evr_brisque_score', 'evr_brisque_destroy'

    def __init__(self, model):
        super().__init__()
        if isinstance(model, (str, os.PathLike)):
            model = load_brisque_model(os.fspath(model))
        self.model = check_brisque_model(*(model[k] for k in ('sv', 'coef', 'gamma', 'rho', 'fmin', 'fmax', 'lower', 'upper')))
        self.source, self.path = model.get('source', 'unknown'), model.get('path')
        m = self.model
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        h = ctypes.c_void_p()
        _lib.check(self.lib.evr_brisque_create(vp(m['sv']), vp(m['coef']), len(m['coef']), m['gamma'], m['rho'], vp(m['fmin']),
                                               vp(m['fmax']), m['lower'], m['upper'], ctypes.byref(h)), 'evr_brisque_create')
        self.handle = h

    def features(self, img, clip=True):
        """-> cuda fp64 [n, 36]: the 18 full-size features, then the 18 half-size ones (unscaled)."""
        v = _as_frames(img)
        return self._run('evr_brisque_features', v, clip, _new(v, NUM_FEATURES))


_brisque_feature_handle = []


def brisque_features(img, clip=True):
    """BRISQUE features of cuda fp32 frames [n,H,W] -> [n, 36] on the device (a features-only handle)."""
    if not _brisque_feature_handle:
        _brisque_feature_handle.append(BRISQUE(dict(sv=np.zeros((0, NUM_FEATURES)), coef=np.zeros(0), gamma=1.0, rho=0.0,
                                                    fmin=np.zeros(NUM_FEATURES), fmax=np.ones(NUM_FEATURES), lower=-1.0,
                                                    upper=1.0, source='features only')))
    return _brisque_feature_handle[0].features(img, clip)


PIQE_BLOCK = 16
PIQE_ACTIVE, PIQE_WHSA, PIQE_WNC = 1, 2, 4      # the bits of a block's flag byte


class PIQE(NoRefMetric):
    """PIQE scores of cuda fp32 frames [n,H,W] -> cuda fp64 [n] (100 for a frame without an active block, e.g. a constant
    one).  No model, hence no handle: the metric is training-free.  The workspace is kept between calls."""
    _workspace_bytes, _score = 'evr_piqe_workspace_bytes', 'evr_piqe_score'

    def blocks(self, img, clip=True):
        """-> (var cuda fp64 [n, ceil(H/16), ceil(W/16)], flags cuda uint8 of the same shape: PIQE_ACTIVE | PIQE_WHSA |
        PIQE_WNC).  MATLAB's activityMask / noticeableArtifactsMask / noiseMask are these bits spread over 16x16 pixels."""
        v = _as_frames(img)
        shape = (-(-v.shape[1] // PIQE_BLOCK), -(-v.shape[2] // PIQE_BLOCK))
        return self._run('evr_piqe_blocks', v, clip, _new(v, *shape), _new(v, *shape, dtype=torch.uint8))


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
    c = sub.add_parser('brisque-convert', help='convert a libsvm BRISQUE model and its svm-scale range file to an .npz')
    c.add_argument('--model', required=True, help='libsvm text model (e.g. allmodel)')
    c.add_argument('--range', default=None, help="svm-scale range file (default: allrange beside the model)")
    c.add_argument('--out', required=True, help='output .npz')
    a = ap.parse_args(argv)
    if a.cmd == 'brisque-convert':
        m = load_brisque_model(a.model, a.range)
        save_brisque_model(a.out, *(m[k] for k in ('sv', 'coef', 'gamma', 'rho', 'fmin', 'fmax', 'lower', 'upper')), m['source'])
        print(f"wrote {a.out}: {len(m['coef'])} support vectors, {m['source']}")
        return 0
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
