"""EvalMetricsTracker of the reference (utils/eval_metrics.py:162-350) with the metric arithmetic on the GPU.

Output files are byte-compatible with the reference (utils/eval_utils.py:57-84): `timestamps.txt`
("{idx} {ts:.15f}"), `<metric>.txt` / `event_rate.txt` ("{idx} {score:.5f}"), `frame_%010d.png`
(round(img*255) uint8) -- the formats analyze_robustness.py:55-65,109-110 and downstream_tasks/ parse.
Frames arrive in batches; gating (start/end time, |ref_ts-img_ts| <= ts_tol_ms, not color) is per frame.

Metric plug-ins keep the reference's contract (utils/eval_metrics.py:18-75): a `BaseMetric` subclass with `name`,
`no_ref`, `calculate(img, ref) -> float | list`, `finish_queue()`, `reset()`.  Three kinds live side by side:
  * the GPU metrics of `_SCORERS` below run batched, one launch set per scorer: 'mse', 'ssim' and 'lpips' are booked frame by
    frame; the others ('lpips-vgg', 'dists', 'psnr', 'ms_ssim', 'gmsd', 'vifp', 'niqe', 'brisque', 'piqe') through the four-frame queue of the
    reference's pyiqa metrics, so their files hold the same lines.  'lpips', 'lpips-vgg', 'dists', 'niqe' and 'brisque' need a weights or
    model file; 'psnr' / 'ms_ssim', 'piqe', 'gmsd' and 'vifp' need none and have a switch (EVREAL_GPU_FR_METRICS,
    EVREAL_GPU_PIQE, EVREAL_GPU_GMSD, EVREAL_GPU_VIFP: '0' sends the name to pyiqa instead -- which knows no 'vifp': its 'vif' is
    the wavelet-domain form, another number, and stays pyiqa's);
  * anything registered with `register_metric(name, factory)` runs per frame on host arrays, exactly like the reference's
    MseMetric / SsimMetric (clipped float32 [H,W] images in, a float or a list of floats out);
  * any other name is looked up in pyiqa.list_models() when pyiqa is importable (queued in batches of 4 as
    PyIqaMetricFactory does, :100-156); without pyiqa it is reported as "Unknown metric", as the reference does for a
    name it does not know (:203).

Adding a GPU metric: a Python wrapper around its kernels (batched frames in, float64 rows out on the device), ONE `_GpuScorer`
entry in `_SCORERS` (names and columns, row width, no_ref, booking, handle, size limit, the call), and its tests.  The tracker and
evaluate()'s chunk loop (evreal_amd/eval.py) are driven by that table and name no metric themselves.
"""
import math
import os
import traceback
import warnings
from os.path import join

import numpy as np
import torch

from .lpips import DISTS, LPIPS, LPIPSVGG
from .prepost import GMSD, VIFP, FullRefMetrics, Metrics, histogram_equalization

DEFAULT_METRICS = ('mse', 'ssim', 'lpips')      # the reference's default (eval.py:413-445, utils/eval_metrics.py:171)
GPU_METRICS = ('mse', 'ssim')
FR_METRICS = ('psnr', 'ms_ssim')                # full-reference, closed form, queued like the reference's pyiqa metrics
FR_METRICS_ENV = 'EVREAL_GPU_FR_METRICS'        # '0': psnr / ms_ssim go to pyiqa (or are unknown without it)
PIQE_ENV = 'EVREAL_GPU_PIQE'                    # '0': piqe goes to pyiqa (or is unknown without it)
GMSD_ENV = 'EVREAL_GPU_GMSD'                    # '0': gmsd goes to pyiqa (or is unknown without it)
VIFP_ENV = 'EVREAL_GPU_VIFP'                    # '0': vifp goes to pyiqa (or is unknown without it)
LPIPS_WEIGHTS_ENV = 'EVREAL_LPIPS_WEIGHTS'      # path to a pyiqa/lpips AlexNet-v0.1 state_dict (torch.save'd)
LPIPS_VGG_WEIGHTS_ENV = 'EVREAL_LPIPS_VGG_WEIGHTS'      # path to a pyiqa lpips-vgg (VGG-16, v0.1) state_dict (torch.save'd)
DISTS_WEIGHTS_ENV = 'EVREAL_DISTS_WEIGHTS'      # path to a pyiqa dists state_dict (torch.save'd)
NIQE_MODEL_ENV = 'EVREAL_NIQE_MODEL'            # path to a NIQE pristine model (.mat of the MATLAB release, or .npz)
NIQE_MODEL_FILES = (os.path.join('pretrained', 'niqe_modelparameters.mat'), os.path.join('pretrained', 'niqe_model.npz'))
BRISQUE_MODEL_ENV = 'EVREAL_BRISQUE_MODEL'      # path to a BRISQUE model (.npz, or a libsvm text model such as allmodel)
BRISQUE_RANGE_ENV = 'EVREAL_BRISQUE_RANGE'      # the svm-scale range file of a libsvm model (default: allrange beside it)


def _load_backbone(name, cls, env, file):
    """`cls` on the state dict at $env or pretrained/`file`.  The reference lets pyiqa download the weights; offline they must be
    supplied as a file, made where pyiqa exists by torch.save(pyiqa.create_metric(name).net.state_dict(), path)."""
    path = os.environ.get(env, os.path.join('pretrained', file))
    if not os.path.exists(path):
        print(f"{name}: no weights at ${env} or pretrained/{file} (pyiqa downloads them; "
              "offline they must be provided) -> falling back to pyiqa if it is installed")
        return None
    return cls(torch.load(path, map_location='cpu', weights_only=False))


def _load_lpips():
    return _load_backbone('lpips', LPIPS, LPIPS_WEIGHTS_ENV, 'lpips_alex.pth')


def _load_lpips_vgg():
    return _load_backbone('lpips-vgg', LPIPSVGG, LPIPS_VGG_WEIGHTS_ENV, 'lpips_vgg.pth')


def _load_dists():
    return _load_backbone('dists', DISTS, DISTS_WEIGHTS_ENV, 'dists.pth')


def gpu_fr_metrics_enabled():
    return os.environ.get(FR_METRICS_ENV, '1') != '0'


def gpu_piqe_enabled():
    return os.environ.get(PIQE_ENV, '1') != '0'


def gpu_gmsd_enabled():
    return os.environ.get(GMSD_ENV, '1') != '0'


def gpu_vifp_enabled():
    return os.environ.get(VIFP_ENV, '1') != '0'


def niqe_model_path():
    """The first of $EVREAL_NIQE_MODEL, pretrained/niqe_modelparameters.mat, pretrained/niqe_model.npz that exists, or None."""
    for path in (os.environ.get(NIQE_MODEL_ENV),) + NIQE_MODEL_FILES:
        if path and os.path.exists(path):
            return path
    return None


def _load_niqe():
    path = niqe_model_path()
    if path is None:
        return None
    from .nriqa import NIQE, load_niqe_model
    model = load_niqe_model(path)
    print(f"niqe: model {path} ({model['source']})")
    return NIQE(model)


def brisque_model_path():
    """-> (model path, range path or None) for the first that exists of: $EVREAL_BRISQUE_MODEL (an .npz, or a libsvm model
    with $EVREAL_BRISQUE_RANGE, else `allrange` beside it), pretrained/brisque_model.npz, pretrained/allmodel with
    pretrained/allrange; None without one."""
    path = os.environ.get(BRISQUE_MODEL_ENV)
    if path and os.path.exists(path):
        if path.lower().endswith('.npz'):
            return path, None
        return path, os.environ.get(BRISQUE_RANGE_ENV) or os.path.join(os.path.dirname(path), 'allrange')
    npz = os.path.join('pretrained', 'brisque_model.npz')
    if os.path.exists(npz):
        return npz, None
    model, rng = os.path.join('pretrained', 'allmodel'), os.path.join('pretrained', 'allrange')
    if os.path.exists(model) and os.path.exists(rng):
        return model, rng
    return None


def _load_brisque():
    found = brisque_model_path()
    if found is None:
        return None
    from .nriqa import BRISQUE, load_brisque_model
    model = load_brisque_model(*found)
    print(f"brisque: model {found[0]} ({model['source']})")
    return BRISQUE(model)


def _load_piqe():
    """PIQE has no model file: the object is its workspace."""
    from .nriqa import PIQE
    return PIQE()


class BaseMetric:
    """Base class for quantitative evaluation metrics -- the plug-in contract of utils/eval_metrics.py:18-75."""

    def __init__(self, name, no_ref=False):
        self.scores = []
        self.name = name
        self.no_ref = no_ref
        self.updated = 0
        self.image_queue = []
        self.ref_queue = []
        self.batch_size = 4

    def reset(self):
        self.scores, self.image_queue, self.ref_queue, self.updated = [], [], [], 0

    def finish_queue(self):
        self.updated = 0

    def get_num_updated(self):
        return self.updated

    def calculate(self, img, ref):
        raise NotImplementedError

    def update(self, img, ref=None):
        self.updated = 0
        score = self.calculate(img, ref)
        self.add(score if isinstance(score, list) else [score])

    def add(self, values):
        """Keep the finite scores (utils/eval_metrics.py:49-53)."""
        self.updated = 0
        for s in values:
            s = float(s)
            if math.isfinite(s) and not math.isnan(s):
                self.updated += 1
                self.scores.append(s)

    def get_num_scores(self):
        return len(self.scores)

    def get_all_scores(self):
        return self.scores

    def get_last_score(self):
        return self.scores[-1]

    def get_last_scores(self, n):
        return self.scores[-n:]

    def get_mean_score(self):
        return -1 if not self.scores else sum(self.scores) / len(self.scores)

    def get_name(self):
        return self.name


class GpuMetric(BaseMetric):
    """'mse' / 'ssim' / 'lpips': the tracker computes a whole batch with one launch and hands the scores to add()."""
    on_gpu = True

    def calculate(self, img, ref):
        raise RuntimeError(f"{self.name} is computed in batches by EvalMetricsTracker.update_batch")


class QueuedGpuMetric(GpuMetric):
    """A GPU metric booked as the reference books its queued pyiqa metrics (utils/eval_metrics.py:119-147, 217-223): the
    scores of every `batch_size` evaluated frames leave together, their finite ones against the last evaluated indices; the
    tail leaves at finalize() as it is (a non-finite tail score is kept, as the reference's finish_queue keeps it)."""

    def reset(self):
        super().reset()
        self.pending = []

    def book(self, history, indices, scores):
        """history: the evaluated indices before this batch; -> the (index, score) lines this batch's frames release."""
        hist, lines = list(history[-self.batch_size:]), []
        for i, s in zip(indices, scores):
            hist.append(i)
            self.pending.append(float(s))
            if len(self.pending) == self.batch_size:
                self.add(self.pending)
                self.pending = []
                if self.updated:
                    lines += zip(hist[-self.updated:], self.get_last_scores(self.updated))
        self.updated = 0
        return lines

    def finish_queue(self):
        self.updated = len(self.pending)
        self.scores.extend(self.pending)
        self.pending = []


_REGISTRY = {}


def register_metric(name, factory):
    """Make `name` available to -qm / quan_eval_metric_names: factory() -> BaseMetric (per-frame, host arrays)."""
    _REGISTRY[name] = factory


class PyIqaMetricFactory:
    """Any pyiqa metric by name (utils/eval_metrics.py:100-156), when pyiqa can be imported: gray frames are replicated
    to 3 channels (cv2torch(num_ch=3), eval_utils.py:46-54), queued, and scored four at a time; the queue's tail is
    flushed by finish_queue()."""

    def __init__(self):
        try:
            import pyiqa
        except Exception:
            pyiqa = None
        self.pyiqa = pyiqa
        self.list_of_metrics = list(pyiqa.list_models()) if pyiqa is not None else []
        self.created_metrics = {}

    def get_metric(self, name):
        if name in self.created_metrics:
            return self.created_metrics[name]
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", category=UserWarning)
            iqa_metric = self.pyiqa.create_metric(name)
        metric = _QueuedIqaMetric(name.lower(), iqa_metric.metric_mode == 'NR', iqa_metric)
        self.created_metrics[name] = metric
        return metric


def _as_batch(image, num_ch=3):
    t = torch.as_tensor(np.asarray(image))
    if t.dim() == 2:
        t = t.unsqueeze(0)
        if num_ch > 1:
            t = t.repeat(num_ch, 1, 1)
    return t.unsqueeze(0) if t.dim() == 3 else t


class _QueuedIqaMetric(BaseMetric):
    def __init__(self, name, no_ref, fn):
        super().__init__(name, no_ref)
        self.fn = fn

    def inference(self):
        if not self.image_queue:
            return []
        imgs = torch.cat(self.image_queue[-self.batch_size:])
        if self.ref_queue[0] is not None:
            scores = self.fn(imgs, torch.cat(self.ref_queue[-self.batch_size:]))
        else:
            scores = self.fn(imgs)
        self.image_queue, self.ref_queue = [], []
        out = scores.squeeze().tolist()
        return out if isinstance(out, list) else [out]

    def finish_queue(self):
        self.updated = 0
        score = self.inference()
        self.updated += len(score)
        self.scores.extend(score)

    def calculate(self, img, ref=None):
        self.image_queue.append(_as_batch(img))
        self.ref_queue.append(None if ref is None else _as_batch(ref))
        return [] if len(self.image_queue) < self.batch_size else self.inference()


_pyiqa_factory = None


def pyiqa_metric_factory():
    global _pyiqa_factory
    if _pyiqa_factory is None:
        _pyiqa_factory = PyIqaMetricFactory()
    return _pyiqa_factory


class _GpuScorer:
    """One GPU launch set and everything the tracker and evaluate()'s chunk loop need to know about it:
    columns: {metric name: column of the output row}; width: doubles per frame; no_ref: takes no reference frames;
    queued: booked with QueuedGpuMetric (else GpuMetric); before_registry: resolved ahead of register_metric's names (else after
    them); enabled(): the environment switch (None: available when the handle exists); handle(tracker): the callable, made at
    the first request; too_small(name, H, W): why `name` is not defined on H x W frames, or None;
    run(handle, img, ref, names, out): the rows of `img` [n,H,W] (and `ref`) into out [n,width], on the current stream -- `names`
    are the wanted ones of `columns`; the other columns hold anything."""

    def __init__(self, columns, width, handle, run, no_ref=False, queued=True, before_registry=False, enabled=None, too_small=None):
        self.columns, self.width, self.handle, self.run = columns, width, handle, run
        self.no_ref, self.queued, self.before_registry, self.enabled = no_ref, queued, before_registry, enabled
        self.too_small = too_small or (lambda name, H, W: None)

    def available(self, tracker):
        return self.enabled() if self.enabled is not None else self.handle(tracker) is not None

    def metric(self, name):
        return (QueuedGpuMetric if self.queued else GpuMetric)(name, no_ref=self.no_ref)


def _run_no_ref(h, img, ref, names, out):
    h(img, clip=True, out=out[:, 0])


# In the order evaluate()'s chunk loop launches them: the reference-needing ones, then the no-reference ones.
_SCORERS = (
    _GpuScorer({'mse': 0, 'ssim': 1}, 2, lambda t: t._gpu, queued=False, before_registry=True,
               run=lambda h, img, ref, names, out: out.copy_(h(img, ref, mse='mse' in names, ssim='ssim' in names, clip=True))),
    _GpuScorer({'lpips': 0}, 1, lambda t: t._lpips_model(), queued=False, before_registry=True,
               run=lambda h, img, ref, names, out: out[:, 0].copy_(h(img, ref, clip=True))),
    # one launch set for both; ms_ssim needs five scales of an 11x11 window
    _GpuScorer({'psnr': 0, 'ms_ssim': 1}, 2, lambda t: t._fr, enabled=gpu_fr_metrics_enabled,
               too_small=lambda name, H, W: FullRefMetrics.too_small(H, W) if name == 'ms_ssim' else None,
               run=lambda h, img, ref, names, out: h(img, ref, psnr='psnr' in names, ms_ssim='ms_ssim' in names, clip=True, out=out)),
    _GpuScorer({'gmsd': 0}, 2, lambda t: t._gmsd, enabled=gpu_gmsd_enabled,           # (column 1: the mean GMS)
               too_small=lambda name, H, W: GMSD.too_small(H, W),
               run=lambda h, img, ref, names, out: h(img, ref, clip=True, out=out)),
    _GpuScorer({'vifp': 0}, 9, lambda t: t._vifp, enabled=gpu_vifp_enabled,           # (columns 1..8: num and den of the four scales)
               too_small=lambda name, H, W: VIFP.too_small(H, W),
               run=lambda h, img, ref, names, out: h(img, ref, clip=True, out=out)),
    _GpuScorer({'lpips-vgg': 0}, 1, lambda t: t._cached('_lpips_vgg_cache'), before_registry=True,
               too_small=lambda name, H, W: LPIPSVGG.too_small(H, W),
               run=lambda h, img, ref, names, out: h(img, ref, clip=True, out=out[:, 0])),
    _GpuScorer({'dists': 0}, 1, lambda t: t._cached('_dists_cache'), before_registry=True,
               too_small=lambda name, H, W: DISTS.too_small(H, W),
               run=lambda h, img, ref, names, out: h(img, ref, clip=True, out=out[:, 0])),
    _GpuScorer({'niqe': 0}, 1, lambda t: t._cached('_niqe_cache'), _run_no_ref, no_ref=True, before_registry=True),
    _GpuScorer({'brisque': 0}, 1, lambda t: t._cached('_brisque_cache'), _run_no_ref, no_ref=True, before_registry=True),
    _GpuScorer({'piqe': 0}, 1, lambda t: t._cached('_piqe_cache'), _run_no_ref, no_ref=True, enabled=gpu_piqe_enabled),
)
_SCORER_OF = {name: s for s in _SCORERS for name in s.columns}


def chunk_scorers(tracker, names, H, W):
    """-> [(scorer, handle, the names it serves)] for a frame loop that computes `names` (of wants_precomputed()) for whole chunks of
    H x W frames itself.  A name that is not defined on frames of this size is left out (the tracker prints the exception and
    resets the metric, as the reference does for a metric that raises); a scorer left without a name is left out altogether."""
    found = []
    for s in _SCORERS:
        served = [name for name in s.columns if name in names and s.too_small(name, H, W) is None]
        if served:
            found.append((s, s.handle(tracker), served))
    return found


class EvalMetricsTracker:
    def __init__(self, save_images=False, save_processed_images=False, output_dir=None, hist_eq='none',
                 quan_eval_metric_names=None, quan_eval_start_time=0, quan_eval_end_time=float('inf'),
                 quan_eval_ts_tol_ms=float('inf'), has_reference_frames=False, color=False):
        if quan_eval_metric_names is None:
            quan_eval_metric_names = list(DEFAULT_METRICS)
        if hist_eq not in ('none', 'global', 'local', 'clahe'):
            raise ValueError(f"Unrecognized histogram equalization argument: {hist_eq}")
        self.save_images, self.output_dir, self.hist_eq = save_images, output_dir, hist_eq
        self.save_processed_images = save_processed_images
        if self.hist_eq == 'none' and self.save_processed_images:
            print("Can not save processed images when hist_eq is none")
            self.save_processed_images = False
        self._pending = []
        self._files = {}
        self.start, self.end, self.tol_ms = quan_eval_start_time, quan_eval_end_time, quan_eval_ts_tol_ms
        self.has_reference_frames, self.color = has_reference_frames, color
        self.quan_eval_indices = []
        self._gpu = Metrics()
        self._fr = FullRefMetrics()
        self._gmsd = GMSD()
        self._vifp = VIFP()
        self.metrics = [m for m in map(self._resolve, quan_eval_metric_names) if m is not None]
        if not self.has_reference_frames:
            self.metrics = [m for m in self.metrics if m.no_ref]
        self.only_no_ref = all(m.no_ref for m in self.metrics)
        self.reset()

    def _resolve(self, name):
        """-> the metric object of `name`: this project's GPU metric, a registered plug-in, pyiqa's -- in that order, with the
        GPU metrics that have a switch after the plug-ins; None (and the reference's line, :203) for a name nobody knows."""
        s = _SCORER_OF.get(name)
        if s is not None and s.before_registry and s.available(self):
            return s.metric(name)
        if name in _REGISTRY:
            return _REGISTRY[name]()
        if s is not None and not s.before_registry and s.available(self):
            return s.metric(name)
        if name in pyiqa_metric_factory().list_of_metrics:
            return pyiqa_metric_factory().get_metric(name)
        print("Unknown metric " + name)
        return None

    # One handle per process and name: [loaded, handle or None], filled at the first request of the name (None without a weights
    # or model file: the name then goes to its other providers).  Tests put stand-ins here, and in _lpips_model.
    _LOADERS = {'_lpips_cache': _load_lpips, '_lpips_vgg_cache': _load_lpips_vgg, '_dists_cache': _load_dists,
                '_niqe_cache': _load_niqe,
                '_brisque_cache': _load_brisque, '_piqe_cache': _load_piqe}
    _lpips_cache = [False, None]
    _lpips_vgg_cache = [False, None]
    _dists_cache = [False, None]
    _niqe_cache = [False, None]
    _brisque_cache = [False, None]
    _piqe_cache = [False, None]

    @classmethod
    def _cached(cls, cache):
        if not getattr(cls, cache)[0]:
            setattr(cls, cache, [True, cls._LOADERS[cache]()])
        return getattr(cls, cache)[1]

    @classmethod
    def _lpips_model(cls):
        return cls._cached('_lpips_cache')

    # -- files --------------------------------------------------------------------------------
    def reset(self):
        os.makedirs(self.output_dir, exist_ok=True)
        if self.save_processed_images:
            self.processed_output_dir = self.output_dir + "_processed"
            os.makedirs(self.processed_output_dir, exist_ok=True)
        self._close_files()
        self._failed = set()        # GPU metrics that refused this sequence's frame size: reset, and left alone from then on
        open(join(self.output_dir, 'timestamps.txt'), 'w', encoding="utf-8").close()
        for m in self.metrics:
            open(join(self.output_dir, m.name + '.txt'), 'w', encoding="utf-8").close()
            m.reset()

    # Text outputs: the reference re-opens a file for every line (eval_utils.py:57-69).  Here a tracker keeps its files
    # open in append mode and writes a batch of lines at a time; finalize() closes them.  Same bytes, no per-frame
    # open/close on the critical path.
    def _file(self, path):
        f = self._files.get(path)
        if f is None:
            f = self._files[path] = open(path, 'a', encoding="utf-8")
        return f

    def _close_files(self):
        for f in self._files.values():
            f.close()
        self._files = {}

    def _append(self, path, pairs, fmt='{} {:.5f}\n'):
        f = self._file(path)
        f.write(''.join(fmt.format(a, b) for a, b in pairs))

    def save_custom_metric(self, idx, metric_name, metric_value, is_int=False):
        path = join(self.output_dir, metric_name + '.txt')
        if idx == 0:      # the reference only truncates on idx 0 (eval_metrics.py:277-278)
            old = self._files.pop(path, None)
            if old is not None:
                old.close()
            open(path, 'w', encoding="utf-8").close()
        self._append(path, [(idx, metric_value)], '{} {}\n' if is_int else '{} {:.5f}\n')

    def save_new_scores(self, metric):
        """eval_metrics.py:217-223: the scores a metric produced since its last update, against the LAST evaluated indices
        (a queued metric returns nothing until its batch is full, then `batch_size` scores at once)."""
        n = metric.get_num_updated()
        if n > 0:
            self._append(join(self.output_dir, metric.name + '.txt'),
                         zip(self.quan_eval_indices[-n:], metric.get_last_scores(n)))

    # -- per batch ----------------------------------------------------------------------------
    def wants_precomputed(self):
        """Names of the GPU metrics a frame loop may compute for a whole chunk itself and hand to update_batch(scores=...):
        only when no histogram equalisation stands between the frames and the scores."""
        if self.hist_eq != 'none' or self.color:
            return []
        if not self.has_reference_frames:       # (only no-reference metrics are left: they need no reference frames)
            return [m.name for m in self.metrics if getattr(m, 'on_gpu', False) and m.no_ref]
        return [m.name for m in self.metrics if getattr(m, 'on_gpu', False)]

    def _shape_refused(self, m, imgs):
        """A GPU metric that is not defined on frames of this size (ms_ssim below 161 pixels a side, gmsd below 2, vifp below 41, lpips-vgg and dists below 16) ends like a metric that
        raises on every frame in the reference (utils/eval_metrics.py:233-242: the exception is printed, the metric reset): its
        file stays empty and its mean is -1.  Decided from the shape, before any launch, and printed once per sequence."""
        if m.name in self._failed:
            return True
        why = _SCORER_OF[m.name].too_small(m.name, int(imgs.shape[-2]), int(imgs.shape[-1]))
        if why is None:
            return False
        print("Exception in metric " + m.get_name() + ": " + why)
        m.reset()
        self._failed.add(m.name)
        return True

    def update_batch(self, indices, imgs, refs, img_ts, ref_ts, scores=None, u8=None):
        """indices: dataset indices; imgs [n,H,W] cuda (unclipped); refs [n,H,W] cuda or None;
        img_ts / ref_ts: python floats per frame (ref_ts None -> img_ts).
        scores: optional {metric name: numpy [n]} already computed for EVERY frame of this call (see wants_precomputed);
        u8: optional numpy uint8 [n,H,W] = round(clip(imgs)*255), already on the host, for the PNG writers."""
        try:
            self._update_batch(indices, imgs, refs, img_ts, ref_ts, scores, u8)
        finally:
            for f in self._files.values():      # one write per file per batch reaches the OS even if a later frame raises
                f.flush()

    def _update_batch(self, indices, imgs, refs, img_ts, ref_ts, pre=None, u8=None):
        n = len(indices)
        if ref_ts is None:
            ref_ts = img_ts
        self._append(join(self.output_dir, 'timestamps.txt'), zip(indices, img_ts), '{} {:.15f}\n')
        if self.save_images:
            self._save_pngs(self.output_dir, indices, imgs, u8)    # clipped inside; BEFORE hist-eq (eval_metrics.py:257-258)
        sel = []
        for j in range(n):
            inside = self.start <= img_ts[j] <= self.end
            tol_ok = abs(ref_ts[j] - img_ts[j]) * 1000 <= self.tol_ms or self.only_no_ref
            if inside and tol_ok and not self.color:
                sel.append(j)
        need_proc = self.hist_eq != 'none' and (self.save_processed_images or (sel and self.metrics))
        if need_proc:
            # histogram equalisation of the clipped frames (eval_metrics.py:260-265); `none` leaves the clip to the kernels
            imgs = histogram_equalization(torch.clamp(imgs, 0.0, 1.0).contiguous(), self.hist_eq)
            if refs is not None and self.has_reference_frames:
                refs = histogram_equalization(torch.clamp(refs, 0.0, 1.0).contiguous(), self.hist_eq)
            if self.save_processed_images:
                self._save_pngs(self.processed_output_dir, indices, imgs)
        if not sel or not self.metrics:
            self.quan_eval_indices.extend(indices[j] for j in sel)
            return
        idxs = [indices[j] for j in sel]
        gpu = [m for m in self.metrics if getattr(m, 'on_gpu', False) and not self._shape_refused(m, imgs)]
        host = [m for m in self.metrics if not getattr(m, 'on_gpu', False)]
        have_pre = pre is not None and not need_proc and all(m.name in pre for m in gpu)
        isel = rsel = None
        if host or (gpu and not have_pre):
            js = torch.tensor(sel, device=imgs.device)
            isel = imgs[js].contiguous()
            rsel = refs[js].contiguous() if refs is not None else None
        if gpu:
            if have_pre:
                cols = {m.name: np.asarray(pre[m.name])[sel] for m in gpu}
            else:
                cols = {}
                for s, handle, names in chunk_scorers(self, [m.name for m in gpu], int(imgs.shape[-2]), int(imgs.shape[-1])):
                    rows = torch.empty((len(sel), s.width), dtype=torch.float64, device=isel.device)
                    s.run(handle, isel, rsel, names, rows)
                    rows = rows.cpu().numpy()
                    cols.update((name, rows[:, s.columns[name]]) for name in names)
            for m in gpu:
                col = cols[m.name]
                if isinstance(m, QueuedGpuMetric):
                    self._append(join(self.output_dir, m.name + '.txt'), m.book(self.quan_eval_indices, idxs, col))
                    continue
                m.add(col)
                self._append(join(self.output_dir, m.name + '.txt'),
                             [(i, float(s)) for i, s in zip(idxs, col) if math.isfinite(s)])
        if not host:
            self.quan_eval_indices.extend(idxs)
            return
        # plug-in metrics: clipped host arrays, frame by frame, exactly as update_quantitative_metrics (:230-242)
        himg = torch.clamp(isel, 0.0, 1.0).cpu().numpy()
        href = torch.clamp(rsel, 0.0, 1.0).cpu().numpy() if (rsel is not None and self.has_reference_frames) else None
        for k, idx in enumerate(idxs):
            self.quan_eval_indices.append(idx)
            for m in host:
                try:
                    if not self.has_reference_frames or m.no_ref:
                        m.update(himg[k])
                    else:
                        m.update(himg[k], href[k])
                    self.save_new_scores(m)
                except Exception as e:
                    print("Exception in metric " + m.get_name() + ": " + str(e))
                    print(traceback.format_exc())
                    m.reset()

    def update_batch_color(self, indices, bgr_u8, img_ts):
        """Colour frames (uint8 BGR [n,H,W,3] on the GPU): timestamps + PNGs only -- the reference skips every
        quantitative metric in colour mode (utils/eval_metrics.py:272)."""
        self._append(join(self.output_dir, 'timestamps.txt'), zip(indices, img_ts), '{} {:.15f}\n')
        if self.save_images:
            rgb = bgr_u8.flip(-1).contiguous().cpu()     # cv2.imwrite stores BGR arrays as RGB files
            if self._use_pil():
                for i, a in zip(indices, rgb.numpy()):
                    self._submit_png(join(self.output_dir, 'frame_{:010d}.png'.format(i)), a, 'RGB')
            else:
                self._submit_native(self.output_dir, indices, rgb, 3)

    # PNG encoding leaves the frame loop.  Round 6: a pool of NATIVE writer threads inside the library
    # (csrc/hostcodec.cpp: filter 0 + one zlib stream of level EVREAL_PNG_LEVEL, default 1; no GIL, ~0.3 ms per 346x260 frame and
    # core) takes whole chunks of frames per call; the files decode to exactly round(clip(img) * 255) (eval_utils.py:80-84).
    # EVREAL_PNG_THREADS=<n> sizes the pool (0: every call waits for its files -- synchronous, as the reference);
    # EVREAL_PNG_WRITER=pil keeps round 5's pool of PIL writers (~3 ms per frame and core, zlib level 6: smaller files).
    # finalize() waits for the files (and raises a writer's failure there).
    _pool = None
    _native = None

    @classmethod
    def _png_threads(cls):
        return int(os.environ.get('EVREAL_PNG_THREADS', '') or min(16, max(4, (os.cpu_count() or 4) // 2)))

    @classmethod
    def _writer_pool(cls):
        if cls._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            cls._pool = ThreadPoolExecutor(max_workers=max(1, cls._png_threads()))
        return cls._pool

    @classmethod
    def _native_pool(cls):
        if cls._native is None:
            import ctypes
            from . import lib as _lib
            h = ctypes.c_void_p()
            _lib.check(_lib.load().evr_png_pool_create(max(1, cls._png_threads()), int(os.environ.get('EVREAL_PNG_LEVEL', '1')), ctypes.byref(h)),
                       'evr_png_pool_create')
            cls._native = h
        return cls._native

    @staticmethod
    def _use_pil():
        return os.environ.get('EVREAL_PNG_WRITER', 'native') == 'pil'

    def _submit_png(self, path, array, mode):
        def job():
            from PIL import Image
            Image.fromarray(array, mode=mode).save(path)
        if os.environ.get('EVREAL_PNG_THREADS', '') == '0':
            job()                                            # synchronous, as the reference
        else:
            self._pending.append(self._writer_pool().submit(job))

    def _submit_native(self, folder, indices, frames, channels):
        """frames: uint8 host array/tensor [n, H, W] or [n, H, W, 3]; frame 0 contiguous, frames a constant stride apart."""
        import ctypes
        from . import lib as _lib
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        n, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
        if n == 0:
            return
        if not t[0].is_contiguous() or (n > 1 and t.stride(0) < H * W * channels):
            t = t.contiguous()
        idx = (ctypes.c_int64 * n)(*[int(i) for i in indices])
        _lib.check(_lib.load().evr_png_pool_submit(self._native_pool(), os.fsencode(folder), idx, n, ctypes.c_void_p(t.data_ptr()), H, W, channels,
                                                  int(t.stride(0)) if n > 1 else 0), 'evr_png_pool_submit')
        self._native_pending = True
        if os.environ.get('EVREAL_PNG_THREADS', '') == '0':
            self._wait_native()

    def _wait_native(self, ignore_errors=False):
        if getattr(self, '_native_pending', False) and type(self)._native is not None:
            from . import lib as _lib
            self._native_pending = False
            rc = _lib.load().evr_png_pool_wait(type(self)._native, None)
            if rc and not ignore_errors:
                _lib.check(rc, 'evr_png_pool_wait')

    def _save_pngs(self, folder, indices, imgs, u8=None):
        if u8 is None:
            u8 = torch.round(torch.clamp(imgs, 0.0, 1.0) * 255).to(torch.uint8).cpu()               # eval_utils.py:83
        if self._use_pil():
            for i, a in zip(indices, u8.numpy() if isinstance(u8, torch.Tensor) else u8):
                self._submit_png(join(folder, 'frame_{:010d}.png'.format(i)), np.ascontiguousarray(a), 'L')
        else:
            self._submit_native(folder, indices, u8, 1)

    def finalize(self, idx, wait_png=True):
        """eval_metrics.py:225-228: flush the queued metrics; then wait for this tracker's files.  wait_png=False (the drop-in's
        sequence loops): the native writers keep working on this tracker's last frames while the next sequence starts; the caller
        owes a wait_all_pngs() before it reports the dataset (evreal_amd.eval does it per dataset) -- 3 ms per 160-frame sequence."""
        self._warn_backbone_range('lpips-vgg', self._lpips_vgg_cache)
        self._warn_backbone_range('dists', self._dists_cache)
        for m in self.metrics:
            if isinstance(m, QueuedGpuMetric):
                m.finish_queue()
                self.save_new_scores(m)
                m.updated = 0
                continue
            if getattr(m, 'on_gpu', False):
                m.updated = 0
                continue
            try:
                m.finish_queue()
                self.save_new_scores(m)
            except Exception as e:
                print("Exception in metric " + m.get_name() + ": " + str(e))
                m.reset()
        for f in self._pending:
            f.result()                                       # re-raises a writer's exception here
        self._pending = []
        if wait_png:
            self._wait_native()                              # ... and a native writer's failure here
        self._close_files()

    def _warn_backbone_range(self, name, cache):
        """One line per sequence when an activation of the VGG trunk of `name` ('lpips-vgg', 'dists') left the exact range of the
        arithmetic mode's packed format (the handle's counter, read and cleared here: it is shared by the trackers of a process, so
        sequences evaluated in lock-step report together with the first of them that finishes).  The scores are kept;
        EVR_ARITH=fp32 computes them without a limit."""
        # (only this project's GPU metric: the same name served by pyiqa or by register_metric has no handle)
        if not any(m.name == name and getattr(m, 'on_gpu', False) for m in self.metrics):
            return
        model = cache[1]
        if model is None or name in self._failed or not self.quan_eval_indices:
            return
        count = model.saturation()
        if count:
            print(f"WARNING: {name}: {count} activation runs left the exact range of the packed format in {self.output_dir} "
                  "(scores kept; EVR_ARITH=fp32 evaluates without the limit)")

    @classmethod
    def wait_all_pngs(cls):
        """Every frame handed to the native writers so far is on disk when this returns; raises the first write failure."""
        if cls._native is not None:
            from . import lib as _lib
            _lib.check(_lib.load().evr_png_pool_wait(cls._native, None), 'evr_png_pool_wait')

    def discard(self):
        """Abandon this tracker (its sequence is re-run from the start with a fresh one, which truncates the same files): wait for
        the PNG writers still holding its frames -- they must not race the re-run's writes to the same paths -- and close the files."""
        for f in self._pending:
            try:
                f.result()
            except Exception:
                pass
        self._pending = []
        self._wait_native(ignore_errors=True)
        self._close_files()

    def get_num_quan_evaluations(self):
        return len(self.quan_eval_indices)

    def get_mean_scores(self):
        return {m.name: m.get_mean_score() for m in self.metrics}


class MetricTracker:
    """eval.py:249-276."""

    def __init__(self):
        self.data_dict = {}

    def init_key(self, key):
        self.data_dict[key] = {'total': 0.0, 'count': 0, 'average': 0.0}

    def update(self, key, value, count=1):
        if count == 0:
            return
        if key not in self.data_dict:
            self.init_key(key)
        d = self.data_dict[key]
        d['total'] += value * count
        d['count'] += count
        d['average'] = d['total'] / d['count']

    def get_average(self, key):
        if key not in self.data_dict:
            self.init_key(key)
        return self.data_dict[key]['average']

    def get_count(self, key):
        if key not in self.data_dict:
            self.init_key(key)
        return self.data_dict[key]['count']
