"""Host side of the pre/post-processing and metric kernels (same names as the reference)."""
import numpy as np
import torch

from . import lib as _lib


def normalize_event_tensor(event_tensor, stats=None):
    """eval.py:398-410, per window, IN PLACE on a cuda tensor [N,B,H,W]."""
    lib = _lib.load()
    assert event_tensor.is_cuda and event_tensor.dtype == torch.float32 and event_tensor.is_contiguous()
    n, B, H, W = event_tensor.shape
    ws = None
    if stats is None:
        ws = torch.empty(n * 32 * 3, dtype=torch.float64, device=event_tensor.device)
    _lib.check(lib.evr_event_tensor_normalize(_lib.ptr(event_tensor), n, B, H, W, _lib.ptr(stats), _lib.ptr(ws),
                                              0 if ws is None else ws.numel() * 8, _lib.stream_ptr()),
               'evr_event_tensor_normalize')
    return event_tensor


def post_process_normalization(img, norm):
    """eval.py:380-395 on cuda tensors [N,H,W] (or [H,W]), in place."""
    if norm == 'none':
        return img
    if norm not in ('robust', 'standard', 'exprobust'):
        raise ValueError(f"Unrecognized normalization argument: {norm}")
    lib = _lib.load()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
    v = img if img.dim() == 3 else img.unsqueeze(0)
    n, H, W = v.shape
    q = (0.0, 100.0) if norm == 'standard' else (1.0, 99.0)
    ws = torch.empty(max(int(lib.evr_percentile_normalize_workspace_bytes(n, H, W)), 16) // 4, dtype=torch.float32, device=img.device)
    _lib.check(lib.evr_percentile_normalize(_lib.ptr(v), n, H, W, q[0], q[1], 1 if norm == 'exprobust' else 0,
                                            _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), 'evr_percentile_normalize')
    return img


_color_values = {}      # (device, exp?) -> float32 [256] on the device: byte level -> image value
_color_ws = {}          # device -> workspace


def color_post_process_normalization(bgr_u8, norm, out=None, return_range=False):
    """eval.py:380-395 as colour mode applies it: on the merged uint8 BGR frames, cuda uint8 [n,H,W,3] (or [H,W,3]).
    Per frame img = float32(u8) / 255 (np.exp of that for 'exprobust'), lo / hi = np.percentile over all 3*H*W values together,
    and the result is the byte the image writer stores, round(clip((img - lo) / (hi - lo), 0, 1) * 255) -- bit-exact against numpy
    (0/0 = NaN, where hi == lo, is byte 0).  Writes into `out` (default: a new tensor; `out=bgr_u8` works in place) and returns it,
    with return_range=True also the float32 [n,2] = (lo, hi) of every frame.  'none' returns the input untouched."""
    if norm not in ('none', 'robust', 'standard', 'exprobust'):
        raise ValueError(f"Unrecognized normalization argument: {norm}")
    if norm == 'none':
        return (bgr_u8, None) if return_range else bgr_u8
    lib = _lib.load()
    assert bgr_u8.is_cuda and bgr_u8.dtype == torch.uint8 and bgr_u8.is_contiguous() and bgr_u8.shape[-1] == 3
    assert bgr_u8.dim() in (3, 4)
    if out is None:
        out = torch.empty_like(bgr_u8)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == bgr_u8.shape
    n = bgr_u8.shape[0] if bgr_u8.dim() == 4 else 1
    H, W = bgr_u8.shape[-3], bgr_u8.shape[-2]
    dev, exp = bgr_u8.device, norm == 'exprobust'
    values = _color_values.get((dev, exp))
    if values is None:
        v = np.arange(256).astype(np.uint8).astype(np.float32) / np.float32(255)
        values = _color_values[(dev, exp)] = torch.from_numpy(np.exp(v) if exp else v).to(dev)
    need = int(lib.evr_color_percentile_normalize_workspace_bytes(n))
    ws = _color_ws.get(dev)
    if return_range or ws is None or ws.numel() * 4 < need:       # (a caller who reads the range keeps its own workspace)
        ws = torch.empty(max(need, 16) // 4, dtype=torch.int32, device=dev)
        if not return_range:
            _color_ws[dev] = ws
    q = (0.0, 100.0) if norm == 'standard' else (1.0, 99.0)
    _lib.check(lib.evr_color_percentile_normalize(_lib.ptr(bgr_u8), _lib.ptr(out), n, H, W, _lib.ptr(values), q[0], q[1],
                                                  _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()),
               'evr_color_percentile_normalize')
    if return_range:
        return out, ws[n * 256:n * 258].view(torch.float32).view(n, 2)
    return out


class Workspace:
    """A handle's device workspace `ws`, sized by the library's `_workspace_bytes`(n, H, W): kept between calls, made anew
    when it is too small or lives on another device."""
    _workspace_bytes = None     # the entry point's name

    def _workspace(self, n, H, W, device):
        need = int(getattr(self.lib, self._workspace_bytes)(n, H, W))
        if self.ws is None or self.ws.numel() < need or self.ws.device != device:
            self.ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self.ws


class PairMetric(Workspace):
    """What the closed-form full-reference handles share.  Constructing one touches neither the library nor the GPU; the
    workspace is owned and grows on demand."""
    MIN_SIDE = 1
    _too_small = None           # the metric's sentence, with {m} for MIN_SIDE and {H}, {W}

    def __init__(self):
        self.lib = None
        self.ws = None

    @classmethod
    def too_small(cls, H, W):
        """The message of the exception the metric raises on frames of this size, or None where it is defined."""
        if min(H, W) >= cls.MIN_SIDE:
            return None
        return cls._too_small.format(m=cls.MIN_SIDE, H=H, W=W)

    def _frames(self, img, ref, sized=True):
        """cuda float32 [n,H,W] (or [H,W], or [...,H,W]) pairs -> (img, ref, n, H, W), contiguous, the library loaded and the
        workspace ready.  sized: frames below MIN_SIDE raise ValueError, decided from the shape: no launch is tried."""
        assert img.is_cuda and ref.is_cuda and img.shape == ref.shape and img.dtype == ref.dtype == torch.float32
        img = img.contiguous(); ref = ref.contiguous()
        v = img if img.dim() == 3 else img.reshape(-1, img.shape[-2], img.shape[-1])
        n, H, W = v.shape
        if sized and self.too_small(H, W):
            raise ValueError(self.too_small(H, W))
        if self.lib is None:
            self.lib = _lib.load()
        self._workspace(n, H, W, img.device)
        return img, ref, n, H, W

    @staticmethod
    def _out(out, shape, device):
        """`out`, or a new tensor where it is None: contiguous cuda float64 of `shape`."""
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == tuple(shape)
        return out


class Metrics(PairMetric):
    """MSE + SSIM of utils/eval_metrics.py:77-97 (with the [0,1] clip of :253-255) for a batch of frames."""
    _workspace_bytes = 'evr_metrics_workspace_bytes'

    def __init__(self):
        super().__init__()
        self.lib = _lib.load()

    def __call__(self, img, ref, mse=True, ssim=True, clip=True):
        img, ref, n, H, W = self._frames(img, ref, sized=False)       # (the entry point refuses SSIM below 12x12)
        out = self._out(None, (n, 2), img.device)
        which = (1 if mse else 0) | (2 if ssim else 0)
        _lib.check(self.lib.evr_metrics(_lib.ptr(img), _lib.ptr(ref), n, H, W, which, 1 if clip else 0,
                                        _lib.ptr(out), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()),
                   'evr_metrics')
        return out


class FullRefMetrics(PairMetric):
    """PSNR + MS-SSIM (pyiqa's `psnr` and `ms_ssim` on [0,1] gray frames, data_range 1) for a batch of frames, in fp64
    (evr_fr_metrics)."""
    MIN_SIDE = 161          # ms_ssim: five scales of an 11x11 window (pytorch-msssim asserts min(H, W) > 160)
    _too_small = "ms_ssim needs frames of at least {m}x{m} pixels (five scales of an 11x11 window), got {H}x{W}"
    _workspace_bytes = 'evr_fr_metrics_workspace_bytes'

    def __call__(self, img, ref, psnr=True, ms_ssim=True, clip=True, out=None, out_scales=None):
        """img, ref: cuda float32 [n,H,W] (or [H,W]) -> float64 [n,2] = (psnr, ms_ssim), 0 in a column not asked for.
        out / out_scales: optional contiguous float64 [n,2] / [n,10] to write into (out_scales: CS_1..5, S_1..5)."""
        img, ref, n, H, W = self._frames(img, ref, sized=ms_ssim)
        out = self._out(out, (n, 2), img.device)
        if out_scales is not None:
            self._out(out_scales, (n, 10), img.device)
        which = (1 if psnr else 0) | (2 if ms_ssim else 0)
        _lib.check(self.lib.evr_fr_metrics(_lib.ptr(img), _lib.ptr(ref), n, H, W, which, 1 if clip else 0, _lib.ptr(out),
                                           _lib.ptr(out_scales), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()),
                   'evr_fr_metrics')
        return out

    def per_scale(self, img, ref, clip=True, psnr=True):
        """-> (scores [n,2], scales [n,10]): the means of the contrast-structure maps CS_1..5, then of the SSIM maps S_1..5."""
        n = 1 if img.dim() == 2 else int(np.prod(img.shape[:-2]))
        scales = torch.empty((n, 10), dtype=torch.float64, device=img.device)
        return self(img, ref, psnr=psnr, ms_ssim=True, clip=clip, out_scales=scales), scales


class GMSD(PairMetric):
    """GMSD (Xue et al. 2014; pyiqa's `gmsd`) for a batch of frame pairs, in fp64 (evr_gmsd): frames quantised to
    rint(255 * clip(v)), 2x2 mean pooling, Prewitt / 3 with zero padding, GMS with c = 170, the standard deviation over the
    pooled pixels with N - 1."""
    MIN_SIDE = 2            # one pixel of the 2x2-pooled plane
    _too_small = "gmsd needs frames of at least {m}x{m} pixels (it pools 2x2 first), got {H}x{W}"
    _workspace_bytes = 'evr_gmsd_workspace_bytes'

    def stats(self, img, ref, clip=True, out=None, out_map=None):
        """img, ref: cuda float32 [n,H,W] (or [H,W]) -> float64 [n,2] = (score, mean GMS).
        out / out_map: optional contiguous float64 [n,2] / [n,H//2,W//2] to write into (out_map: the GMS map q)."""
        img, ref, n, H, W = self._frames(img, ref)
        out = self._out(out, (n, 2), img.device)
        if out_map is not None:
            self._out(out_map, (n, H // 2, W // 2), img.device)
        _lib.check(self.lib.evr_gmsd(_lib.ptr(img), _lib.ptr(ref), n, H, W, 1 if clip else 0, _lib.ptr(out), _lib.ptr(out_map),
                                     _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr()), 'evr_gmsd')
        return out

    def __call__(self, img, ref, clip=True, out=None):
        """-> float64 [n] scores.  out: optional float64 [n,2] (score, mean GMS) to write into; its first column is returned."""
        return self.stats(img, ref, clip=clip, out=out)[:, 0]

    def map(self, img, ref, clip=True):
        """-> (stats [n,2], GMS map [n,H//2,W//2])."""
        n = 1 if img.dim() == 2 else int(np.prod(img.shape[:-2]))
        q = torch.empty((n, img.shape[-2] // 2, img.shape[-1] // 2), dtype=torch.float64, device=img.device)
        return self.stats(img, ref, clip=clip, out_map=q), q


class VIFP(PairMetric):
    """VIFp (Sheikh & Bovik 2006, pixel domain: vifp_mscale.m, sewar.vifp) for a batch of frame pairs, in fp64 (evr_vifp): four
    scales of Gaussian-windowed second moments of 255 * frame over the valid region, sum of the information that survives the
    channel g*x + noise over the reference's own.  `img` is the reconstruction, `ref` the reference: the score is not symmetric."""
    MIN_SIDE = 41           # 41 -> 17 -> 7 -> 3: one 3x3 window at the fourth scale
    _too_small = "vifp needs frames of at least {m}x{m} pixels (four scales, the last one 3x3 window), got {H}x{W}"
    _workspace_bytes = 'evr_vifp_workspace_bytes'

    def stats(self, img, ref, clip=True, out=None):
        """img, ref: cuda float32 [n,H,W] (or [H,W]) -> float64 [n,9] = (score, num_1..4, den_1..4).
        out: optional contiguous float64 [n,9] to write into."""
        img, ref, n, H, W = self._frames(img, ref)
        out = self._out(out, (n, 9), img.device)
        _lib.check(self.lib.evr_vifp(_lib.ptr(img), _lib.ptr(ref), n, H, W, 1 if clip else 0, _lib.ptr(out), _lib.ptr(self.ws),
                                     self.ws.numel(), _lib.stream_ptr()), 'evr_vifp')
        return out

    def __call__(self, img, ref, clip=True, out=None):
        """-> float64 [n] scores.  out: optional float64 [n,9] to write the whole rows into; its first column is returned."""
        return self.stats(img, ref, clip=clip, out=out)[:, 0]

    def scales(self, img, ref, clip=True):
        """-> float64 [n,4,2]: (num_s, den_s) of each scale."""
        rows = self.stats(img, ref, clip=clip)
        return torch.stack([rows[:, 1:5], rows[:, 5:9]], dim=2)


HISTEQ_MODES ={'none': 0, 'global': 1, 'local': 2, 'clahe': 3}
_histeq_ws = {}


def histogram_equalization(img, mode):
    """EvalMetricsTracker.histogram_equalization (utils/eval_metrics.py:326-350) on cuda tensors [N,H,W] already clipped
    to [0,1], in place.  'none' returns the input; an unknown name raises like the reference."""
    if mode not in HISTEQ_MODES:
        raise ValueError(f"Unrecognized histogram equalization argument: {mode}")
    if mode == 'none':
        return img
    lib = _lib.load()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
    v = img if img.dim() == 3 else img.unsqueeze(0)
    n, H, W = v.shape
    code = HISTEQ_MODES[mode]
    need = lib.evr_hist_equalize_workspace_bytes(n, H, W, code)
    ws = _histeq_ws.get(img.device)
    if need and (ws is None or ws.numel() < need):
        ws = _histeq_ws[img.device] = torch.empty(int(need), dtype=torch.uint8, device=img.device)
    _lib.check(lib.evr_hist_equalize(_lib.ptr(v), n, H, W, code, _lib.ptr(ws) if need else None, int(need),
                                     _lib.stream_ptr()), 'evr_hist_equalize')
    return img
