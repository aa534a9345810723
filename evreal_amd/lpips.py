"""Host side of the LPIPS metric (evr_lpips_*): pyiqa.create_metric('lpips') stand-in on the GPU."""
import ctypes

import numpy as np
import torch

from . import lib as _lib


def _tensor_table(state_dict):
    """-> (ctypes array of evr_tensor, the host arrays it points into) for a state dict of tensors or arrays."""
    sd = {k: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
          for k, v in state_dict.items()}
    tensors = (_lib.Tensor * len(sd))()
    keep = []
    for i, (k, v) in enumerate(sd.items()):
        name = k.encode(); keep.append((name, v))
        tensors[i].name = name
        tensors[i].data_host = v.ctypes.data_as(ctypes.c_void_p)
        tensors[i].ndim = v.ndim
        for d in range(v.ndim):
            tensors[i].shape[d] = v.shape[d]
    return tensors, keep


class _Backbone:
    """What the backbone handles (LPIPS, LPIPSVGG, DISTS) share: `_entry` is the prefix of the backbone's C entry points."""
    _entry = None

    def _create(self, state_dict, *args):
        _lib.require_gpu()
        self.lib = _lib.load()
        tensors, self._keep = _tensor_table(state_dict)
        h = ctypes.c_void_p()
        self.handle = None
        _lib.check(getattr(self.lib, self._entry + '_create')(tensors, len(tensors), *args, ctypes.byref(h)), self._entry + '_create')
        self.handle = h

    @staticmethod
    def _inputs(img, ref, out):
        """-> the frames contiguous, and `out` or a new double [n] for the scores."""
        assert img.is_cuda and ref.is_cuda and img.shape == ref.shape and img.dim() == 3
        if out is None:
            out = torch.empty(img.shape[0], dtype=torch.float64, device=img.device)
        return img.contiguous(), ref.contiguous(), out

    def flops(self):
        return float(getattr(self.lib, self._entry + '_flops')(self.handle))

    def __del__(self):
        try:
            if self.handle is not None:
                getattr(self.lib, self._entry + '_destroy')(self.handle); self.handle = None
        except Exception:
            pass


class LPIPS(_Backbone):
    _entry = 'evr_lpips'

    def __init__(self, state_dict):
        self._create(state_dict)

    def __call__(self, img, ref, clip=True, out=None):
        """img, ref: cuda fp32 [n,H,W] in [0,1] -> double [n] on device."""
        img, ref, out = self._inputs(img, ref, out)
        n, H, W = img.shape
        _lib.check(self.lib.evr_lpips_forward(self.handle, _lib.ptr(img), _lib.ptr(ref), n, H, W, 1 if clip else 0,
                                              _lib.ptr(out), _lib.stream_ptr()), 'evr_lpips_forward')
        return out


class _VggTrunkMetric(_Backbone):
    """The metrics on the VGG-16 trunk (csrc/vgg_trunk.h): their entry points have one shape.

    max_pairs: frame pairs per pass (0: as many as keep the handle's two activation buffers within 1 GiB); a call with more pairs
    runs in passes."""
    # the trunk's kernels run down to the 1x1 maps of a 16x16 frame: LPIPS-VGG's four floor-mode 2x2 pools must leave one pixel
    # (pyiqa's dists would accept smaller frames)
    MIN_SIDE = 16
    _too_small = None       # the metric's sentence, with {m} for MIN_SIDE and {H}, {W}

    def __init__(self, state_dict, max_pairs=0):
        self._create(state_dict, int(max_pairs))

    @classmethod
    def too_small(cls, H, W):
        """The message of the exception the metric raises on frames of this size, or None where it is defined."""
        if min(H, W) >= cls.MIN_SIDE:
            return None
        return cls._too_small.format(m=cls.MIN_SIDE, H=H, W=W)

    def _forward(self, img, ref, clip, out, parts):
        """parts: None, or the device array of the per-layer / per-stage distances to fill."""
        img, ref, out = self._inputs(img, ref, out)
        assert img.dtype == ref.dtype == torch.float32
        n, H, W = img.shape
        if self.too_small(H, W):
            raise ValueError(self.too_small(H, W))          # decided from the shape: no launch is tried
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == n
        _lib.check(getattr(self.lib, self._entry + '_forward')(self.handle, _lib.ptr(img), _lib.ptr(ref), n, H, W, 1 if clip else 0,
                                                               _lib.ptr(out), _lib.ptr(parts), _lib.stream_ptr()), self._entry + '_forward')
        return out

    def saturation(self):
        """Output runs that left the exact range of the arithmetic mode's activation format since the last call (the counter is
        cleared); waits for the current stream."""
        c = ctypes.c_int64(0)
        _lib.check(getattr(self.lib, self._entry + '_saturation')(self.handle, ctypes.byref(c), _lib.stream_ptr()),
                   self._entry + '_saturation')
        return int(c.value)


class LPIPSVGG(_VggTrunkMetric):
    """pyiqa.create_metric('lpips-vgg') stand-in on the GPU (evr_lpips_vgg_*): same call shape as LPIPS."""
    _entry = 'evr_lpips_vgg'
    _too_small = "lpips-vgg needs frames of at least {m}x{m} pixels (VGG-16 pools 2x2 four times), got {H}x{W}"

    def __call__(self, img, ref, clip=True, out=None):
        """img, ref: cuda fp32 [n,H,W] in [0,1] -> double [n] on device."""
        return self._forward(img, ref, clip, out, None)

    def layers(self, img, ref, clip=True):
        """-> double [n,5]: the distances of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (their sum is the score)."""
        layers = torch.empty((img.shape[0], 5), dtype=torch.float64, device=img.device)
        self._forward(img, ref, clip, None, layers)
        return layers


class DISTS(_VggTrunkMetric):
    """pyiqa.create_metric('dists') stand-in on the GPU (evr_dists_*): same call shape as LPIPSVGG, on the same VGG-16 trunk."""
    _entry = 'evr_dists'
    _too_small = "dists needs frames of at least {m}x{m} pixels on this VGG-16 trunk, got {H}x{W}"

    def __call__(self, img, ref, clip=True, out=None):
        """img, ref: cuda fp32 [n,H,W] in [0,1] -> double [n] on device: 1 - (D1 + D2)."""
        return self._forward(img, ref, clip, out, None)

    def stages(self, img, ref, clip=True):
        """-> double [n,6,2]: the structure ([..., 0]) and texture ([..., 1]) distances of the six feature sets -- the input, relu1_2,
        relu2_2, relu3_3, relu4_3, relu5_3; their sum is the score up to rounding."""
        stages = torch.empty((img.shape[0], 6, 2), dtype=torch.float64, device=img.device)
        self._forward(img, ref, clip, None, stages)
        return stages


