"""Oracle: LPIPS (VGG-16 backbone, v0.1) on torch-CPU.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED.  The reference obtains the metric from pyiqa (`pyiqa.create_metric('lpips-vgg')`, utils/eval_metrics.py:115)
on inputs built by cv2torch(img, num_ch=3) (utils/eval_utils.py:46-54); pyiqa and torchvision are not in the reference tree, not
installed, and the weights are downloaded at run time.  This restates the published algorithm (Zhang et al., CVPR 2018;
richzhang/PerceptualSimilarity v0.1 with net='vgg', which pyiqa wraps): inputs in [0,1] -> 2x-1 -> (x - shift)/scale ->
torchvision vgg16.features with taps after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 -> channel-unit-normalised features
(f/(|f| + 1e-10)) -> squared difference -> non-negative 1x1 'lin' weights -> spatial mean -> sum over the five layers.
Conventions that stay unpinned until tests/test_lpips_vgg_pins.py has run where pyiqa exists -- recalled from the published code,
not read from it: the state-dict names net.slice1.{0,2}, net.slice2.{5,7}, net.slice3.{10,12,14}, net.slice4.{17,19,21},
net.slice5.{24,26,28} (.weight, .bias) and lin{0..4}.model.1.weight (64, 128, 256, 512, 512 elements), and the pool positions
(torchvision indices 4, 9, 16, 23: MaxPool2d(2, 2) in floor mode is the first operation of slices 2-5).

`dtype`: torch.float64 is the truth; torch.float32 gives the reference arithmetic's own error on the same inputs.
"""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (slice, torchvision index of its convolutions)
SLICES = [(1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28))]
CHANNELS = (64, 128, 256, 512, 512)
MIN_SIDE = 16


def prep(a, dtype):
    """gray [n,H,W] in [0,1] -> the scaled three-channel input [n,3,H,W]."""
    x = 2 * torch.as_tensor(np.asarray(a)).to(dtype).unsqueeze(1).repeat(1, 3, 1, 1) - 1
    return (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)


def features(sd, x):
    """x: [n,3,H,W] already scaled.  Returns relu1_2, relu2_2, relu3_3, relu4_3, relu5_3."""
    outs = []
    for s, idxs in SLICES:
        if s > 1:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for i in idxs:
            x = torch.relu(F.conv2d(x, sd[f'net.slice{s}.{i}.weight'], sd[f'net.slice{s}.{i}.bias'], stride=1, padding=1))
        outs.append(x)
    return outs


def distances(f0, f1, lins):
    """-> [n,5] of the dtype of the features."""
    cols = []
    for a, b, w in zip(f0, f1, lins):
        an = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
        bn = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
        cols.append((((an - bn) ** 2) * w.view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(cols, dim=1)


def lpips_vgg(sd, img, ref, dtype=torch.float64):
    """img, ref: float32 [n,H,W] in [0,1] (gray).  Returns (totals [n], per-layer distances [n,5]) as float64 arrays."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}
    with torch.no_grad():
        f0, f1 = features(sd, prep(img, dtype)), features(sd, prep(ref, dtype))
        d = distances(f0, f1, [sd[f'lin{l}.model.1.weight'] for l in range(5)]).double()
    return d.sum(dim=1).numpy(), d.numpy()


def frame_pairs(H, W, n=3, seed=7):
    """The sinusoid-plus-noise frames of test_lpips_vs_oracle (pair 0 identical) + one zeros-versus-ones pair -> img, ref [n+1,H,W]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.stack([0.5 + 0.4 * np.sin(xx / (7.0 + i)) * np.cos(yy / (9.0 + i)) for i in range(n)]).astype(np.float32)
    img = np.clip(ref + 0.1 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    img[0] = ref[0]
    img = np.concatenate([img, np.zeros((1, H, W), np.float32)])
    ref = np.concatenate([ref, np.ones((1, H, W), np.float32)])
    return img, ref
