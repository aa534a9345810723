"""Oracle: DISTS on torch-CPU.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED.  The reference obtains the metric from pyiqa (`pyiqa.create_metric('dists')`, utils/eval_metrics.py:115) on inputs
built by cv2torch(img, num_ch=3) (utils/eval_utils.py:46-54); pyiqa is not in the reference tree, not installed, and the weights are
downloaded at run time.  This restates the published algorithm (Ding, Ma, Wang, Simoncelli, "Image Quality Assessment: Unifying
Structure and Texture Similarity", 2020; dingkeyan93/DISTS, which pyiqa wraps), recalled from the published code, not read from it:

  1. x = the gray frame in [0,1] on three channels; h = (x - mean_c)/std_c.
  2. Five VGG-16 stages (3x3 convolutions, padding 1, ReLU); stages 2-5 begin with an L2 pool:
     sqrt(conv2d(f^2, k, stride 2, padding 1, depthwise) + 1e-12), k = (0.5, 1, 0.5) x (0.5, 1, 0.5) / its sum, zero padding:
     output side (s + 1) // 2.
  3. Six feature sets: x (before the normalisation), relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (3 + 64 + 128 + 256 + 512 + 512 = 1475
     channels).
  4. Per set and channel over the spatial positions: mx, my, vx = mean((fx - mx)^2), vy, cxy = mean(fx fy) - mx my (two-pass variance,
     as the published code), S1 = (2 mx my + c1)/(mx^2 + my^2 + c1), S2 = (2 cxy + c2)/(vx + vy + c2), c1 = c2 = 1e-6.
  5. w = sum(alpha) + sum(beta); score = 1 - (sum (alpha_c/w) S1_c + sum (beta_c/w) S2_c).
Unpinned until tests/test_dists_pins.py has run where pyiqa exists: all of the above and the state-dict names stage1.{0,2},
stage2.{5,7}, stage3.{10,12,14}, stage4.{17,19,21}, stage5.{24,26,28} (.weight, .bias), alpha, beta ([1,1475,1,1]), mean, std.

`dtype`: torch.float64 is the truth; torch.float32 gives the reference arithmetic's own error on the same inputs.
"""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# (stage, torchvision index of its convolutions)
STAGES = [(1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28))]
CHANNELS = (3, 64, 128, 256, 512, 512)
MIN_SIDE = 16
C1 = C2 = 1e-6


def l2pool(x):
    """[n,C,h,w] -> [n,C,(h+1)//2,(w+1)//2]."""
    a = torch.tensor([0.5, 1.0, 0.5], dtype=x.dtype)
    k = a[:, None] * a[None, :]
    k = (k / k.sum())[None, None].repeat(x.shape[1], 1, 1, 1)
    return torch.sqrt(F.conv2d(x ** 2, k, stride=2, padding=1, groups=x.shape[1]) + 1e-12)


def three_channels(a, dtype):
    """gray [n,H,W] -> [n,3,H,W], not normalised."""
    return torch.as_tensor(np.asarray(a)).to(dtype).unsqueeze(1).repeat(1, 3, 1, 1)


def normalise(x, sd=None):
    mean = sd['mean'].reshape(-1) if sd is not None and 'mean' in sd else torch.tensor(MEAN, dtype=x.dtype)
    std = sd['std'].reshape(-1) if sd is not None and 'std' in sd else torch.tensor(STD, dtype=x.dtype)
    return (x - mean.to(x.dtype).view(1, 3, 1, 1)) / std.to(x.dtype).view(1, 3, 1, 1)


def features(sd, x):
    """x: [n,3,H,W] in [0,1].  Returns the six feature sets."""
    outs = [x]
    h = normalise(x, sd)
    for s, idxs in STAGES:
        if s > 1:
            h = l2pool(h)
        for i in idxs:
            h = torch.relu(F.conv2d(h, sd[f'stage{s}.{i}.weight'], sd[f'stage{s}.{i}.bias'], stride=1, padding=1))
        outs.append(h)
    return outs


def similarities(fx, fy):
    """-> (S1, S2), [n,C] each, of one feature set."""
    mx, my = fx.mean(dim=(2, 3), keepdim=True), fy.mean(dim=(2, 3), keepdim=True)
    s1 = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)
    vx, vy = ((fx - mx) ** 2).mean(dim=(2, 3), keepdim=True), ((fy - my) ** 2).mean(dim=(2, 3), keepdim=True)
    cxy = (fx * fy).mean(dim=(2, 3), keepdim=True) - mx * my
    s2 = (2 * cxy + C2) / (vx + vy + C2)
    return s1.flatten(1), s2.flatten(1)


def stage_distances(f0, f1, alpha, beta):
    """-> (score [n], distances [n,6,2]) of the dtype of the features: distances[b][k] = (sum (alpha_c/w)(1 - S1_c),
    sum (beta_c/w)(1 - S2_c)) over the channels of set k."""
    w = alpha.sum() + beta.sum()
    al, be = torch.split(alpha.reshape(-1) / w, CHANNELS), torch.split(beta.reshape(-1) / w, CHANNELS)
    d1 = d2 = 0
    cols = []
    for k in range(6):
        s1, s2 = similarities(f0[k], f1[k])
        d1 = d1 + (al[k][None] * s1).sum(dim=1)
        d2 = d2 + (be[k][None] * s2).sum(dim=1)
        cols.append(torch.stack([(al[k][None] * (1 - s1)).sum(dim=1), (be[k][None] * (1 - s2)).sum(dim=1)], dim=1))
    return 1 - (d1 + d2), torch.stack(cols, dim=1)


def dists(sd, img, ref, dtype=torch.float64):
    """img, ref: float32 [n,H,W] in [0,1] (gray).  Returns (totals [n], per-set distances [n,6,2]) as float64 arrays."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}
    with torch.no_grad():
        f0, f1 = features(sd, three_channels(img, dtype)), features(sd, three_channels(ref, dtype))
        total, stages = stage_distances(f0, f1, sd['alpha'], sd['beta'])
    return total.double().numpy(), stages.double().numpy()


def frame_pairs(H, W, seed=7):
    """Four pairs -> img, ref [4,H,W]: 0 identical; 1 a contrast and brightness change plus noise; 2 a gamma change plus noise against
    the vertically flipped frame; 3 ones against zeros (conv1_1's border term; a real mean difference for the input's feature set)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.stack([0.5 + 0.4 * np.sin(xx / (7.0 + i)) * np.cos(yy / (9.0 + i)) for i in range(3)]).astype(np.float32)
    ref = np.clip(ref + 0.05 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    img = np.empty_like(ref)
    img[0] = ref[0]
    img[1] = np.clip(0.7 * ref[1] + 0.05 + 0.05 * rng.standard_normal((H, W)), 0, 1)
    img[2] = np.clip(ref[2][::-1] ** 1.6 + 0.05 * rng.standard_normal((H, W)), 0, 1)
    img = np.concatenate([img, np.ones((1, H, W), np.float32)])
    ref = np.concatenate([ref, np.zeros((1, H, W), np.float32)])
    return img.astype(np.float32), ref.astype(np.float32)
