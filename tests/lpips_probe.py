"""Inputs, lin-head variants, references and injected errors for the per-layer tests of the AlexNet LPIPS (csrc/lpips.hip):
tests/test_lpips_probe_cpu.py checks on the CPU that these inputs notice each class of error, tests/test_gpu_lpips_probe.py holds the
kernels to them.  Nothing here touches the GPU.

LPIPS is a difference of two feature sets that went through the same kernels, averaged over the pixels and summed over five layers:
an error made on both images alike cancels to first order, a border pixel is one among thousands, and a layer's own error hides in
the sum.  So the inputs here are small maps (every pixel near a border or a tile seam), pairs that do not cancel (texture against a
constant) or whose interior cancels exactly (only a frame differs), and lin heads that leave one layer, or one 4-channel run of it.

SHAPES (relu1, pool1 = relu2, pool2 = relu3..5):
  35 x 47     8x11, 3x5, 1x2    relu3..5 have two pixels, every conv1 pixel is at or next to a border, conv3..5 far below one tile
  71 x 99     17x24, 8x11, 3x5  2 x 2 conv1 tiles (one-row second tile row, 8-column second tile column, seam at row / column 16);
                                pool1 drops relu1's last column
  135 x 139   33x34, 16x16, 7x7 3 x 3 conv1 tiles, tile (1,1) interior (62 + 71 = 133 <= 135, 139): the folded bias of the direct
                                kernel; 33 * 34 = 1122 pixels end the score kernel's four-pixels-per-wave path on a ragged group
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = [(35, 47), (71, 99), (135, 139)]
CHANNELS = [64, 192, 384, 256, 256]
NPAIRS = 5
FRAME = 12         # pair 4: width of the inverted frame (6 left the 4-channel scores of relu3..5 at 135 x 139 under 1e-3)
SEED = 3           # of the synthetic weights, as in the neighbouring LPIPS tests
VARIANTS = [f'{kind}_{l}' for l in range(5) for kind in ('only', 'tail')]
_CACHE = {}


def pairs(shape):
    """-> img, ref float32 [5, H, W]: (0) identical, (1) texture / another texture, (2) texture / zeros, (3) ones / texture,
    (4) a texture against itself with a FRAME-pixel frame inverted (every pixel whose window lies inside contributes exactly 0).
    Pairs 2 and 3 make conv1's padding term (wb, wbsum) a first-order part of the score.  Textures are uniform-random per pixel in
    [0, 1); the other texture of pair 1 in [0, 0.3) and that of pair 4 in [0, 0.1) (its frame then in (0.9, 1]): two white-noise
    textures of one range differ so little behind the synthetic weights that a 4-channel score of relu3..5 fell to 1e-4, where the
    gate's absolute term would start to carry it (tests/test_lpips_probe_cpu.py holds every gated score to >= 1e-3)."""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    t = rng.random((6, H, W), dtype=np.float32)
    img, ref = np.empty((NPAIRS, H, W), np.float32), np.empty((NPAIRS, H, W), np.float32)
    img[0] = ref[0] = t[0]
    img[1], ref[1] = t[1], 0.3 * t[2]
    img[2], ref[2] = t[3], 0.0
    img[3], ref[3] = 1.0, t[4]
    ref[4] = 0.1 * t[5]
    img[4] = 1.0 - ref[4]
    img[4, FRAME:H - FRAME, FRAME:W - FRAME] = ref[4, FRAME:H - FRAME, FRAME:W - FRAME]
    return img, ref


def base_state_dict():
    if 'sd' not in _CACHE:
        from evreal_amd import weights
        _CACHE['sd'] = weights.synth_lpips_state_dict(seed=SEED)
    return _CACHE['sd']


def variant(name):
    """The state dict of `only_l` (every lin head but layer l's zero: the score is that layer's) or `tail_l` (as only_l, lin_l zero but
    for its last four channels at 1.0: one 4-channel run, the last of a PLAIN row for relu1, of the last PACKED group for relu2..5)."""
    kind, l = name.split('_')
    l = int(l)
    sd = OrderedDict((k, np.array(v, copy=True)) for k, v in base_state_dict().items())
    for k in range(5):
        w = sd[f'lin{k}.model.1.weight']
        if k != l:
            w[...] = 0.0
        elif kind == 'tail':
            w[...] = 0.0
            w.reshape(-1)[-4:] = 1.0
        else:
            assert kind == 'only', name
    return sd


def reference(shape, name):
    """(want64, want32) of oracle.lpips.lpips on pairs(shape) with variant(name): computed once, never modified."""
    key = ('ref', tuple(shape), name)
    if key not in _CACHE:
        from oracle import lpips as ol
        img, ref = pairs(shape)
        sd = variant(name)
        w64, w32 = ol.lpips(sd, img, ref, torch.float64), ol.lpips(sd, img, ref, torch.float32)
        w64.setflags(write=False); w32.setflags(write=False)
        _CACHE[key] = (w64, w32)
    return _CACHE[key]


# ---- the oracle's arithmetic restated in float64, with hooks for deliberate errors -----------------------------------------------
# Each error is one a kernel of lpips.hip (or the conv / pool it launches) could make and stay inside today's gates.  The first four
# are the rows of the table in tests/test_lpips_probe_cpu.py.
ERRORS = OrderedDict([
    ('conv2_pixel00_from_neighbour', 'conv2 output pixel (0,0) takes the value of pixel (0,1)'),
    ('conv5_bias_lost_last4', 'conv5 bias lost on its last 4 channels'),
    ('relu1_score_skips_last_pixel', "relu1's score leaves out its last pixel"),
    ('conv1_last_col_loses_tap_col', "conv1's last output column loses the image's last column from its window"),
    ('conv1_pad_is_gray0', "conv1's padding holds the affine image of gray 0 instead of 0"),
    ('relu1_row16_from_row15', 'relu1 output row 16 is a copy of row 15 (tile seam)'),
    ('conv1_interior_bias_one_tap', "conv1's folded bias is wrong by one tap's wb on interior-tile pixels only"),
    ('pool1_last_col_2x2', 'pool1 uses a 2x2 window in its last output column'),
    ('pair_scored_against_next_ref', 'pair i is scored against the reference of pair i + 1'),
    # further ones, from reading the kernels
    ('relu1_score_drops_ragged_group', "relu1's score drops the last hw % 4 pixels (four pixels per wave)"),
    ('score_second_run_lin_aliased', "a lane's second 4-channel run (channels >= 256) takes the lin weights of its first"),
    ('pool2_last_row_2x2', 'pool2 uses a 2x2 window in its last output row'),
    ('conv1_col16_from_col15', 'relu1 output column 16 is a copy of column 15 (tile seam)'),
    ('packed_group_last4_from_first4', "relu2..5: the last 4-channel run of the last 16-channel group holds the group's first run"),
])
TABLE_ERRORS = list(ERRORS)[:4]

_NAMES = ["net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10"]
_STRIDE_PAD = [(4, 2), (1, 2), (1, 1), (1, 1), (1, 1)]
_SHIFT = (-.030, -.088, -.188)
_SCALE = (.458, .448, .450)


def _pool(x, two_by_two_last=None):
    y = F.max_pool2d(x, kernel_size=3, stride=2)
    if two_by_two_last is not None:
        z = F.max_pool2d(x, kernel_size=2, stride=2)
        if two_by_two_last == 'col':
            y[..., :, -1] = z[..., :y.shape[-2], y.shape[-1] - 1]
        else:
            y[..., -1, :] = z[..., y.shape[-2] - 1, :y.shape[-1]]
    return y


def _features(sd, g, error):
    """g: [n, H, W] float64 gray -> the five relu outputs, as oracle.lpips.features computes them but for `error`."""
    dt = torch.float64
    shift, scale = (torch.tensor(c, dtype=dt).view(1, 3, 1, 1) for c in (_SHIFT, _SCALE))
    x = ((2 * g.unsqueeze(1).repeat(1, 3, 1, 1) - 1) - shift) / scale
    beta = ((-1.0 - shift) / scale)                              # the affine image of gray 0
    H, W = g.shape[-2:]
    outs = []
    for i, (name, (stride, pad)) in enumerate(zip(_NAMES, _STRIDE_PAD)):
        w, b = sd[name + '.weight'], sd[name + '.bias']
        if i == 1:
            x = _pool(x, 'col' if error == 'pool1_last_col_2x2' else None)
        if i == 2:
            x = _pool(x, 'row' if error == 'pool2_last_row_2x2' else None)
        if i == 4 and error == 'conv5_bias_lost_last4':
            b = b.clone(); b[-4:] = 0.0
        if i == 0 and error == 'conv1_pad_is_gray0':
            xp = beta.expand(x.shape[0], 3, H + 4, W + 4).clone()
            xp[..., 2:-2, 2:-2] = x
            y = F.conv2d(xp, w, b, stride=stride, padding=0)
        else:
            y = F.conv2d(x, w, b, stride=stride, padding=pad)
        if i == 0 and error == 'conv1_last_col_loses_tap_col':
            x2 = x.clone(); x2[..., W - 1] = 0.0
            y[..., -1] = F.conv2d(x2, w, b, stride=stride, padding=pad)[..., -1]
        if i == 0 and error == 'conv1_interior_bias_one_tap':
            wb0 = (w[:, :, 0, 0] * beta.view(1, 3)).sum(dim=1)   # [64]: tap (0,0) of the padding term
            for ty in range((y.shape[-2] + 15) // 16):
                for tx in range((y.shape[-1] + 15) // 16):
                    if ty * 64 - 2 >= 0 and tx * 64 - 2 >= 0 and ty * 64 - 2 + 71 <= H and tx * 64 - 2 + 71 <= W:
                        y[..., ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] += wb0.view(1, -1, 1, 1)
        x = torch.relu(y)
        if i == 0 and error == 'relu1_row16_from_row15' and x.shape[-2] > 16:
            x[..., 16, :] = x[..., 15, :]
        if i == 0 and error == 'conv1_col16_from_col15' and x.shape[-1] > 16:
            x[..., :, 16] = x[..., :, 15]
        if i == 1 and error == 'conv2_pixel00_from_neighbour':
            x[..., 0, 0] = x[..., 0, 1]
        if i >= 1 and error == 'packed_group_last4_from_first4':
            x[:, -4:] = x[:, -16:-12]
        outs.append(x)
    return outs


def channel_means(img, ref, error=None):
    """-> five float64 arrays [n, C_l]: per layer and channel, the spatial mean of the squared difference of the unit-normalised
    features -- what a lin head then weighs.  The heads are applied by `scores`, so one pass serves every variant."""
    sd = {k: torch.as_tensor(v).to(torch.float64) for k, v in base_state_dict().items()}
    ref = np.asarray(ref)
    if error == 'pair_scored_against_next_ref':
        ref = np.roll(ref, -1, axis=0)
    with torch.no_grad():
        f0 = _features(sd, torch.as_tensor(np.asarray(img)).to(torch.float64), error)
        f1 = _features(sd, torch.as_tensor(ref).to(torch.float64), error)
        out = []
        for l, (a, b) in enumerate(zip(f0, f1)):
            an = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
            bn = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
            d = ((an - bn) ** 2).flatten(2)                      # [n, C, hw]
            hw = d.shape[-1]
            if l == 0 and error == 'relu1_score_skips_last_pixel':
                d = d[..., :hw - 1]
            if l == 0 and error == 'relu1_score_drops_ragged_group':
                d = d[..., :hw - hw % 4]
            out.append((d.sum(dim=2) / hw).numpy())
    return out


def scores(means, sd, error=None):
    """The LPIPS scores [n] of the state dict `sd` (a variant, or the base) from channel_means' output."""
    total = 0.0
    for l, m in enumerate(means):
        w = np.asarray(sd[f'lin{l}.model.1.weight'], dtype=np.float64).reshape(-1)
        if error == 'score_second_run_lin_aliased' and w.size > 256:
            w = w.copy(); w[256:] = w[:w.size - 256]
        total = total + m @ w
    return total
