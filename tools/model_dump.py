#!/usr/bin/env python
"""Dump what one golden model configuration computes, byte for byte, and compare two dumps.

    python tools/model_dump.py TAG OUT.npz [--n-seq N] [--debug-taps]
    python tools/model_dump.py --compare A.npz B.npz

The model is rebuilt as tests/test_gpu_model.py builds it (the golden's weights, its synthetic voxels), all frames of the golden
run, and OUT.npz gets every frame's image, after the last frame every debug name the family defines, the arithmetic the library
settled on and its FLOPs per step.  One configuration per process; the arithmetic comes from the environment (EVR_ARITH / EVR_FP32)
and the library from EVR_LIB, so two builds of the library are compared by dumping each and running --compare: a refactor of the
executor (csrc/model.cpp) must leave every array byte-identical.

TAG: firenet firenetplus | e2vid_bn e2vid_plus e2vid_gru_tiny e2vid_in e2vid_hyper e2vid_hyper_in | spade | etnet etnet_bn etnet_in
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

FIRE = ('firenet', 'firenetplus')
E2VID = ('e2vid_bn', 'e2vid_plus', 'e2vid_gru_tiny', 'e2vid_in', 'e2vid_hyper', 'e2vid_hyper_in')
ETNET = {'etnet': None, 'etnet_bn': 'BN', 'etnet_in': 'IN'}
TAGS = FIRE + E2VID + ('spade',) + tuple(ETNET)


def build(tag, debug_taps):
    """-> (model, voxels [F,B,H,W], debug names of the family)"""
    from evreal_amd import model, synth, weights
    z = np.load(os.path.join(GOLDEN, f'{tag}_seq.npz'), allow_pickle=False)
    seed, F, B, H, W = [int(v) for v in z['voxel_args']]
    if tag in FIRE:
        w = np.load(os.path.join(GOLDEN, f'{tag}_weights.npz'), allow_pickle=False)
        sd = {k: w[k] for k in w.files}
        if tag == 'firenet':
            m = model.FireNet_legacy(unet_kwargs=dict(num_bins=5, skip_type='no_skip', recurrent_block_type='convgru',
                                                      base_num_channels=16, num_residual_blocks=2,
                                                      recurrent_blocks={'resblock': [0]}, kernel_size=3, norm='none'))
        else:
            m = model.FireNet(num_bins=5, base_num_channels=16, kernel_size=3)
        vox = synth.sparse_voxels(seed, F, B, H, W)
        names = ['head', 'h0', 'h1', 'res0', 'res1']
    elif tag in E2VID:
        kw = json.loads(bytes(z['kwargs']).decode())
        fixed = {k[6:]: z[k] for k in z.files if k.startswith('fixed.')}
        sd = weights.synth_state_dict(weights.unet_recurrent_schema(**kw), seed=int(z['seed']), fixed=fixed)
        m = model.E2VIDRecurrent(kw)
        vox = synth.sparse_voxels(seed, F, B, H, W)
        E, R = kw['num_encoders'], kw['num_residual_blocks']
        names = ['head'] + [f'enc{i}.conv' for i in range(E)] + [f'h{i}' for i in range(E)]
        if kw['recurrent_block_type'] == 'convlstm':
            names += [f'c{i}' for i in range(E)]
        names += [f'res{i}' for i in range(R)] + [f'dec{i}' for i in range(E)]
        if kw.get('use_dynamic_decoder'):
            names += ['ctx', 'coeff']
        if kw['use_upsample_conv']:
            names += [f'dec{i}.up' for i in range(E) if not (i == 0 and kw.get('use_dynamic_decoder'))]
    elif tag == 'spade':
        sd = weights.synth_state_dict(weights.spade_e2vid_schema(), seed=int(z['seed']))
        m = model.SpadeE2vid()
        vox = synth.sparse_voxels(seed, F, B, H, W, density=0.15)
        names = ['head'] + [f'h{i}' for i in range(4)] + [f'c{i}' for i in range(4)] + ['res0', 'res1', 'up0', 'up1']
    else:
        norm = ETNET[tag]
        sd = weights.synth_state_dict(weights.etnet_schema(norm=norm), seed=int(z['seed']))
        m = model.EITR({'num_bins': 5, 'norm': norm})
        vox = synth.sparse_voxels(seed, F, B, H, W, density=0.15)
        names = ['head'] + [f'h{i}' for i in range(3)] + [f'c{i}' for i in range(3)] + ['hs_trans', 'dec0', 'dec1', 'dec2']
    assert weights.state_dict_digest(sd) == str(z['weights_sha']), 'the golden was made from other weights'
    m.debug_taps = debug_taps
    m.load_state_dict(sd)
    return m, vox, names


def dump(tag, out, n_seq, debug_taps):
    import torch
    m, vox, names = build(tag, debug_taps)
    arrays = {}
    m.reset_states()
    for f in range(vox.shape[0]):
        x = torch.from_numpy(vox[f:f + 1]).cuda().repeat(n_seq, 1, 1, 1)
        arrays[f'image.{f}'] = m(x)['image'].cpu().numpy()
    for name in names:
        arrays[f'tensor.{name}'] = m.read_tensor(name).cpu().numpy()
    arrays['arith'] = np.array(m.arith)
    arrays['flops_per_step'] = np.array(m.flops_per_step())
    np.savez(out, **arrays)
    print(f'{tag}: arith {m.arith}, {vox.shape[0]} frames x {n_seq} sequences, {len(names)} tensors -> {out}')


def compare(a_path, b_path):
    a, b = np.load(a_path, allow_pickle=False), np.load(b_path, allow_pickle=False)
    differ = 0
    for k in sorted(set(a.files) | set(b.files)):
        if k not in a.files or k not in b.files:
            print(f'{k:24s} only in {a_path if k in a.files else b_path}')
            differ += 1
        elif a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes():
            print(f'{k:24s} equal bytes ({a[k].nbytes})')
        elif a[k].shape != b[k].shape or a[k].dtype.kind not in 'fiu':
            print(f'{k:24s} DIFFERS: {a[k].dtype}{a[k].shape} {a[k] if a[k].ndim == 0 else ""} / {b[k].dtype}{b[k].shape} {b[k] if b[k].ndim == 0 else ""}')
            differ += 1
        else:
            print(f'{k:24s} DIFFERS: max abs {np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max():.3e}')
            differ += 1
    print(f'{differ} of {len(set(a.files) | set(b.files))} arrays differ')
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('args', nargs=2, metavar='ARG', help='TAG OUT.npz, or with --compare: A.npz B.npz')
    ap.add_argument('--compare', action='store_true')
    ap.add_argument('--n-seq', type=int, default=1)
    ap.add_argument('--debug-taps', action='store_true', help='keep every intermediate readable, as the single-sequence tests do')
    o = ap.parse_args()
    if o.compare:
        return compare(*o.args)
    if o.args[0] not in TAGS:
        ap.error(f'unknown tag {o.args[0]!r}: one of {" ".join(TAGS)}')
    dump(o.args[0], o.args[1], o.n_seq, o.debug_taps)
    return 0


if __name__ == '__main__':
    sys.exit(main())
