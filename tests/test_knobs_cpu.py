"""The library's run-time switches outside the conv dispatch, without a GPU: csrc/knobs.cpp is pure host code, so tests/knobs_cpu.cpp --
a program with its own main() -- is compiled against it alone with build.py's hipcc and the LibKnobs table it prints for each
environment is compared, field by field, with tests/golden/lib_knobs.json: nothing set, every switch at "0", "1", empty and a
non-number, and the values with a meaning of their own (negative numbers, the arithmetic names, two switches together).  The
environment is a map inside the program, never the process's.

The second half keeps README.md's "Run-time switches" and the table in step with the code: every EVR_* / EVREAL_* name the package
quotes is in the README, and nothing under csrc/ but knobs.cpp and conv_knobs() reads the environment."""
import json
import os
import re
import subprocess

import pytest

from evreal_amd import build as evr_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'evreal_amd')
CSRC = os.path.join(PKG, 'csrc')

needs_hipcc = pytest.mark.skipif(not os.path.exists(evr_build.HIPCC), reason='no hipcc')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('knobs') / 'knobs_cpu')
    cmd = [evr_build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-I' + CSRC, '-Wall', '-Werror',
           '-x', 'hip', os.path.join(ROOT, 'tests', 'knobs_cpu.cpp'), os.path.join(CSRC, 'knobs.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # (the program must not look at the process's environment: give it switches that would change every row if it did)
    env = dict({k: v for k, v in os.environ.items() if not k.startswith(('EVR_', 'EVREAL_'))}, EVR_FP32='1', EVR_WINO='0', EVR_ABLATE='7')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return {d.pop('id'): d for d in map(json.loads, r.stdout.splitlines())}


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'lib_knobs.json')) as fh:
        return {k: v for k, v in json.load(fh).items() if not k.startswith('_')}


@needs_hipcc
def test_every_row_matches_the_golden_table(rows, golden):
    assert sorted(rows) == sorted(golden)
    assert rows['empty'] == golden['empty']
    wrong = {rid: (rows[rid], want) for rid, want in golden.items() if rows[rid] != dict(golden['empty'], **want)}
    assert not wrong, wrong


@needs_hipcc
def test_the_defaults(rows):
    d = rows['empty']
    assert (d['arith'], d['group_store'], d['wino_blocks'], d['head_wlds'], d['head_blocks']) == (3, 1, 256, 0, 512)
    assert (d['lpips_band5_kb'], d['lpips_score_split'], d['pct_pair'], d['pct_fast'], d['wino_order']) == (8, 1, 1, 1, 1)
    assert all(d[k] == 1 for k in ('tconv_inter', 'firenet_h3', 'wino', 'wino_tconv', 'wino_s2d', 'wino_fastact'))
    assert all(d[k] == 0 for k in ('firenet_pad32', 'no_pred_dot', 'lpips_conv1_valu', 'vox_acc_kb_set', 'vox_split', 'vox_chunks', 'attn_valu',
                                   'png_per_dir', 'ablate', 'ablate_all', 'wino_var', 'vox_scanprobe'))


@needs_hipcc
def test_the_arithmetic_rule(rows):
    arith = lambda rid: rows[rid]['arith']
    # EVR_FP32 set to anything -- empty and 0 too -- is exact fp32, whatever EVR_ARITH says
    assert [arith(r) for r in ('EVR_FP32=1', 'EVR_FP32=0', 'EVR_FP32=', 'EVR_ARITH=mx EVR_FP32=1', 'EVR_ARITH=mx6 EVR_FP32=0')] == [0] * 5
    assert [arith(r) for r in ('empty', 'EVR_ARITH=', 'EVR_ARITH=h3', 'EVR_ARITH=mx6', 'EVR_ARITH=mx', 'EVR_ARITH=fp32', 'EVR_ARITH=abc')] == [3, 3, 3, 4, 2, 0, 3]


@needs_hipcc
def test_defaults_that_replace_a_value_out_of_range(rows):
    assert [rows[r]['wino_blocks'] for r in ('EVR_WINO_BLOCKS=0', 'EVR_WINO_BLOCKS=-3', 'EVR_WINO_BLOCKS=', 'EVR_WINO_BLOCKS=abc', 'EVR_WINO_BLOCKS=128')] == [256] * 4 + [128]
    # the head kernel's grid: three work-groups per CU once its weights live in LDS
    assert [rows[r]['head_blocks'] for r in ('EVR_HEAD_WLDS=1', 'EVR_HEAD_WLDS=0', 'EVR_HEAD_BLOCKS=0', 'EVR_HEAD_BLOCKS=-2', 'EVR_HEAD_BLOCKS=1024',
                                             'EVR_HEAD_BLOCKS=300 EVR_HEAD_WLDS=1', 'EVR_HEAD_BLOCKS=0 EVR_HEAD_WLDS=1')] == [768, 512, 512, 512, 1024, 300, 768]
    assert rows['EVR_LPIPS_BAND5=-1']['lpips_band5_kb'] == -1 and rows['EVR_LPIPS_BAND5=']['lpips_band5_kb'] == 0
    # "unset" survives for the tensorizer's cell budget: voxelize.hip owns the default and the clamp
    assert (rows['EVR_VOX_ACC_KB=0']['vox_acc_kb_set'], rows['EVR_VOX_ACC_KB=0']['vox_acc_kb']) == (1, 0)
    assert (rows['EVR_VOX_ACC_KB=500']['vox_acc_kb_set'], rows['EVR_VOX_ACC_KB=500']['vox_acc_kb']) == (1, 500)


@needs_hipcc
def test_the_three_ways_to_be_a_flag(rows):
    # set, any value
    for name, field in (('EVR_NO_PRED_DOT', 'no_pred_dot'), ('EVR_LPIPS_CONV1_VALU', 'lpips_conv1_valu'), ('EVR_ABLATE_ALL', 'ablate_all')):
        assert [rows[f'{name}={v}'][field] for v in ('0', '1', '', 'abc')] == [1, 1, 1, 1], name
    # on unless it reads as 0: empty and a non-number switch it off too
    for name, field in (('EVR_TCONV_INTER', 'tconv_inter'), ('EVR_FIRENET_H3', 'firenet_h3'), ('EVR_WINO', 'wino'), ('EVR_WINO_TCONV', 'wino_tconv'),
                        ('EVR_WINO_S2D', 'wino_s2d'), ('EVR_WINO_FASTACT', 'wino_fastact')):
        assert [rows[f'{name}={v}'][field] for v in ('0', '1', '', 'abc')] == [0, 1, 0, 0], name
    # off unless it reads as non-zero
    for name, field in (('EVR_FIRENET_PAD32', 'firenet_pad32'), ('EVR_ATTN_VALU', 'attn_valu')):
        assert [rows[f'{name}={v}'][field] for v in ('0', '1', '', 'abc')] == [0, 1, 0, 0], name


def _sources(*exts):
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(exts):
                yield os.path.join(d, f)


def test_the_readme_names_every_switch_the_package_reads():
    with open(os.path.join(ROOT, 'README.md')) as fh:
        readme = fh.read()
    names = {}
    for path in _sources('.py', '.cpp', '.hip', '.h'):
        with open(path, errors='replace') as fh:
            for m in re.finditer(r'''["']((?:EVR|EVREAL)_[A-Z0-9_]+)["']''', fh.read()):
                names.setdefault(m.group(1), os.path.relpath(path, ROOT))
    assert len(names) > 60      # (the scan found the code)
    missing = {n: p for n, p in names.items() if not re.search(r'\b' + n + r'\b', readme)}
    assert not missing, missing


def test_only_the_two_tables_read_the_environment():
    found = {}
    for path in _sources('.cpp', '.hip', '.h'):
        if os.path.dirname(path) != CSRC:
            continue
        with open(path, errors='replace') as fh:
            hits = [line.strip() for line in fh if 'getenv(' in line]
        if hits:
            found[os.path.basename(path)] = hits
    assert sorted(found) == ['conv_route.cpp', 'knobs.cpp'], found
    # conv_route.cpp: the one read behind conv_knobs()
    assert len(found['conv_route.cpp']) == 1 and 'conv_knobs_from(' in found['conv_route.cpp'][0], found['conv_route.cpp']
    assert len(found['knobs.cpp']) == 1 and 'lib_knobs_from(' in found['knobs.cpp'][0], found['knobs.cpp']
