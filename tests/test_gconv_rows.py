"""The 16-channel-block grouped 3x3 kernel (csrc/gconv_rows.hip: gconv_rows_kernel) against the fp64 grouped conv of the same operand planes,
forced onto every shape (LP_GCONV_ROWS=2), with its full epilogue (statistics partials, 16-bit-resident output, bf16x3 planes, alpha2, amax),
with one workgroup walking many tiles (LP_GCONV_ROWS_WGS = 1 | 3) and bit-identical results across tile walks.  The cases run in one fresh
interpreter per env setting (tests/gconv_rows_cases.py; the knobs are read once per process), each interpreter once for all tests here.  The
index arithmetic of the kernel is also restated on the CPU (scripts/gconv_rows_emu.py, run by the non-GPU test below)."""
import functools
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _child(wgs):
    env = dict(os.environ, LP_GCONV_ROWS='0' if wgs == 'old' else '2')      # 'old': conv_dma_kernel's block-diagonal form on the walk shape
    env.pop('LP_GCONV_ROWS_WGS', None)
    if wgs and wgs != 'old':
        env['LP_GCONV_ROWS_WGS'] = wgs
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'gconv_rows_cases.py')] + (['walk'] if wgs else [])
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-8000:])
    return r.returncode, r.stdout, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize('wgs', ['', '1', '3', '16', 'old'])      # 16: XCD-ordered walk, two tiles per workgroup; 1: also proves which kernel ran (amax slots)
def test_gconv_rows_cases(wgs):
    rc, out, err = _child(wgs)
    assert rc == 0 and 'GCONV_ROWS_OK' in out, (out[-3000:], err[-3000:])


@pytest.mark.gpu
def test_gconv_rows_is_bit_identical_across_launches_and_tile_walks():
    """no atomics in y or the partials, and a summation order per output that does not depend on which workgroup walks which tiles -- and is
    the order of conv_dma_kernel's grouped form ('old'), partials included: the training step computes the same bits on either route"""
    dets = []
    for wgs in ('', '1', '3', '16', 'old'):
        rc, out, err = _child(wgs)
        assert rc == 0, (out[-3000:], err[-3000:])           # (each child has already compared two launches of its own)
        dets.append(dict(re.findall(r'^DET (\d) ([0-9a-f]{64})$', out, re.M)))
    assert set(dets[0]) == {'1', '2'} and all(d == dets[0] for d in dets), dets


def test_gconv_rows_index_arithmetic_on_cpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'gconv_rows_emu.py')], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'GCONV_ROWS_EMU_OK' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'FAILED' not in r.stdout and r.stdout.count('worst halo read 4 LDS cycles') >= 18, r.stdout[-2000:]
