"""conv_dma_kernel and splitk_reduce_kernel (csrc/conv_dma.hip) in every dispatch form, bit for bit against the fp64 contraction of exact integer
operands -- tests/conv_dma_cases.py, once per knob setting in a fresh interpreter (the knob table is read once per process): the default plus the
conv entries of tests/test_kernel_variants.py.  The scripts append the launch record of every case to one file; after all settings have run, every
form of the literal table below must have been recorded at least once.  The budget of every case is asserted on the CPU (no GPU needed)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conv_dma_cases as M  # noqa: E402
from test_kernel_variants import VARIANTS  # noqa: E402

SETTINGS = [{}] + [v for v in VARIANTS if all(k.startswith('LP_CONV') for k in v)]
IDS = [','.join(f'{k}={v}' for k, v in e.items()) or 'default' for e in SETTINGS]
SCRIPT, OK = 'conv_dma_cases.py', 'CONV_DMA_EXACT_OK'
KNOBS = ('LP_CONV_PP', 'LP_CONV_W8', 'LP_CONV_KSPLIT', 'LP_CONV_SPLIT_WGS', 'LP_CONV_NBUF', 'LP_CONV_XCD', 'LP_CONV_PIPE', 'LP_CONV_PIPE_MR', 'LP_CONV1X1_PIPE')

# every form of conv_dma_kernel's dispatch: (name, fields the record of at least one exact case must show)
D = dict(kernel='dma')
FORMS = [
    ('<4,1,4,1> 3x3', dict(D, ks=3, ups=0, wm=4, wn=1, mr=4, nr=1)),
    ('<4,1,4,4> 3x3', dict(D, ks=3, ups=0, wm=4, wn=1, mr=4, nr=4)),
    ('<4,1,4,4> 3x3 ups', dict(D, ks=3, ups=1, wm=4, wn=1, mr=4, nr=4)),
    ('<2,2,4,4> 3x3', dict(D, ks=3, ups=0, wm=2, wn=2, mr=4, nr=4)),
    ('<2,2,4,4> 3x3 ups', dict(D, ks=3, ups=1, wm=2, wn=2, mr=4, nr=4)),
    ('8-wave <2,4,4,2> 3x3', dict(D, ks=3, ups=0, wm=2, wn=4, mr=4, nr=2)),
    ('8-wave <2,4,4,2> 3x3 ups', dict(D, ks=3, ups=1, wm=2, wn=4, mr=4, nr=2)),
    ('8-wave <2,4,4,2> 1x1', dict(D, ks=1, wm=2, wn=4, mr=4, nr=2)),
    ('bf16x3 <2,2,4,2> 3x3', dict(D, prec=1, ks=3, ups=0, wm=2, wn=2, mr=4, nr=2)),
    ('bf16x3 <2,2,4,2> 3x3 ups', dict(D, prec=1, ks=3, ups=1, wm=2, wn=2, mr=4, nr=2)),
    ('1x1 <4,1,4,4> 32-channel chunks', dict(D, ks=1, wm=4, wn=1, mr=4, nr=4, cc=32)),
    ('1x1 <2,2,4,4> 32-channel chunks', dict(D, ks=1, wm=2, wn=2, mr=4, nr=4, cc=32)),
    ('1x1 <4,1,4,4> 64-channel chunks', dict(D, ks=1, wm=4, wn=1, mr=4, nr=4, cc=64)),
    ('1x1 <2,2,4,4> 64-channel chunks', dict(D, ks=1, wm=2, wn=2, mr=4, nr=4, cc=64)),
    ('1x1 bf16x3 single activation buffer', dict(D, prec=1, ks=1, cc=32, a_dbuf=0)),
    ('1x1 bf16x3 double activation buffer', dict(D, prec=1, ks=1, cc=32, a_dbuf=1)),
    ('ping-pong', dict(D, ks=3, pp=1)),
    ('ping-pong upsampled', dict(D, ks=3, ups=1, pp=1)),
    ('2-deep weight ring', dict(D, pp=0, nbuf=2)),
    ('3-deep weight ring', dict(D, pp=0, nbuf=3)),
    ('split-K 2', dict(D, ksplit=2, finish=1)),
    ('split-K 4', dict(D, ksplit=4, finish=1)),
    ('split-K 8', dict(D, ksplit=8, finish=1)),
    ('split-K 6 (18 chunks)', dict(D, ksplit=6, finish=1)),
    ('split-K upsampled', dict(D, ups=1, ksplit=4, finish=1)),
    ('split-K 8-wave', dict(D, wm=2, wn=4, ksplit=4)),
    ('split-K 4-wave', dict(D, wm=2, wn=2, mr=4, nr=4, ksplit=2)),
    ('split-K bf16x3', dict(D, prec=1, wm=2, wn=2, mr=4, nr=2, ksplit=4)),
    ('statistics offered', dict(D, stats=1)),
]

_RUNS = {}


def run_setting(i, tmp):
    """one script run per knob setting and module, cached: -> (returncode, stdout, stderr, records)"""
    if i not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(SETTINGS[i])
        log = os.path.join(tmp, f'forms_{i}.jsonl')
        env['LP_FORM_LOG'] = log
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', SCRIPT)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        recs = [json.loads(line) for line in open(log)] if os.path.exists(log) else []
        _RUNS[i] = (r.returncode, r.stdout, r.stderr, recs)
    return _RUNS[i]


@pytest.fixture(scope='module')
def form_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('conv_dma_forms'))


def test_every_case_is_within_the_exactness_budget():
    """CPU: build() asserts alpha * conv(|A|, |W|) + |bias| + |res| <= 2^22 quanta for every case, mode and role, and that the reference is an fp32 value"""
    for prec in M.PRECS:
        for index, case in enumerate(M.CASES):
            for wide in M.roles(index, prec):
                b = M.build(case, prec, wide, 0 if case['dgrad'] else (0, 2)[index & 1])
                assert b['quanta'] <= 2 ** 22


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(SETTINGS)), ids=IDS)
def test_conv_dma_kernel_is_exact_on_integer_operands(i, form_dir):
    rc, out, err, _ = run_setting(i, form_dir)
    print(out[-20000:])
    assert rc == 0 and OK in out, (out[-6000:], err[-3000:])


@pytest.mark.gpu
def test_every_conv_dma_form_was_recorded(form_dir):
    recs = []
    for i in range(len(SETTINGS)):
        rc, out, err, r = run_setting(i, form_dir)
        assert rc == 0 and OK in out, (IDS[i], out[-3000:], err[-3000:])
        recs += [x['rec'] for x in r]
    missing = [name for name, want in FORMS if not any(all(rec.get(k) == v for k, v in want.items()) for rec in recs)]
    assert not missing, f'forms no exact case reached: {missing}'
