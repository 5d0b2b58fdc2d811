"""conv_pipe_kernel and conv1x1_pipe_kernel (csrc/conv_pipe.hip) in every tile form, bit for bit against the fp64 contraction of exact integer operands
-- tests/conv_pipe_exact_cases.py, once per knob setting in a fresh interpreter (the knob table is read once per process): LP_CONV_PIPE_MR = 4 and 8
force the tap-pipelined 3x3 kernel (bf16x3 included), LP_CONV1X1_PIPE = 2 the chunk-pipelined 1x1 kernel.  The scripts append the launch record of every
case to one file; after all settings have run, every tile form of the literal table below must have been recorded in every precision mode.  The budget
of every case is asserted on the CPU (no GPU needed)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conv_dma_cases as DMA  # noqa: E402
import conv_pipe_exact_cases as M  # noqa: E402

SETTINGS = [{'LP_CONV_PIPE_MR': '4'}, {'LP_CONV_PIPE_MR': '8'}, {'LP_CONV1X1_PIPE': '2'}]
IDS = [','.join(f'{k}={v}' for k, v in e.items()) for e in SETTINGS]
SCRIPT, OK = 'conv_pipe_exact_cases.py', 'CONV_PIPE_EXACT_OK'
KNOBS = ('LP_CONV_PP', 'LP_CONV_W8', 'LP_CONV_KSPLIT', 'LP_CONV_SPLIT_WGS', 'LP_CONV_NBUF', 'LP_CONV_XCD', 'LP_CONV_PIPE', 'LP_CONV_PIPE_MR', 'LP_CONV1X1_PIPE')

# the six tile forms of conv_pipe_kernel and the two of conv1x1_pipe_kernel; every one is required once per precision mode
TILE_FORMS = [
    ('3x3 <2,2,8,4>', dict(kernel='pipe', ks=3, ups=0, wm=2, wn=2, mr=8, nr=4)),
    ('3x3 <2,2,8,4> ups', dict(kernel='pipe', ks=3, ups=1, wm=2, wn=2, mr=8, nr=4)),
    ('3x3 <2,2,4,4>', dict(kernel='pipe', ks=3, ups=0, wm=2, wn=2, mr=4, nr=4)),
    ('3x3 <2,2,4,4> ups', dict(kernel='pipe', ks=3, ups=1, wm=2, wn=2, mr=4, nr=4)),
    ('3x3 <4,1,4,4>', dict(kernel='pipe', ks=3, ups=0, wm=4, wn=1, mr=4, nr=4)),
    ('3x3 <4,1,4,4> ups', dict(kernel='pipe', ks=3, ups=1, wm=4, wn=1, mr=4, nr=4)),
    ('1x1 <4,1>', dict(kernel='pipe1x1', ks=1, wm=4, wn=1)),
    ('1x1 <2,2>', dict(kernel='pipe1x1', ks=1, wm=2, wn=2)),
]
RING = {0: 4, 1: 3, 2: 4}          # ring depth of conv1x1_pipe_kernel per precision mode
FORMS = [(f'{name} prec={prec}', dict(want, prec=prec, **(dict(nbuf=RING[prec]) if want['ks'] == 1 else {}))) for name, want in TILE_FORMS for prec in (0, 1, 2)] + \
        [('statistics offered 3x3', dict(kernel='pipe', stats=1)), ('statistics offered 1x1', dict(kernel='pipe1x1', stats=1))]

_RUNS = {}


def run_setting(i, tmp):
    """one script run per knob setting, cached: -> (returncode, stdout, stderr, records)"""
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
    return str(tmp_path_factory.mktemp('conv_pipe_forms'))


def test_every_case_is_within_the_exactness_budget():
    """CPU: build() asserts alpha * conv(|A|, |W|) + |bias| + |res| <= 2^22 quanta for every case, mode and role, and that the reference is an fp32 value"""
    for prec in M.PRECS:
        for index, case in enumerate(M.CASES):
            for wide in M.roles(index, prec):
                b = DMA.build(case, prec, wide, M.pro_of(index, case))
                assert b['quanta'] <= 2 ** 22


def test_every_setting_runs_the_cases_of_the_kernel_it_forces():
    assert [len(M.cases_of(e)) for e in SETTINGS] == [len(M.CASES_3X3), len(M.CASES_3X3), len(M.CASES_1X1)]
    assert len(FORMS) == 3 * 8 + 2


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(SETTINGS)), ids=IDS)
def test_pipelined_kernels_are_exact_on_integer_operands(i, form_dir):
    rc, out, err, _ = run_setting(i, form_dir)
    print(out[-20000:])
    assert rc == 0 and OK in out, (out[-6000:], err[-3000:])


@pytest.mark.gpu
def test_every_pipelined_tile_form_was_recorded(form_dir):
    recs = []
    for i in range(len(SETTINGS)):
        rc, out, err, r = run_setting(i, form_dir)
        assert rc == 0 and OK in out, (IDS[i], out[-3000:], err[-3000:])
        recs += [x['rec'] for x in r]
    missing = [name for name, want in FORMS if not any(all(rec.get(k) == v for k, v in want.items()) for rec in recs)]
    assert not missing, f'forms no exact case reached: {missing}'
