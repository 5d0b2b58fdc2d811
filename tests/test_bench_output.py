"""What bench.py hands its caller: the ONE stdout result line stays short enough to survive a driver that keeps only the end of stdout (a
22 KB line once lost its head, `ms_per_step` included), --dump-outputs writes float32 / float64 arrays, a fixed sample of large tensors,
within 64 MB (CPU), and two runs with the same arguments compute bit-identical outputs (GPU)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _record(name):
    with open(os.path.join(ROOT, 'profiles', name)) as f:
        return json.loads([l for l in f.read().splitlines() if l.startswith('{')][-1])


def test_result_line_is_bounded_and_keeps_the_headline():
    import bench
    assert len(json.dumps(_record('r06_bench.json'))) > 3 * bench.RESULT_LINE_MAX_BYTES          # the whole record that once failed to parse
    for name in ('r06_bench.json', 'r06_bench_dp2_gloo_one_gpu_functional.json', 'r06_bench_generator.json'):
        full = _record(name)
        line = bench.result_line(full)
        assert '\n' not in line and len(line) <= bench.RESULT_LINE_MAX_BYTES, (name, len(line))
        j = json.loads(line)
        for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step'):
            assert j[k] == full[k], (name, k)
        assert j['config']['parallelism'] == full['config']['parallelism'] and j['roofline']['frac'] == full['roofline']['frac']
    j = json.loads(bench.result_line(_record('r06_bench_dp2_gloo_one_gpu_functional.json')))
    assert j['replicas']['bit_identical_parameters'] is True and j['single_gpu_same_workload']['value'] > 0
    j = json.loads(bench.result_line(_record('r06_bench.json')))
    assert j['finetune_step']['ms_per_step'] > 0 and j['cpu_baseline']['value'] > 0 and j['parity']['gates_met']


def test_result_line_is_strict_json_and_survives_any_record():
    import bench
    full = _record('r06_bench.json')
    full['value'] = float('nan')
    full['finetune_step'] = {'error': 'x' * 10000}
    full['roofline_huge'] = {'note': 'y' * 20000}
    full['config']['workload'] = 'z' * 20000
    line = bench.result_line(full)
    assert len(line) <= bench.RESULT_LINE_MAX_BYTES
    j = json.loads(line, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    assert j['value'] is None and j['ms_per_step'] == full['ms_per_step']


def test_dump_outputs_writes_fixed_samples_within_64_mb(tmp_path):
    import zlib
    import bench
    g = torch.Generator().manual_seed(0)
    frames = torch.randn(16, 8, 3, 256, 256, generator=g)          # 100 MB in fp32: must be sampled
    outputs = {'all_data': {'enc_rgbs': frames, 'fake_rgbs': torch.randn(8, 3, 64, 64, generator=g).half(),
                            'label': torch.arange(8), 'features': [torch.ones(2, 3), torch.zeros(4)], 'tag': 'not an array',
                            'score64': torch.tensor([1 / 3, 2 ** -40 + 1], dtype=torch.float64)},
               'losses_G': {'adversarial': torch.tensor(0.25, requires_grad=True) * 2, 'py': 1 / 3}, 'losses_D': {}}
    written = bench.dump_outputs(str(tmp_path / 'a'), outputs)
    bench.dump_outputs(str(tmp_path / 'b'), outputs)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(n + '.npy' for n in written) == ['all_data.enc_rgbs.npy', 'all_data.fake_rgbs.npy', 'all_data.features.0.npy',
                                                            'all_data.features.1.npy', 'all_data.label.npy', 'all_data.score64.npy',
                                                            'losses_G.adversarial.npy', 'losses_G.py.npy']
    total = sum(os.path.getsize(tmp_path / 'a' / f) for f in files)
    assert 60 << 20 < total <= 64 << 20, total                      # the budget is used, not half of it
    for f in files:
        x, y = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f          # same elements picked on every run
    assert np.load(tmp_path / 'a' / 'all_data.fake_rgbs.npy').shape == (8, 3, 64, 64)
    assert np.load(tmp_path / 'a' / 'all_data.label.npy').dtype == np.float64
    s64 = np.load(tmp_path / 'a' / 'all_data.score64.npy')
    assert s64.dtype == np.float64 and s64.tolist() == [1 / 3, 2 ** -40 + 1]          # float64 outputs keep their precision
    assert np.load(tmp_path / 'a' / 'losses_G.py.npy').dtype == np.float64 and float(np.load(tmp_path / 'a' / 'losses_G.py.npy')) == 1 / 3
    assert np.load(tmp_path / 'a' / 'losses_G.adversarial.npy').dtype == np.float32
    assert float(np.load(tmp_path / 'a' / 'losses_G.adversarial.npy')) == 0.5
    sample = np.load(tmp_path / 'a' / 'all_data.enc_rgbs.npy')
    assert sample.ndim == 1 and (1 << 20) < sample.size < frames.numel() and written['all_data.enc_rgbs'] == (tuple(frames.shape), sample.size)
    idx = np.sort(np.random.default_rng(zlib.crc32(b'all_data.enc_rgbs')).choice(frames.numel(), sample.size, replace=False))
    assert np.array_equal(sample, frames.reshape(-1).numpy()[idx])      # exactly the seeded sample of the tensor's elements


@pytest.mark.gpu
def test_two_bench_runs_compute_bit_identical_outputs(tmp_path):
    """the same arguments twice, each run in its own process: the dumped inputs (the synthetic batch inside all_data) and, after several
    optimizer steps of the captured meta-training step, every output (all_data, losses) are bit-identical -- no float atomics or other
    order-dependent reductions on the timed path"""
    import subprocess
    dumps = []
    for k in range(2):
        d = str(tmp_path / f'run{k}')
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2', '--image_size', '128',
                            '--no-cpu-baseline', '--no-also', '--no-drive', '--dump-outputs', d], cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])['steps'] == 3
        dumps.append(d)
    files = sorted(os.listdir(dumps[0]))
    assert files == sorted(os.listdir(dumps[1])) and any(f.startswith('all_data.fake_rgbs') for f in files)
    inputs = [f'all_data.{k}.npy' for k in ('enc_rgbs', 'pose_input_rgbs', 'target_rgbs', 'real_segm', 'label')]
    assert set(inputs) <= set(files), files          # the synthetic batch is part of the dump: identical inputs are checked, not assumed
    differ = [f for f in files if not np.array_equal(np.load(os.path.join(dumps[0], f)), np.load(os.path.join(dumps[1], f)), equal_nan=True)]
    assert not differ, differ
