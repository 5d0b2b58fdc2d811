"""Host-side checks of the image-quality metric (no GPU):
  * the fp64 restatement (tests/image_quality_restatement.py) on cases with a closed form: identical images, two constant images, values outside
    [0, 1], a mask that is one pixel wide (it must act at the window CENTRE);
  * the plugin resolves through the runner's loader, its flag defaults to True, ``hipops.image_quality`` and the C entry point refuse bad arguments
    before any device call;
  * ``run_epoch`` puts ``compute_metrics`` into the epoch meter as ``Metric_<name>`` and is unchanged without a metric."""
import argparse
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import image_quality_restatement as IQ          # noqa: E402


# ---- restatement ---------------------------------------------------------------------------------------------------------------------------------------
def test_identical_images_give_1_100_0():
    x = torch.rand(2, 3, 19, 23, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    t = IQ.table(x, x.clone(), torch.ones(2, 19, 23, dtype=torch.float64))
    for n in range(2):
        assert t[n].tolist() == [1.0, 100.0, 0.0, 1.0, 100.0, 0.0], t[n].tolist()
    assert bool(torch.isnan(IQ.table(x, x)[:, 3:]).all())          # no mask: the foreground columns are undefined


@pytest.mark.parametrize('mu,delta', [(0.7, 0.001), (0.25, 0.5), (0.0, 1.0)])
def test_constant_images_have_the_closed_form(mu, delta):
    x = torch.full((1, 3, 14, 17), mu, dtype=torch.float64)
    y = torch.full((1, 3, 14, 17), mu + delta, dtype=torch.float64)
    t = IQ.table(x, y, torch.full((1, 14, 17), 0.3, dtype=torch.float64))[0]
    ssim = (2 * mu * (mu + delta) + IQ.C1) / (mu ** 2 + (mu + delta) ** 2 + IQ.C1)
    for col in (0, 3):
        assert abs(t[col].item() - ssim) <= 1e-12, (col, t[col].item(), ssim)
    for col in (1, 4):
        assert abs(t[col].item() + 20 * math.log10(delta)) <= 1e-12, (col, t[col].item())
    for col in (2, 5):
        assert abs(t[col].item() - delta) <= 1e-12


def test_values_outside_the_unit_interval_are_clamped():
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 16, 16, generator=g, dtype=torch.float64) * 2 - 0.5
    y = torch.rand(2, 3, 16, 16, generator=g, dtype=torch.float64) * 2 - 0.5
    m = torch.rand(2, 16, 16, generator=g, dtype=torch.float64)
    assert bool((x < 0).any()) and bool((x > 1).any())
    assert torch.equal(IQ.table(x, y, m), IQ.table(x.clamp(0, 1), y.clamp(0, 1), m))
    assert not torch.equal(IQ.table(x, y, m)[:, :3], IQ.table(x, y.clamp(0, 1) * 0.5, m)[:, :3])
    # the mask is NOT clamped: twice the weights give the same ratios
    assert torch.allclose(IQ.table(x, y, 2 * m), IQ.table(x, y, m), rtol=1e-13, atol=0)


def test_the_mask_weighs_a_window_by_its_centre_pixel():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(1, 2, 15, 18, generator=g, dtype=torch.float64)
    y = torch.rand(1, 2, 15, 18, generator=g, dtype=torch.float64)
    S = IQ.ssim_map(x, y)                                # [1, 2, 5, 8]
    m = torch.zeros(1, 15, 18, dtype=torch.float64)
    m[0, 5 + 3, 5 + 6] = 0.25                            # the centre of window (3, 6)
    t = IQ.table(x, y, m)[0]
    assert abs(t[3].item() - S[0, :, 3, 6].mean().item()) <= 1e-15
    d = (x - y)[0, :, 8, 11]
    assert abs(t[5].item() - d.abs().mean().item()) <= 1e-15
    # a mask that lives in the 5-pixel border only: no window centre carries weight -> ssim_fg undefined, the pixel columns defined
    m = torch.zeros(1, 15, 18, dtype=torch.float64)
    m[0, 2, 2] = 1.0
    t = IQ.table(x, y, m)[0]
    assert math.isnan(t[3].item()) and not math.isnan(t[4].item()) and not math.isnan(t[5].item())
    # no weight at all: the three foreground columns are NaN, the whole-frame ones are not
    t = IQ.table(x, y, torch.zeros(1, 15, 18, dtype=torch.float64))[0]
    assert bool(torch.isnan(t[3:]).all()) and not bool(torch.isnan(t[:3]).any())


def test_target_frames_axis_takes_frame_0():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 12, 12, generator=g, dtype=torch.float64)
    y = torch.rand(2, 2, 3, 12, 12, generator=g, dtype=torch.float64)
    assert torch.equal(IQ.table(x, y)[:, :3], IQ.table(x, y[:, 0].contiguous())[:, :3])
    assert not torch.equal(IQ.table(x, y)[:, :3], IQ.table(x, y[:, 1].contiguous())[:, :3])


# ---- plugin, wrapper, C entry point -------------------------------------------------------------------------------------------------------------------
def test_plugin_resolves_and_flag_defaults_to_true():
    from utils.argparse_utils import MyArgumentParser
    from utils.utils import load_wrappers_for_module_list
    wrappers = load_wrappers_for_module_list('image_quality', 'metrics')
    assert len(wrappers) == 1
    parser = MyArgumentParser(conflict_handler='resolve')
    wrappers[0].get_args(parser)
    assert parser.parse_args([]).image_quality_foreground is True
    assert parser.parse_args(['--no-image_quality_foreground']).image_quality_foreground is False
    net = wrappers[0].get_net(argparse.Namespace(image_quality_foreground=False, device='cpu'))
    assert isinstance(net, torch.nn.Module) and net.foreground is False and not list(net.parameters())


def test_wrapper_refuses_bad_inputs_before_any_device_call():
    from latent_pose_reenactment_amd import hipops as ops
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match='CUDA'):
        ops.image_quality(x, x.clone())
    with pytest.raises(ValueError, match='fp32'):
        ops.image_quality(x.double(), x.double())
    with pytest.raises(ValueError, match='fp32'):
        ops.image_quality(x, x.clone(), torch.ones(2, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match='>= 11'):
        ops.image_quality(torch.zeros(1, 3, 10, 10), torch.zeros(1, 3, 10, 10))
    with pytest.raises(ValueError, match='>= 11'):
        ops.image_quality(torch.zeros(1, 3, 16, 10), torch.zeros(1, 3, 16, 10))
    with pytest.raises(ValueError, match='mismatch'):
        ops.image_quality(x, torch.zeros(2, 3, 16, 17))
    with pytest.raises(ValueError, match='mismatch'):
        ops.image_quality(x, torch.zeros(2, 1, 1, 16, 16))          # frame 0 of the 5-D target has another channel count
    with pytest.raises(ValueError, match='mismatch'):
        ops.image_quality(x, x.clone(), torch.ones(2, 3, 16, 16))
    with pytest.raises(ValueError, match='4 channels'):
        ops.image_quality(torch.zeros(1, 5, 16, 16), torch.zeros(1, 5, 16, 16))
    with pytest.raises(ValueError, match='expected x'):
        ops.image_quality(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))


def test_c_entry_point_validates_before_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    assert l.lp_image_quality_workspace_bytes(1, 11, 11) == 8 * 4                      # one tile, eight partial sums
    assert l.lp_image_quality_workspace_bytes(3, 27, 43) == 3 * 2 * 3 * 8 * 4          # 17 x 33 window positions = 2 x 3 tiles of 16 x 16
    assert l.lp_image_quality_workspace_bytes(8, 256, 256) == 8 * 256 * 8 * 4
    assert l.lp_image_quality_workspace_bytes(1, 10, 64) == 0
    st = (ctypes.c_longlong * 4)(768, 256, 16, 1)
    sp, fake = ctypes.addressof(st), 4096          # (never dereferenced: every call below is refused first)
    assert l.lp_image_quality(None, sp, fake, sp, None, None, 1, 3, 16, 16, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    assert l.lp_image_quality(fake, sp, fake, sp, fake, None, 1, 3, 16, 16, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    assert l.lp_image_quality(fake, sp, fake, sp, None, None, 0, 3, 16, 16, fake, fake, None) == -1 and b'B >= 1' in l.lp_last_error()
    assert l.lp_image_quality(fake, sp, fake, sp, None, None, 1, 5, 16, 16, fake, fake, None) == -1 and b'1 .. 4' in l.lp_last_error()
    assert l.lp_image_quality(fake, sp, fake, sp, None, None, 1, 3, 10, 16, fake, fake, None) == -1 and b'11' in l.lp_last_error()
    assert l.lp_image_quality(fake, sp, fake, sp, None, None, 1, 3, 16, 10, fake, fake, None) == -1 and b'11' in l.lp_last_error()


def test_abi_tests_hold_with_the_two_new_symbols():
    import test_abi
    decls = test_abi.parse_header()
    assert 'lp_image_quality' in decls and 'lp_image_quality_workspace_bytes' in decls
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_ctypes_signatures_match_header()
    test_abi.test_abi_version_and_error_string()


# ---- runner ---------------------------------------------------------------------------------------------------------------------------------------------
class _StubMetric(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, data_dict):
        self.seen.append(data_dict)
        return {'a': 2.0, 'b': float('nan')}, {'a': 3, 'b': 0}


def _stub_epoch(metrics, detailed=True, iterations=2):
    from runners import holycow
    all_data = {'fake_rgbs': torch.zeros(1, 3, 16, 16), 'target_rgbs': torch.zeros(1, 1, 3, 16, 16)}

    class Stub(holycow.TrainingModule):
        def forward(self, data_dict, target_dict):
            return all_data, {'g': torch.tensor(1.5)}, {'d': torch.tensor(0.5)}
    tm = Stub(None, None, None, [], metrics, running_averages=None)
    args = argparse.Namespace(device='cpu', detailed_metrics=detailed, log_frequency_loss=1, hip_graph=False, iteration=0)
    loader = [({'x': torch.zeros(1)}, {'y': torch.zeros(1)}) for _ in range(iterations)]
    with torch.no_grad():
        meter = holycow.run_epoch(loader, tm, None, None, 0, args, phase='val')
    return meter, all_data, args


def test_run_epoch_adds_the_metrics_to_the_epoch_meter():
    metric = _StubMetric()
    meter, all_data, args = _stub_epoch([metric], iterations=1)
    assert set(meter.keys()) == {'Data_time', 'Batch_time', 'Loss_g', 'Loss_d', 'Metric_a'}
    assert meter.get_average('Metric_a') == 2.0 and meter.get_last('Metric_a') == 2.0 and meter.get_num_measurements('Metric_a') == 3
    assert 'Metric_b' not in meter.last_value and meter.get_num_measurements('Metric_b') == 0
    assert len(metric.seen) == 1 and metric.seen[0] is all_data
    assert args.iteration == 0          # 'val' does not advance the iteration counter
    metric = _StubMetric()
    meter, _, _ = _stub_epoch([metric], iterations=2)          # the images of an epoch add up
    assert meter.get_average('Metric_a') == 2.0 and meter.get_num_measurements('Metric_a') == 6 and len(metric.seen) == 2


def test_run_epoch_without_a_metric_is_what_it_was():
    meter, _, _ = _stub_epoch([])
    assert set(meter.keys()) == {'Data_time', 'Batch_time', 'Loss_g', 'Loss_d'}
    assert meter.get_num_measurements('Loss_g') == 2 and meter.get_average('Loss_g') == 1.5
    # --no-detailed_metrics: neither losses nor metrics are read back
    metric = _StubMetric()
    meter, _, _ = _stub_epoch([metric], detailed=False)
    assert set(meter.keys()) == {'Data_time', 'Batch_time'} and not metric.seen
