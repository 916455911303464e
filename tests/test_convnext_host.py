"""ConvNeXt without a GPU: the fixtures against a live run of the reference (when its tree is present), state_dict keys
and shapes against the reference classes, the drop-path ladder, the YAML through the Engine on cpu, the refusals, and
the k = 2 / stride 2 descriptors of the downsample convolutions through the emulator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnext_model_util as MU
import emu
from passl_amd.hip import config as hip_config
from passl_amd.hip import plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.isdir('/root/reference/passl/models')
FACTORIES = ('convnext_tiny', 'convnext_small', 'convnext_base', 'convnext_large', 'convnext_xlarge')


@pytest.fixture(scope='module')
def live_reference():
    """One run of tests/golden/make_golden_convnext.py --check in a process of its own (the reference's `passl` package
    cannot live next to the product's): -> (exit status, output, {model: [[key, shape]]})."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'make_golden_convnext.py'), '--check'],
                       capture_output=True, text=True, cwd=ROOT)
    keys = [l for l in r.stdout.splitlines() if l.startswith('KEYS ')]
    text = '\n'.join(l for l in r.stdout.splitlines() if not l.startswith('KEYS '))
    return r.returncode, text[-2000:] + r.stderr[-2000:], json.loads(keys[-1][5:]) if keys else None


@pytest.mark.skipif(not HAVE_REF, reason='reference tree not present')
def test_fixtures_equal_a_live_reference_run(live_reference):
    rc, text, _keys = live_reference
    assert rc == 0, text
    assert 'fixtures equal the live reference run' in text


def _product(name, **kw):
    import passl.models as PM
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    return PM.build_model(dict(name=name, **kw))


@pytest.mark.skipif(not HAVE_REF, reason='reference tree not present')
@pytest.mark.parametrize('name', ('small',) + FACTORIES)
def test_state_dict_keys_and_shapes_are_the_reference_classes(live_reference, name):
    _rc, text, keys = live_reference
    assert keys is not None, text
    model = _product('ConvNeXt', **MU.MODEL) if name == 'small' else _product(name)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == dict((k, s) for k, s in keys[name])


def test_state_dict_keys_against_the_fixture():
    """(Runs without the reference tree: the fixture records the reference's keys and shapes.)"""
    model = _product('ConvNeXt', **MU.MODEL)
    got = sorted('%s:%s' % (k, 'x'.join(map(str, v.shape))) for k, v in model.state_dict().items())
    for name in MU.CASES:
        assert got == sorted(MU.load(name)['keys'].tolist())
    assert 'downsample_layers.0.0.weight:8x3x4x4' in got and 'stages.2.1.gamma:32' in got
    assert 'downsample_layers.3.1.weight:64x32x2x2' in got and 'stages.0.0.dwconv.weight:8x1x7x7' in got


def test_drop_path_ladder_is_the_fixtures():
    for name, rate in MU.CASES.items():
        fx = MU.load(name)
        model = _product('ConvNeXt', drop_path_rate=rate, **MU.MODEL)
        assert np.array_equal(np.asarray(model.dp_rates, dtype=np.float64), fx['dp_rates'])
        blocks = [b for st in model.stages for b in st]
        assert [b.drop_path for b in blocks] == model.dp_rates
        _rates, keep_prob = MU.ladder(rate)
        assert [b.keep_prob for b in blocks if b.drop_path > 0] == keep_prob
        owners = model._drop_path.blocks if model._drop_path is not None else []
        assert len(owners) == (4 if rate else 0)
        if rate:
            assert fx['s0_keep'].shape == (4, MU.BATCH) and set(np.unique(fx['s0_keep'])) <= {0.0, 1.0}


def test_initialisation_and_head_init_scale():
    torch.manual_seed(0)
    a = _product('ConvNeXt', **MU.MODEL)
    torch.manual_seed(0)
    b = _product('ConvNeXt', head_init_scale=0.5, **MU.MODEL)
    sa, sb = a.state_dict(), b.state_dict()
    for k, v in sa.items():
        if k.endswith('gamma'):
            assert torch.equal(v, torch.full_like(v, 1e-6))
        elif k.endswith('bias'):
            assert not v.any()
        elif v.dim() == 1:
            assert torch.equal(v, torch.ones_like(v))
        else:
            assert float(v.abs().max()) <= 0.04 + 1e-7 and float(v.std()) > 0.005      # trunc-normal(0.02) in +-2 std
    assert torch.equal(sb['head.weight'], sa['head.weight'] * 0.5)
    assert torch.equal(sb['stages.3.0.pwconv1.weight'], sa['stages.3.0.pwconv1.weight'])


def test_refusals_raise_by_name():
    with pytest.raises(NotImplementedError, match='layer_scale_init_value'):
        _product('ConvNeXt', layer_scale_init_value=0, **MU.MODEL)
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        _product('ConvNeXt', **dict(MU.MODEL, dims=[8, 16, 36, 64]))
    model = _product('ConvNeXt', **MU.MODEL)
    with pytest.raises(NotImplementedError, match='multiple of 32'):
        model(torch.zeros(1, 3, 64, 80))
    with pytest.raises(ValueError, match='drop_path_rate'):
        _product('ConvNeXt', drop_path_rate=1.0, **MU.MODEL)
    from passl_amd.hip import nn
    with pytest.raises(NotImplementedError, match='stride'):
        nn.PatchConv2D(8, 16, 2, 1)
    with pytest.raises(ValueError, match='must be contiguous'):
        nn.layer_scale_add(torch.zeros(4, 16)[:, ::2], torch.zeros(4, 8), torch.ones(8), None, 1.0, 1, 4)
    with pytest.raises(AttributeError):
        import passl.models as PM
        PM.build_model(dict(name='convnext_nano'))


def test_yaml_loads_and_the_engine_builds_on_cpu(tmp_path):
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    path = os.path.join(ROOT, 'configs', 'v2', 'convnext_base_synthetic.yaml')
    text = open(path).read()
    for word in ('no_weight_decay_name', 'EMA', 'TimmAutoAugment', 'TransformOpSampler'):
        assert word in text.split('\nGlobal:')[0], 'the header must say that %s is left out' % word
    cfg = get_config(path, ['Global.device=cpu', 'Global.output_dir=%s' % tmp_path,
                            'DataLoader.Train.dataset.num_samples=16', 'DataLoader.Train.dataset.image_size=64',
                            'DataLoader.Train.dataset.num_classes=8', 'DataLoader.Train.sampler.batch_size=8',
                            'DataLoader.Eval.dataset.num_samples=8', 'DataLoader.Eval.dataset.image_size=64',
                            'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=8'])
    assert cfg['Model'] == dict(name='convnext_base', drop_path_rate=0.5, class_num=1000)
    assert cfg['LRScheduler']['name'] == 'TimmCosine' and cfg['LRScheduler']['learning_rate'] == 4e-3
    assert cfg['Optimizer']['weight_decay'] == 0.05 and 'no_weight_decay_name' not in cfg['Optimizer']
    assert cfg['Global']['seed'] == 42 and cfg['Global']['epochs'] == 300 and cfg['FP16']['level'] == 'O2'
    cfg['Model'] = dict(name='ConvNeXt', drop_path_rate=cfg['Model']['drop_path_rate'], **MU.MODEL)
    eng = Engine(cfg, mode='train')
    assert type(eng.model).__name__ == 'ConvNeXt' and type(eng.lr_scheduler).__name__ == 'TimmCosine'
    assert type(eng.optimizer).__name__ == 'AdamW'
    assert eng.lr_scheduler.warmup_steps == 20 * 2 and eng.lr_scheduler.eta_min == 1e-6


@pytest.mark.parametrize('nhw', [(2, 16, 24), (1, 2, 6), (3, 4, 2)])
@pytest.mark.parametrize('chans', [(8, 16), (32, 64)])
def test_patch_conv_descriptors_match_autograd(nhw, chans):
    """k = 2, stride 2, no padding, with the bias as the epilogue's shift: forward, the residue classes of the data
    gradient and the weight gradient through the emulator against torch autograd in float64."""
    N, H, W = nhw
    g = P.ConvGeom(cin=chans[0], cout=chans[1], k=2, stride=2, pad=0)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, g.cin, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(g.cout, g.cin, 2, 2, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(g.cout, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, 2, 0)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(dy)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()           # noqa: E731
    w_krsc = w.detach().permute(0, 2, 3, 1).contiguous()
    x_flat, dy_nhwc = nhwc(x.detach()).reshape(-1), nhwc(dy)
    d = P.fwd_desc(g, N, H, W)
    assert (d.OP, d.OQ) == (H // 2, W // 2)
    yf = torch.zeros(N * d.OP * d.OQ * g.cout, dtype=torch.float64)
    emu.emu_conv(d, x_flat, emu.emu_pack(d.pack, w_krsc), yf, shift=b.detach())
    torch.testing.assert_close(yf.view(N, d.OP, d.OQ, g.cout), nhwc(y.detach()))
    descs, skipped = P.dgrad_plan(g, N, H, W)
    dxf = torch.full((N * H * W * g.cin,), float('nan'), dtype=torch.float64)
    if skipped:
        dxf.zero_()
    for dd in descs:
        emu.emu_conv(dd, dy_nhwc.reshape(-1), emu.emu_pack(dd.pack, w_krsc), dxf)
    assert not torch.isnan(dxf).any(), 'the residue classes do not cover dx'
    torch.testing.assert_close(dxf.view(N, H, W, g.cin), nhwc(x.grad))
    dw = emu.emu_wgrad(P.wgrad_desc(g, N, H, W), x_flat, dy_nhwc.reshape(-1, g.cout))
    torch.testing.assert_close(dw.view(g.cout, 2, 2, g.cin), w.grad.permute(0, 2, 3, 1))
    torch.testing.assert_close(dy_nhwc.reshape(-1, g.cout).sum(0), b.grad)
