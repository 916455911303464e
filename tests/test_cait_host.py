"""CaiT on the CPU: the float64 restatement of tests/cait_util.py against what the reference's own TalkingHeadAttn and
ClassAttn computed (tests/golden/cait_layers.npz), the condition on the inputs of the kernel tests, planted defects
against the criteria of the GPU test, and the model's names, refusals and config.  No GPU, no kernel."""
import collections
import os

import numpy as np
import pytest
import torch

import attention_util as A
import cait_model_util as MU
import cait_util as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(z, name):
    st = {k[len(name + '/state/'):]: torch.from_numpy(v).double() for k, v in z.items() if k.startswith(name + '/state/')}
    return st, torch.from_numpy(z[name + '/x']).double(), torch.from_numpy(z[name + '/out']).double()


def test_restatement_equals_the_reference_layers():
    z = MU.load(MU.LAYERS)
    st, x, ref = _layer(z, 'th')
    B, T, Cw = x.shape
    H = st['proj_l.bias'].numel()
    d = dict(qkv=(x @ st['qkv.weight'] + st['qkv.bias']).reshape(B, T, 3, H, Cw // H), dout=torch.zeros(B, T, H, Cw // H),
             wl=st['proj_l.weight'], bl=st['proj_l.bias'], ww=st['proj_w.weight'], bw=st['proj_w.bias'],
             scale=(Cw // H) ** -0.5)
    out = C.reference(d)['out'].reshape(B, T, Cw) @ st['proj.weight'] + st['proj.bias']
    assert float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # the orientation of the head mixes is seen: the transposed one is far away
    bad = C.reference(d, defect='mix_transposed')['out'].reshape(B, T, Cw) @ st['proj.weight'] + st['proj.bias']
    assert float((bad - ref).abs().max()) > 1e-2 * float(ref.abs().max())
    st, x, ref = _layer(z, 'ca')
    B, T, Cw = x.shape
    H = 3
    d = dict(q=(x[:, 0] @ st['q.weight'] + st['q.bias']).reshape(B, H, Cw // H),
             k=(x @ st['k.weight'] + st['k.bias']).reshape(B, T, H, Cw // H),
             v=(x @ st['v.weight'] + st['v.bias']).reshape(B, T, H, Cw // H), dout=torch.zeros(B, H, Cw // H),
             scale=(Cw // H) ** -0.5)
    out = (C.cls_reference(d)['out'].reshape(B, Cw) @ st['proj.weight'] + st['proj.bias']).unsqueeze(1)
    assert float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_backward_of_the_restatement_is_autograd_s():
    """The closed-form backward against torch.autograd on the literal forward, float64."""
    d = C.make_case((2, 5, 4), 'plain', 1.0)
    leaves = {n: d[n].double().requires_grad_() for n in ('qkv', 'wl', 'bl', 'ww', 'bw')}
    q, k, v = [leaves['qkv'][:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    S = (q @ k.transpose(-1, -2)) * d['scale']
    P = torch.softmax(torch.einsum('bhij,hg->bgij', S, leaves['wl']) + leaves['bl'].view(1, -1, 1, 1), -1)
    R = torch.einsum('bhij,hg->bgij', P, leaves['ww']) + leaves['bw'].view(1, -1, 1, 1)
    out = (R @ v).permute(0, 2, 1, 3)
    out.backward(d['dout'].double())
    r = C.reference(d)
    g = leaves['qkv'].grad
    for n, want in (('out', out.detach()), ('dq', g[:, :, 0]), ('dk', g[:, :, 1]), ('dv', g[:, :, 2]),
                    ('dwl', leaves['wl'].grad), ('dww', leaves['ww'].grad), ('dbw', leaves['bw'].grad),
                    ('dbl', leaves['bl'].grad)):
        assert A.limit_usage(r[n], want, r['b_' + n], 1e-12)[0] <= 1, n
    assert float(r['dbl'].abs().max()) <= 1e-12 * float(r['b_dbl'].max())        # analytically zero
    dc = C.make_cls_case((2, 5, 3), 'plain')
    lv = {n: dc[n].double().requires_grad_() for n in ('q', 'k', 'v')}
    p = torch.softmax(torch.einsum('bhd,bthd->bht', lv['q'], lv['k']) * dc['scale'], -1)
    o = torch.einsum('bht,bthd->bhd', p, lv['v'])
    o.backward(dc['dout'].double())
    r = C.cls_reference(dc)
    for n, want in (('out', o.detach()), ('dq', lv['q'].grad), ('dk', lv['k'].grad), ('dv', lv['v'].grad)):
        assert A.limit_usage(r[n], want, r['b_' + n], 1e-12)[0] <= 1, n


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_no_bound_underflows_and_the_rounding_model_is_inside_the_limits(case):
    """The condition on the inputs (no element of any compared tensor has a bound below 2^-100), for every case of the
    GPU test; and the criteria accept the rounding model."""
    for kind in C.KINDS:
        for dev in C.DEVS:
            d = C.make_case(case, kind, dev)
            ref = C.reference(d)
            assert C.smallest_bound(ref, C.TENSORS) >= A.TINY, (kind, dev, C.smallest_bound(ref, C.TENSORS))
            model = C.reference(d, round_out=True)
            assert not C.violations(model, ref, C.LIMIT_BF16, C.TENSORS), (kind, dev)


@pytest.mark.parametrize('case', C.CLS_CASES, ids=C.case_id)
def test_class_attention_bounds_do_not_underflow(case):
    """One query per (image, head): under `peaked` its scores have standard deviation |q| 3.5 / sqrt(48) x 3.5 sqrt(48),
    about 12 and up to 15 for a long q (|q| of 48 normals spreads by 10 %), so a key more than 69 = ln 2^100 below the
    row's maximum (about +2.9 sigma over 208 keys), i.e. below -1.7 .. -2.8 sigma, has a probability under 2^-100 and
    rows of dk / dv that nothing can be compared with: 0.3 % to 4 % of a row, and a tensor holds only 4 to 16 rows.
    C.CLS_UNDERFLOW_CAP = 2 % of a tensor may be so under `peaked` (1 % for the dense kernels, attention_util, whose
    tensors average over T queries per head); those elements are held to 2^-100 absolutely.  `vmean` (q, k x 3) has the odd
    such element, `plain` none."""
    for kind in C.KINDS:
        d = C.make_cls_case(case, kind)
        ref = C.cls_reference(d)
        for n in C.CLS_TENSORS:
            assert A.underflow_share(ref['b_' + n]) <= (0. if kind == 'plain' else C.CLS_UNDERFLOW_CAP), (kind, n)
        assert not C.violations(C.cls_reference(d, round_out=True), ref, C.CLS_LIMIT_BF16, C.CLS_TENSORS), kind


@pytest.mark.parametrize('defect', C.DEFECTS)
def test_criteria_see_the_planted_defects(defect):
    """Each defect, planted in the rounding model, is outside a limit on at least one kernel case.  `pad_key` is also
    shown on cait_util.pad_key_inputs(), built so that the padded key would take most of the softmax mass."""
    seen = []
    for case in C.CASES[1:4]:                              # T = 5, 17, 33: none a multiple of 16
        d = C.make_case(case, 'plain', 1.0)
        bad = C.violations(C.reference(d, round_out=True, defect=defect), C.reference(d), C.LIMIT_BF16, C.TENSORS)
        seen += [(C.case_id(case), n, round(u, 2)) for n, u, _ in bad]
    print(defect, seen)
    assert seen, 'the criteria do not see the planted defect %s' % defect
    if defect == 'pad_key':
        d = C.pad_key_inputs()
        bad = C.violations(C.reference(d, round_out=True, defect=defect), C.reference(d), C.LIMIT_BF16, C.TENSORS)
        assert {n for n, _u, _m in bad} >= {'out', 'dv'}, bad


def _cpu_model(**kw):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    hip_config.set_device('cpu')
    return PM.build_model(dict(kw))


def _keys(model):
    return ['%s:%s' % (k, 'x'.join(map(str, v.shape))) for k, v in model.state_dict().items()]


def test_state_dict_keys_and_shapes_of_the_fixture_model_and_all_ten_factories():
    import passl.models as PM
    from passl_amd.models import cait as CM
    fx = MU.load('cait_small')
    model = _cpu_model(name='Cait', drop_path_rate=0.5, **MU.MODEL)
    assert _keys(model) == list(fx['keys'])
    assert sorted(model.no_weight_decay()) == list(fx['model_no_weight_decay']) and model.get_classifier() is model.head
    assert [b.drop_path for b in model.blocks] == [0.5, 0.5] and [b.drop_path for b in model.blocks_token_only] == [0., 0.]
    want = collections.defaultdict(list)
    for row in bytes(MU.load(MU.LAYERS)['factory_keys']).decode().split('\n'):
        f, k = row.split('|')
        want[f].append(k)
    assert sorted(want) == sorted(MU.FACTORIES) and len(want) == 10
    assert sorted(n for n in CM.__all__ if n.startswith('cait_')) == sorted(MU.FACTORIES)
    for f in want:                                         # the seven large ones build as well
        assert _keys(getattr(PM, f)()) == want[f], f


def test_refusals_are_by_name():
    for kw, word in ((dict(drop_rate=0.1), 'drop_rate'), (dict(attn_drop_rate=0.1), 'attn_drop_rate'),
                     (dict(qk_scale=0.5), 'qk_scale'), (dict(embed_dim=100), 'multiple')):
        with pytest.raises(NotImplementedError, match=word):
            _cpu_model(name='Cait', **dict(MU.MODEL, **kw))
    with pytest.raises(ValueError):
        _cpu_model(name='Cait', **dict(MU.MODEL, drop_path_rate=1.0))
    assert _cpu_model(name='Cait', **dict(MU.MODEL, drop_rate=0.0)).drop_path_rate == 0.


def test_the_yaml_loads_and_the_engine_builds_its_no_decay_groups(tmp_path):
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    path = os.path.join(ROOT, 'configs', 'v2', 'cait_s24_224_synthetic.yaml')
    header = open(path).read().split('\nGlobal:')[0]
    for word in ('TimmAutoAugment', 'TransformOpSampler', 'RandomResizedCrop', 'RepeatedAugSampler', 'GradScaler'):
        assert word in header, 'the header must say that %s is left out' % word
    cfg = get_config(path, ['Global.device=cpu', 'Global.output_dir=%s' % tmp_path,
                            'DataLoader.Train.dataset.num_samples=16', 'DataLoader.Train.dataset.num_classes=8',
                            'DataLoader.Train.sampler.batch_size=8', 'DataLoader.Eval.dataset.num_samples=8',
                            'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=8'])
    assert cfg['Model'] == dict(name='cait_s24_224', drop_path_rate=0.1, drop_rate=0.0, num_classes=1000)
    assert cfg['LRScheduler']['name'] == 'TimmCosine' and cfg['LRScheduler']['learning_rate'] == 1e-3
    assert cfg['LRScheduler']['eta_min'] == 1e-5 and cfg['LRScheduler']['warmup_start_lr'] == 1e-6
    assert cfg['LRScheduler']['decay_unit'] == 'epoch' and cfg['LRScheduler']['warmup_epoch'] == 5
    assert cfg['Optimizer']['weight_decay'] == 0.05 and list(cfg['Optimizer']['no_weight_decay_name']) == MU.NO_DECAY
    assert cfg['Optimizer']['eps'] == 1e-8 and cfg['Global']['seed'] == 2022 and cfg['Global']['epochs'] == 400
    assert 'grad_clip' not in cfg['Optimizer']
    cfg['Model'] = dict(name='Cait', drop_path_rate=0.5, **MU.MODEL)
    eng = Engine(cfg, mode='train')
    fx = MU.load('cait_small')
    assert eng.no_weight_decay_names(MU.NO_DECAY) == list(fx['no_decay'])
    table = {n: wd for rows in eng.optimizer._param_table for n, _s, wd in rows}
    assert collections.Counter(table.values()) == {0.0: len(fx['no_decay']),
                                                   0.05: len(list(eng.model.parameters())) - len(fx['no_decay'])}
    assert eng.lr_decay_unit == 'epoch'


def test_fixture_holds_what_the_issue_lists():
    for name, rate in MU.CASES.items():
        fx = MU.load(name)
        grads = [k for k in fx if k.startswith('s0_grad/')]
        assert len(grads) == len(fx['keys']) and 's1_loss' in fx and 's0_logits' in fx and float(fx['rate']) == rate
        finals = {k[len('final/'):] for k in fx if k.startswith('final/')}
        assert finals == {k.split(':')[0] for k in fx['keys']
                          if int(np.prod([int(s) for s in k.split(':')[1].split('x')])) <= MU.FINAL_MAX}
        if rate:
            assert fx['s0_keep'].shape == (2 * MU.MODEL['depth'], MU.BATCH)
        zero = MU.zero_grad_names([k.split(':')[0] for k in fx['keys']])
        assert len(zero) == 2 + 2 + 2                     # proj_l.bias x 2 trunk blocks, qkv.bias x 2, k.bias x 2
        for n in zero:
            g = fx['s0_grad/' + n]
            if n.endswith('qkv.bias'):
                g = g[g.size // 3:2 * g.size // 3]        # the key third
            assert float(np.abs(g).max()) <= 1e-6, n
