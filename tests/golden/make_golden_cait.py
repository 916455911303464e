"""Generate tests/golden/cait_small.npz, cait_small_dp.npz and cait_layers.npz by EXECUTING THE REFERENCE's CaiT
(passl/models/cait.py: ClassAttn, LayerScaleBlockClassAttn, TalkingHeadAttn, LayerScaleBlock, Cait; Mlp / PatchEmbed /
DropPath of passl/models/vision_transformer.py; passl/loss CELoss) on torch-CPU through the paddle shim
(oracle/ref_runner_v2.py shows how the v2 tree is imported).

    python tests/golden/make_golden_cait.py          # its own process
    python tests/golden/make_golden_cait.py --check  # run again and compare with the committed files, exactly

The model is tests/cait_model_util.py's: 8 x 20 input, 4-pixel patches (10 patch tokens), width 96 = 2 heads of 48,
2 trunk and 2 token-only blocks, mlp_ratio 0.5, 8 classes, batch 2, the seed-defined state and inputs; one file per
``drop_path_rate`` (0 and 0.5), two training steps each.  Recorded: logits, loss and EVERY parameter gradient of step 0,
the loss of step 1, the parameters of at most ``FINAL_MAX`` elements after the two AdamW steps (decay 0 for the names of
the config's ``no_weight_decay_name``; no clipping, the recipe has none), with a rate the keep table of each step —
built from the draws of ``paddle.rand`` (wrapped here to record them) as floor(float32(1 - p) + u), two per trunk
block —, the state_dict key list, the no-decay name list.  cait_layers.npz: the outputs of one TalkingHeadAttn and one
ClassAttn on recorded inputs (the host test holds tests/cait_util.py's restatement against them) and the state_dict
keys and shapes of the ten factories.

Supplied HERE, in this process only, because oracle/paddle_shim.py lacks them (restated assumptions
[Paddle-semantics]):
  * ``paddle.concat(xs, axis)`` = torch.cat;  ``paddle.ParamAttr(name=...)`` carries a name and nothing else;
  * ``Layer.create_parameter(shape, attr=...)`` = an fp32 Parameter of that shape;
  * ``Tensor.expand(shape)`` / ``Tensor.reshape(shape)`` with one tuple or list = torch's with the unpacked sizes;
    ``Tensor.transpose(perm)`` with a tuple or list = permute;  keyword ``axis=`` of ``Tensor.unsqueeze`` /
    ``Tensor.mean`` = torch's ``dim``;  ``Tensor.astype`` = a cast;
  * ``nn.functional.softmax(x, axis)`` = softmax over that axis;  ``nn.Linear`` keeps its weight [in, out] (the shim's);
  * ``nn.LayerList`` = a ModuleList, ``nn.Identity`` / ``nn.Dropout(0)`` pass through;
  * ``to_2tuple`` of passl/models/vision_transformer.py passes a tuple through, so that PatchEmbed accepts the
    non-square ``img_size`` of the fixture;
  * ``scipy.special`` is imported by cait.py and never used: an empty module stands in when SciPy is absent;
  * ``passl.nn.init.trunc_normal_ / zeros_ / constant_``: initial values only (the state is overwritten);
  * AdamW: the statement of the Paddle ``adamw`` op in oracle/ref_runner_v2.py (``_adamw_op``), beta powers b^t at step t.
Whatever of these the shim already has is left as it is (each piece is installed only when missing or failing)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import cait_model_util as MU                                              # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402


def _seq(args):
    return tuple(args[0]) if len(args) == 1 and isinstance(args[0], (tuple, list)) else None


def load_reference():
    """-> (namespace with .cait and .loss, the paddle module)."""
    import importlib
    ns = ref_runner_v2.load_solver()
    paddle = sys.modules['paddle']
    nn = paddle.nn
    supplied = {
        'concat': lambda xs, axis=0: torch.cat(list(xs), dim=axis),
        'floor': torch.floor,
        'ParamAttr': lambda name=None, **kw: types.SimpleNamespace(name=name),
    }
    for name, fn in supplied.items():
        if not hasattr(paddle, name):
            setattr(paddle, name, fn)
    try:
        import scipy.special                                              # noqa: F401
    except ImportError:
        sys.modules.setdefault('scipy', types.ModuleType('scipy'))
        sys.modules.setdefault('scipy.special', types.ModuleType('scipy.special'))
        sys.modules['scipy'].special = sys.modules['scipy.special']
    T = torch.Tensor
    if not hasattr(T, 'astype'):
        T.astype = lambda self, dt: self.to(getattr(torch, dt) if isinstance(dt, str) else dt)
    t_transpose, t_unsqueeze, t_mean, t_expand, t_reshape = T.transpose, T.unsqueeze, T.mean, T.expand, T.reshape

    def transpose(self, *args, perm=None):
        perm = perm if perm is not None else _seq(args)
        return self.permute(*perm) if perm is not None else t_transpose(self, *args)

    def unsqueeze(self, *args, axis=None):
        return t_unsqueeze(self, axis) if axis is not None else t_unsqueeze(self, *args)

    def mean(self, *args, axis=None, **kw):
        return t_mean(self, dim=axis, **kw) if axis is not None else t_mean(self, *args, **kw)

    def expand(self, *args):
        s = _seq(args)
        return t_expand(self, *s) if s is not None else t_expand(self, *args)

    def reshape(self, *args):
        s = _seq(args)
        return t_reshape(self, *s) if s is not None else t_reshape(self, *args)
    T.transpose, T.unsqueeze, T.mean, T.expand, T.reshape = transpose, unsqueeze, mean, expand, reshape
    f_softmax = getattr(nn.functional, 'softmax', None)

    def softmax(x, axis=-1, **kw):
        return torch.softmax(x, dim=axis)
    try:
        f_softmax(torch.zeros(1, 2), axis=-1)
    except Exception:
        nn.functional.softmax = softmax
    try:
        nn.Layer().create_parameter(shape=(1, 1, 2), attr=paddle.ParamAttr(name='x'))
    except Exception:
        nn.Layer.create_parameter = lambda self, shape, attr=None, **kw: torch.nn.Parameter(torch.zeros(*shape))
    for name, cls in (('LayerList', torch.nn.ModuleList), ('Identity', torch.nn.Identity)):
        if not hasattr(nn, name):
            setattr(nn, name, cls)
    init = sys.modules['passl.nn.init']

    def keep(tensor, *a, **k):
        return tensor
    init.trunc_normal_ = init.zeros_ = init.constant_ = keep
    vt = importlib.import_module('passl.models.vision_transformer')
    vt.to_2tuple = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    ns.cait = importlib.import_module('passl.models.cait')
    return ns, paddle


def params_of(model):
    return dict(model.named_parameters())


def no_decay_names(params):
    return [n for n in params if any(nd in n for nd in MU.NO_DECAY)]


def set_state(layer):
    state = MU.fixture_state([(k, tuple(v.shape)) for k, v in layer.state_dict().items()])
    with torch.no_grad():
        for k, v in layer.state_dict().items():
            v.copy_(state[k])
    return state


def record_layers(ns):
    """cait_layers: one TalkingHeadAttn and one ClassAttn of the reference on recorded inputs, and the state_dict keys
    and shapes of the ten factories."""
    Cm = ns.cait
    out = {}
    gen = torch.Generator().manual_seed(78)
    th = Cm.TalkingHeadAttn(dim=96, num_heads=2, qkv_bias=True)
    ca = Cm.ClassAttn(dim=144, num_heads=3, qkv_bias=True)
    for layer, name, shape in ((th, 'th', (2, 11, 96)), (ca, 'ca', (2, 7, 144))):
        layer.eval()
        set_state(layer)
        x = torch.randn(*shape, generator=gen)
        with torch.no_grad():
            out[name + '/x'] = x.numpy().copy()
            out[name + '/out'] = layer(x).numpy().copy()
        for k, v in layer.state_dict().items():
            out[name + '/state/' + k] = v.detach().numpy().copy()
    # one byte string: an array of Python strings is stored at four bytes a character
    out['factory_keys'] = np.frombuffer('\n'.join(factory_keys(ns)).encode(), dtype=np.uint8)
    return out


def run_case(ns, paddle, name, rate, write=True):
    model = ns.cait.Cait(drop_path_rate=rate, **MU.MODEL)
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    state = set_state(model)
    params = params_of(model)
    assert sorted(state) == sorted(params), 'every parameter, and nothing else, has a seed-defined value'
    model.train()
    keep_prob = MU.keep_probs(rate)
    celoss = ns.loss.celoss.CELoss()
    draws, rand0 = [], paddle.rand

    def rand(shape, *a, **k):
        u = rand0(shape, *a, **k)
        draws.append(u.detach().clone().reshape(-1))
        return u
    paddle.rand = rand
    torch.manual_seed(5)                                  # the draws of paddle.rand
    moments = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in params.items()}
    s = MU.SOLVER
    skip = set(no_decay_names(params))
    out = {}
    try:
        for step, (x, y) in enumerate(MU.batches()):
            for p in params.values():
                p.grad = None
            del draws[:]
            logits = model(x)
            loss = celoss(logits, y)['CELoss']
            loss.backward()
            assert len(draws) == len(keep_prob) and all(u.numel() == MU.BATCH for u in draws)
            if keep_prob:
                keep = np.stack([np.floor((np.float32(kp) + u.numpy().astype(np.float32)).astype(np.float32))
                                 for kp, u in zip(keep_prob, draws)]).astype(np.float32)
                assert np.all((keep == 0) | (keep == 1))
                out['s%d_keep' % step] = keep
                print(name, 'step', step, 'keep', keep.tolist())
            out['s%d_loss' % step] = np.float64(loss.item())
            if step == 0:
                out['s0_logits'] = logits.detach().numpy().copy()
                for k, p in params.items():
                    out['s0_grad/' + k] = p.grad.detach().numpy().copy()
            for k, p in params.items():
                m, v = moments[k]
                b1p = torch.tensor(s['beta1'] ** (step + 1))
                b2p = torch.tensor(s['beta2'] ** (step + 1))
                attrs = ('beta1', s['beta1'], 'beta2', s['beta2'], 'epsilon', s['epsilon'], 'with_decay', True,
                         'coeff', 0.0 if k in skip else s['weight_decay'])
                ref_runner_v2._adamw_op(p, p.grad, s['lr'], m, v, b1p, b2p, None, None, None, None, None, None, None,
                                        *attrs)
            print(name, 'step', step, 'loss %.6f' % loss.item())
    finally:
        paddle.rand = rand0
    for k, p in params.items():
        if p.numel() <= MU.FINAL_MAX:
            out['final/' + k] = p.detach().numpy().copy()
    if keep_prob:
        k0 = out['s0_keep']
        assert (k0 == 0).any() and (k0 == 1).any(), 'step 0 must both drop and keep'
    out['rate'] = np.float64(rate)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    out['no_decay'] = np.array(no_decay_names(params))
    out['model_no_weight_decay'] = np.array(sorted(model.no_weight_decay()))
    if write:
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print('wrote', path, os.path.getsize(path), 'bytes')
    return out


def factory_keys(ns):
    """'factory|key:shape' of every state_dict entry of the ten factories as the reference classes build them."""
    rows = []
    for f in MU.FACTORIES:
        for k, v in getattr(ns.cait, f)().state_dict().items():
            rows.append('%s|%s:%s' % (f, k, 'x'.join(map(str, v.shape))))
    return rows


def main(argv):
    assert ref_runner_v2.available(), 'needs the reference tree'
    ns, paddle = load_reference()
    check = '--check' in argv
    bad = []
    for name, rate in list(MU.CASES.items()) + [(MU.LAYERS, None)]:
        if rate is None:
            out = record_layers(ns)
            if not check:
                np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
                print('wrote', name, os.path.getsize(os.path.join(HERE, name + '.npz')), 'bytes')
        else:
            out = run_case(ns, paddle, name, rate, write=not check)
        if check:
            have = MU.load(name)
            bad += ['%s: %s' % (name, k) for k in sorted(set(out) | set(have))
                    if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
    if check:
        print('DIFFERENT: %s' % bad if bad else 'fixtures equal the live reference run')
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main(sys.argv[1:])
