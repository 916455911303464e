"""Generate tests/golden/swin_small.npz, swin_small_dp.npz and swin_layers.npz by EXECUTING THE REFERENCE's Swin Transformer
(passl/models/swin_transformer.py: WindowAttention, SwinTransformerBlock, PatchMerging, BasicLayer, SwinTransformer;
Mlp / PatchEmbed / DropPath of passl/models/vision_transformer.py; passl/loss CELoss) on torch-CPU through the paddle
shim (oracle/ref_runner_v2.py shows how the v2 tree is imported).

    python tests/golden/make_golden_swin.py          # its own process

The model is tests/swin_model_util.py's: 32 x 64 input, embed_dim 32, depths (2, 2), heads (1, 2), window 4, mlp_ratio 2, 8 classes,
batch 2, the seed-defined state (bias tables of order 0.5) and inputs; one file per ``drop_path_rate`` (0 and 0.5), two
training steps each.  Recorded: logits, loss and EVERY parameter gradient of step 0, the loss of step 1, every parameter
after the two AdamW steps (decay 0 for the names of the config's ``no_weight_decay_name``, global-norm clipping at 5),
the two groups' gradient norms, the drop-path ladder, with a rate the keep table of each step — built from the draws of
``paddle.rand`` (wrapped here to record them) as floor(float32(1 - p) + u) —, the state_dict key list, the no-decay
name list.  swin_layers.npz: the outputs of one WindowAttention and one shifted SwinTransformerBlock on recorded inputs
(the host test holds tests/swin_util.py's restatement against them) and the state_dict keys and shapes of the thirteen
factories.

Supplied HERE, in this process only, because oracle/paddle_shim.py lacks them (restated assumptions
[Paddle-semantics]):
  * ``paddle.roll(x, shifts, axis)`` = torch.roll(x, shifts, dims);  ``paddle.stack`` / ``paddle.ones_like`` /
    ``paddle.index_select(x, index)`` (axis 0) / ``paddle.meshgrid`` ('ij' indexing) / ``paddle.flatten`` = torch's;
  * ``nn.Softmax(axis)`` = softmax over that axis;  ``Tensor.astype('float32')`` = a cast;
  * keyword ``axis=`` of ``Tensor.unsqueeze`` / ``Tensor.mean`` = torch's ``dim``;  ``Tensor.transpose(perm)`` with a
    tuple or list = permute;
  * ``Layer.create_parameter(shape)`` = an fp32 Parameter;  ``Layer.register_buffer(name, None)`` keeps no entry;
  * ``to_2tuple`` of passl/models/vision_transformer.py (``tuple([x] * 2)``, which nests a tuple) passes a tuple through,
    as swin_transformer.py's own ``to_2tuple`` does: PatchEmbed then accepts the non-square ``img_size`` of the fixture;
  * ``passl.nn.init.trunc_normal_ / zeros_ / constant_``: initial values only (the state is overwritten);
  * AdamW: the statement of the Paddle ``adamw`` op in oracle/ref_runner_v2.py (``_adamw_op``), beta powers b^t at step
    t; ``ClipGradByGlobalNorm(c)`` once per parameter group (decay, no decay), as the reference's optimizers call it:
    every gradient of the group times c / (norm + 1e-6) when the group's norm exceeds c (passl/core/grad_clip.py).
Whatever of these the shim already has is left as it is (each piece is installed only when missing or failing)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import swin_model_util as MU                                              # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402


def _as_dims(a):
    return tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list)) else tuple(a)


def load_reference():
    """-> (namespace with .swin and .loss, the paddle module)."""
    import importlib
    ns = ref_runner_v2.load_solver()
    paddle = sys.modules['paddle']
    nn = paddle.nn
    supplied = {
        'roll': lambda x, shifts, axis=None: torch.roll(x, shifts, dims=axis),
        'stack': lambda xs, axis=0: torch.stack(list(xs), dim=axis),
        'ones_like': torch.ones_like,
        'index_select': lambda x, index, axis=0: torch.index_select(x, axis, index),
        'meshgrid': lambda *xs: torch.meshgrid(*_as_dims(xs), indexing='ij'),
        'flatten': lambda x, start_axis=0, stop_axis=-1: torch.flatten(x, start_axis, stop_axis),
        'floor': torch.floor,
    }
    for name, fn in supplied.items():
        if not hasattr(paddle, name):
            setattr(paddle, name, fn)
    if not hasattr(nn, 'Softmax'):
        class Softmax(nn.Layer):
            def __init__(self, axis=-1):
                super().__init__()
                self.axis = axis

            def forward(self, x):
                return torch.softmax(x, dim=self.axis)
        nn.Softmax = Softmax
    T = torch.Tensor
    if not hasattr(T, 'astype'):
        T.astype = lambda self, dt: self.to(getattr(torch, dt) if isinstance(dt, str) else dt)
    t_transpose, t_unsqueeze, t_mean = T.transpose, T.unsqueeze, T.mean

    def transpose(self, *args, perm=None):
        if perm is None and len(args) == 1 and isinstance(args[0], (tuple, list)):
            perm = args[0]
        return self.permute(*perm) if perm is not None else t_transpose(self, *args)

    def unsqueeze(self, *args, axis=None):
        return t_unsqueeze(self, axis) if axis is not None else t_unsqueeze(self, *args)

    def mean(self, *args, axis=None, **kw):
        return t_mean(self, dim=axis, **kw) if axis is not None else t_mean(self, *args, **kw)
    T.transpose, T.unsqueeze, T.mean = transpose, unsqueeze, mean
    if not hasattr(nn.Layer, 'create_parameter'):
        nn.Layer.create_parameter = lambda self, shape, **kw: torch.nn.Parameter(torch.zeros(*shape))
    init = sys.modules['passl.nn.init']

    def keep(tensor, *a, **k):
        return tensor
    init.trunc_normal_ = init.zeros_ = init.constant_ = keep
    ns.swin = importlib.import_module('passl.models.swin_transformer')
    # a non-square img_size: swin_transformer.py's own to_2tuple passes a tuple through, vision_transformer.py's (used by
    # PatchEmbed) would nest it
    vt = sys.modules['passl.models.vision_transformer']
    vt.to_2tuple = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    return ns, paddle


def params_of(model):
    """Trainable parameters by state_dict name (the buffers are not parameters)."""
    return dict(model.named_parameters())


def no_decay_names(params):
    return [n for n in params if any(nd in n for nd in MU.NO_DECAY)]


def record_layers(ns):
    """swin_layers: one WindowAttention (with a mask) and one shifted SwinTransformerBlock of the reference on recorded
    inputs, and the state_dict keys and shapes of the thirteen factories."""
    S = ns.swin
    out = {}
    gen = torch.Generator().manual_seed(77)
    blk = S.SwinTransformerBlock(dim=64, input_resolution=(8, 12), num_heads=2, window_size=4, shift_size=2)
    blk.eval()
    state = MU.fixture_state([(k, tuple(v.shape)) for k, v in blk.state_dict().items()])
    with torch.no_grad():
        for k, v in blk.state_dict().items():
            if k in state:
                v.copy_(state[k])
    x = torch.randn(2, 8 * 12, 64, generator=gen)
    xw = torch.randn(2 * 6, 16, 64, generator=gen)
    with torch.no_grad():
        out['layer/x'] = x.numpy().copy()
        out['layer/block_out'] = blk(x).numpy().copy()
        out['layer/xw'] = xw.numpy().copy()
        out['layer/attn_out'] = blk.attn(xw, mask=blk.attn_mask).numpy().copy()
        out['layer/attn_mask'] = blk.attn_mask.numpy().copy()
        out['layer/index'] = blk.attn.relative_position_index.numpy().copy()
    for k, v in blk.state_dict().items():
        out['layer/state/' + k] = v.detach().numpy().copy()
    # one byte string: an array of Python strings is stored at four bytes a character
    out['factory_keys'] = np.frombuffer('\n'.join(factory_keys(ns)).encode(), dtype=np.uint8)
    return out


def run_case(ns, paddle, name, rate, write=True):
    model = ns.swin.SwinTransformer(drop_path_rate=rate, **MU.MODEL)
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    state = MU.fixture_state(keys_shapes)
    params = params_of(model)
    assert sorted(state) == sorted(params), 'every parameter, and nothing else, has a seed-defined value'
    with torch.no_grad():
        for k, v in state.items():
            sd[k].copy_(v)
    model.train()
    rates, keep_prob = MU.ladder(rate)
    celoss = ns.loss.celoss.CELoss()
    draws, rand0 = [], paddle.rand

    def rand(shape, *a, **k):
        u = rand0(shape, *a, **k)
        draws.append(u.detach().clone().reshape(-1))
        return u
    paddle.rand = rand
    torch.manual_seed(4)                                  # the draws of paddle.rand
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
            # one norm per parameter group, as the reference's optimizers clip (passl/optimizer/adamw.py:53-55)
            coef = {}
            for gname, members in (('decay', [k for k in params if k not in skip]), ('no_decay', sorted(skip))):
                gnorm = float(torch.sqrt(sum((params[k].grad.float() ** 2).sum() for k in members)))
                out['s%d_gnorm_%s' % (step, gname)] = np.float64(gnorm)
                c = 1.0 if gnorm <= s['clip_norm'] else s['clip_norm'] / (gnorm + 1e-6)
                coef.update({k: c for k in members})
            for k, p in params.items():
                m, v = moments[k]
                b1p = torch.tensor(s['beta1'] ** (step + 1))
                b2p = torch.tensor(s['beta2'] ** (step + 1))
                attrs = ('beta1', s['beta1'], 'beta2', s['beta2'], 'epsilon', s['epsilon'], 'with_decay', True,
                         'coeff', 0.0 if k in skip else s['weight_decay'])
                ref_runner_v2._adamw_op(p, p.grad * coef[k], s['lr'], m, v, b1p, b2p, None, None, None, None, None, None,
                                        None, *attrs)
            print(name, 'step', step, 'loss %.6f' % loss.item(), 'norms', [out['s%d_gnorm_%s' % (step, g)] for g in ('decay', 'no_decay')])
    finally:
        paddle.rand = rand0
    for k, p in params.items():
        out['final/' + k] = p.detach().numpy().copy()
    if keep_prob:
        k0 = out['s0_keep']
        assert (k0 == 0).any() and (k0 == 1).any(), 'step 0 must both drop and keep'
    out['rate'] = np.float64(rate)
    out['dp_rates'] = np.asarray(rates, dtype=np.float64)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    out['no_decay'] = np.array(no_decay_names(params))
    out['model_no_weight_decay'] = np.array(sorted(model.no_weight_decay()))
    if write:
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print('wrote', path, os.path.getsize(path), 'bytes')
    return out


def factory_keys(ns):
    """'factory|key:shape' of every state_dict entry of the thirteen factories as the reference classes build them."""
    S = ns.swin
    rows = []
    for f in S.__all__:
        if f == 'SwinTransformer':
            continue
        for k, v in getattr(S, f)().state_dict().items():
            rows.append('%s|%s:%s' % (f, k, 'x'.join(map(str, v.shape))))
    return rows


def main(argv):
    """no argument: write the three files.  --check: run the reference again and compare with the committed files, array
    by array, exactly (exit status 1 on a difference)."""
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
