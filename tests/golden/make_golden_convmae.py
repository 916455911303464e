"""Generate tests/golden/convmae_small.npz, convvit_small.npz and convvit_small_dp.npz by EXECUTING THE REFERENCE's
ConvMAE (passl/models/convmae/conv_mae.py: MaskedAutoencoderConvViT; conv_vit.py: CMlp, CBlock, CPatchEmbed, ConvViT;
Block / DropPath of passl/models/vision_transformer.py; passl/loss CELoss) on torch-CPU through the paddle shim
(oracle/ref_runner_v2.py shows how the v2 tree is imported).

    python tests/golden/make_golden_convmae.py          # its own process
    python tests/golden/make_golden_convmae.py --check  # run again, compare with the committed files, print the keys

The models are tests/convmae_model_util.py's (the reference's fixed 224 / 56 / 28 sizes, small widths and depths), the
seed-defined state and inputs, two training steps each.  Recorded, large arrays as their first elements
(convmae_model_util.clip):
  convmae_small        the injected noise, mask, ids_restore, a slice of pred, the loss and EVERY parameter gradient of
                       step 0, the loss of step 1, every parameter after the two AdamW steps;
  convvit_small[_dp]   for global_pool False ('tok/') and True ('pool/'): logits, loss and every gradient of step 0, the
                       loss of step 1, the parameters after two steps, the drop-path ladder and, with a rate, the keep
                       table of each step — built from the draws of ``paddle.rand`` (wrapped here to record them) as
                       floor(float32(1 - p) + u), so that the product fed the table sees the reference's keep decisions.

Supplied HERE, in this process only, because oracle/paddle_shim.py lacks them (restated assumptions
[Paddle-semantics]):
  * ``paddle.nn.Conv2D`` with ``groups``: a subclass of the shim's class that keeps its parameters and calls
    torch.nn.functional.conv2d(groups=...) — zero padding, cross-correlation, weight [out, in / groups, kh, kw];
  * ``Tensor.transpose(perm)`` with a tuple / list = permute; ``paddle.einsum`` / ``floor`` / ``sqrt`` = torch's;
    ``Tensor._share_buffer_to(dst)`` = dst.copy_(self) (initial values only: the state is overwritten);
  * indexing ``x[paddle.arange(N).unsqueeze(1), ids]`` is torch's advanced indexing, which has Paddle's meaning here;
  * AdamW: the statement of the Paddle ``adamw`` op in oracle/ref_runner_v2.py (``_adamw_op``), decay on every
    parameter, beta powers b^t at step t;
  * ``passl.nn.init.trunc_normal_`` = torch's (initial values only).
``paddle.rand`` is wrapped: the masked model receives the fixture's noise (so ``random_masking`` is executed on it),
the classifier's draws are recorded."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import convmae_model_util as MU                                           # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402


def load_reference():
    """-> (namespace with .conv_mae, .conv_vit and .loss, the paddle module)."""
    ns = ref_runner_v2.load_solver()
    paddle = sys.modules['paddle']
    nn = paddle.nn
    base_conv = nn.Conv2D

    class GroupedConv2D(base_conv):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, **kw):
            super().__init__(in_channels // groups, out_channels, kernel_size, stride=stride, padding=padding, **kw)
            self._groups = groups

        def forward(self, x):
            return TF.conv2d(x, self.weight, self.bias, self._stride, self._padding, 1, self._groups)
    nn.Conv2D = GroupedConv2D
    shim_transpose = torch.Tensor.transpose

    def transpose(self, *args, perm=None):
        if perm is None and len(args) == 1 and isinstance(args[0], (tuple, list)):
            perm = args[0]
        return self.permute(*perm) if perm is not None else shim_transpose(self, *args)
    torch.Tensor.transpose = transpose
    for fn in ('einsum', 'floor', 'sqrt'):
        if not hasattr(paddle, fn):
            setattr(paddle, fn, getattr(torch, fn))
    if not hasattr(torch.Tensor, '_share_buffer_to'):
        def _share_buffer_to(self, dst):
            with torch.no_grad():
                dst.copy_(self.reshape(dst.shape))
        torch.Tensor._share_buffer_to = _share_buffer_to
    init = sys.modules['passl.nn.init']

    def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
        with torch.no_grad():
            return torch.nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)
    init.trunc_normal_ = trunc_normal_
    importlib.import_module('passl.models.utils.pos_embed')
    ref_runner_v2._pkg('passl.models.convmae', os.path.join(ref_runner_v2.REF_ROOT, 'passl', 'models', 'convmae'))
    ns.conv_vit = importlib.import_module('passl.models.convmae.conv_vit')
    ns.conv_mae = importlib.import_module('passl.models.convmae.conv_mae')
    return ns, paddle


def set_state(model):
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    state = MU.fixture_state(keys_shapes)
    with torch.no_grad():
        for k, v in sd.items():
            if k in state:
                v.copy_(state[k])
    return keys_shapes


def adamw_step(params, moments, step):
    s = MU.SOLVER
    attrs = ('beta1', s['beta1'], 'beta2', s['beta2'], 'epsilon', s['epsilon'], 'with_decay', True,
             'coeff', s['weight_decay'])
    for k, p in params.items():
        m, v = moments[k]
        b1p = torch.tensor(s['beta1'] ** (step + 1))
        b2p = torch.tensor(s['beta2'] ** (step + 1))
        ref_runner_v2._adamw_op(p, p.grad, s['lr'], m, v, b1p, b2p, None, None, None, None, None, None, None, *attrs)


def trainable(model):
    return {k: p for k, p in model.named_parameters() if not getattr(p, 'stop_gradient', False) and p.requires_grad}


def run_mae(ns, paddle):
    model = ns.conv_mae.MaskedAutoencoderConvViT(norm_layer=MU.norm_layer(paddle.nn), **MU.MAE_MODEL)
    keys_shapes = set_state(model)
    model.train()
    params = trainable(model)
    assert 'pos_embed' in params and 'decoder_pos_embed' not in params, sorted(params)[:4]
    moments = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in params.items()}
    rand0, feed = paddle.rand, []

    def rand(shape, *a, **k):
        u = feed.pop(0)
        assert list(shape) == list(u.shape)
        return u.clone()
    paddle.rand = rand
    out = {}
    try:
        for step, (imgs, _labels, noise) in enumerate(MU.batches()):
            for p in params.values():
                p.grad = None
            feed.append(noise)
            loss, pred, mask = model(imgs, MU.MASK_RATIO)
            assert not feed
            loss.backward()
            out['s%d_loss' % step] = np.float64(loss.item())
            if step == 0:
                ids_restore = torch.argsort(torch.argsort(noise, dim=1), dim=1)
                assert torch.equal(mask, (ids_restore >= MU.K).float()), 'no ties in the noise: any argsort agrees'
                out['s0_noise'] = noise.numpy().copy()
                out['s0_mask'] = mask.detach().numpy().copy()
                out['s0_ids_restore'] = ids_restore.numpy().astype(np.int32)
                out['s0_pred'] = pred.detach().numpy()[:, :MU.PRED_ROWS].copy()
                for k, p in params.items():
                    out['s0_grad/' + k] = MU.clip(p.grad.detach().numpy())
                    out['s0_gmax/' + k] = np.float64(p.grad.detach().abs().max().item())
            adamw_step(params, moments, step)
            print('convmae_small step', step, 'loss %.6f' % loss.item())
    finally:
        paddle.rand = rand0
    for k, p in params.items():
        out['final/' + k] = MU.clip(p.detach().numpy())
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    return out


def run_vit(ns, paddle, name, rate):
    out = {}
    celoss = ns.loss.celoss.CELoss()
    rates, keep_prob = MU.ladder(rate)
    for prefix, pool in MU.POOLS:
        model = ns.conv_vit.ConvViT(drop_path_rate=rate, global_pool=pool, norm_layer=MU.norm_layer(paddle.nn),
                                    **MU.VIT_MODEL)
        keys_shapes = set_state(model)
        model.train()
        params = trainable(model)
        droppers = [m for m in model.modules() if type(m).__name__ == 'DropPath']
        # one DropPath layer per block with p > 0, called at both residuals: two draws per such block and forward
        assert 2 * len(droppers) == len(keep_prob), (len(droppers), len(keep_prob))
        moments = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in params.items()}
        draws, rand0 = [], paddle.rand

        def rand(shape, *a, **k):
            u = rand0(shape, *a, **k)
            draws.append(u.detach().clone().reshape(-1))
            return u
        paddle.rand = rand
        torch.manual_seed(6)                                  # the draws of paddle.rand
        try:
            for step, (imgs, labels, _noise) in enumerate(MU.batches()):
                for p in params.values():
                    p.grad = None
                del draws[:]
                logits = model(imgs)
                loss = celoss(logits, labels)['CELoss']
                loss.backward()
                assert len(draws) == len(keep_prob) and all(u.numel() == MU.BATCH for u in draws)
                if keep_prob:
                    keep = np.stack([np.floor((np.float32(kp) + u.numpy().astype(np.float32)).astype(np.float32))
                                     for kp, u in zip(keep_prob, draws)]).astype(np.float32)
                    assert np.all((keep == 0) | (keep == 1))
                    out[prefix + 's%d_keep' % step] = keep
                    print(name, prefix, 'step', step, 'keep', keep.tolist())
                out[prefix + 's%d_loss' % step] = np.float64(loss.item())
                if step == 0:
                    out[prefix + 's0_logits'] = logits.detach().numpy().copy()
                    for k, p in params.items():
                        out[prefix + 's0_grad/' + k] = MU.clip(p.grad.detach().numpy())
                        out[prefix + 's0_gmax/' + k] = np.float64(p.grad.detach().abs().max().item())
                adamw_step(params, moments, step)
                print(name, prefix, 'step', step, 'loss %.6f' % loss.item())
        finally:
            paddle.rand = rand0
        for k, p in params.items():
            out[prefix + 'final/' + k] = MU.clip(p.detach().numpy())
        if keep_prob:
            k0 = out[prefix + 's0_keep']
            assert (k0 == 0).any() and (k0 == 1).any(), 'step 0 must both drop and keep'
        out[prefix + 'keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    out['rate'] = np.float64(rate)
    out['dp_rates'] = np.asarray(rates, dtype=np.float64)
    return out


def reference_keys(ns, paddle):
    """{model name: [[key, shape], ...]} of the small models and the two factories as the reference classes build them
    (their initialisers switched off: only names and shapes are read)."""
    init = sys.modules['passl.nn.init']
    for fn in ('trunc_normal_', 'constant_', 'xavier_uniform_', 'normal_'):
        setattr(init, fn, lambda tensor, *a, **k: tensor)
    nl = MU.norm_layer(paddle.nn)
    models = {'convmae_small': lambda: ns.conv_mae.MaskedAutoencoderConvViT(norm_layer=nl, **MU.MAE_MODEL),
              'convvit_small': lambda: ns.conv_vit.ConvViT(norm_layer=nl, **MU.VIT_MODEL),
              'convvit_small_pool': lambda: ns.conv_vit.ConvViT(norm_layer=nl, global_pool=True, **MU.VIT_MODEL),
              'convmae_convvit_base_patch16': ns.conv_mae.convmae_convvit_base_patch16,
              'convvit_base_patch16': ns.conv_vit.convvit_base_patch16}
    return {n: [[k, list(v.shape)] for k, v in make().state_dict().items()] for n, make in models.items()}


def main(argv):
    """no argument: write the three files and tests/golden/convmae_keys.json (the reference's state_dict keys and
    shapes).  --check: run the reference again and compare with the committed files, array by array, exactly (exit
    status 1 on a difference)."""
    import json
    assert ref_runner_v2.available(), 'needs the reference tree'
    ns, paddle = load_reference()
    check = '--check' in argv
    cases = [('convmae_small', lambda: run_mae(ns, paddle))]
    cases += [(name, (lambda n=name, r=rate: run_vit(ns, paddle, n, r))) for name, rate in MU.VIT_CASES.items()]
    bad = []
    for name, run in cases:
        out = run()
        if check:
            have = MU.load(name)
            bad += ['%s: %s' % (name, k) for k in sorted(set(out) | set(have))
                    if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
        else:
            path = os.path.join(HERE, name + '.npz')
            np.savez_compressed(path, **out)
            print('wrote', path, os.path.getsize(path), 'bytes')
    keys = reference_keys(ns, paddle)
    kpath = os.path.join(HERE, 'convmae_keys.json')
    if check:
        bad += ['convmae_keys.json'] if json.load(open(kpath)) != keys else []
        print('DIFFERENT: %s' % bad if bad else 'fixtures equal the live reference run')
        sys.exit(1 if bad else 0)
    json.dump(keys, open(kpath, 'w'), indent=0, sort_keys=True)
    print('wrote', kpath, os.path.getsize(kpath), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1:])
