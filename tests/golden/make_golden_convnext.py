"""Generate tests/golden/convnext_small.npz and convnext_small_dp.npz by EXECUTING THE REFERENCE's ConvNeXt
(passl/models/convnext.py: LayerNorm, Block, ConvNeXt; DropPath / drop_path() of passl/models/vision_transformer.py;
passl/loss CELoss) on torch-CPU through the paddle shim (oracle/ref_runner_v2.py shows how the v2 tree is imported).

    python tests/golden/make_golden_convnext.py          # its own process

The model is tests/convnext_model_util.py's: depths [1, 1, 2, 1], dims [8, 16, 32, 64], 8 classes, input
2 x 3 x 64 x 96, the seed-defined state (gammas of order 1) and inputs; one file per ``drop_path_rate`` (0 and 0.5), two
training steps each.  Recorded: logits, loss and EVERY parameter gradient of step 0, the loss of step 1, every parameter
after the two AdamW steps, the drop-path ladder and, with a rate, the keep table of each step — built from the draws of
``paddle.rand`` (wrapped here to record them) as floor(float32(1 - p) + u), the way the mae_ft_dp_* fixtures do, so that
the product fed the table sees the reference's keep decisions.

Supplied HERE, in this process only, because oracle/paddle_shim.py lacks them (restated assumptions
[Paddle-semantics]):
  * ``paddle.nn.Conv2D`` with ``groups``: a subclass of the shim's class that keeps its parameters and calls
    torch.nn.functional.conv2d(groups=...) — zero padding, cross-correlation, weight [out, in / groups, kh, kw];
  * ``paddle.nn.functional.layer_norm(x, shape, weight, bias, epsilon)``: biased variance over the last axis;
  * ``Tensor.transpose(perm=[...])`` as a keyword = permute;  ``paddle.floor`` / ``paddle.sqrt`` = torch's;
  * AdamW: the statement of the Paddle ``adamw`` op in oracle/ref_runner_v2.py (``_adamw_op``), decay on every
    parameter, beta powers b^t at step t.
  * ``passl.nn.init.trunc_normal_`` = torch's (initial values only: the state is overwritten).
``paddle.linspace`` (float32), ``nn.Identity`` and ``paddle.rand`` are the shim's own."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import convnext_model_util as MU                                          # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402


def load_reference():
    """-> (namespace with .convnext and .loss, the paddle module)."""
    import importlib
    ns = ref_runner_v2.load_solver()
    paddle = sys.modules['paddle']
    nn, F = paddle.nn, paddle.nn.functional
    base_conv = nn.Conv2D

    class GroupedConv2D(base_conv):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, **kw):
            super().__init__(in_channels // groups, out_channels, kernel_size, stride=stride, padding=padding, **kw)
            self._groups = groups

        def forward(self, x):
            return TF.conv2d(x, self.weight, self.bias, self._stride, self._padding, 1, self._groups)
    nn.Conv2D = GroupedConv2D
    if not hasattr(F, 'layer_norm'):
        F.layer_norm = lambda x, shape, weight=None, bias=None, epsilon=1e-5: TF.layer_norm(
            x, tuple(shape), weight, bias, epsilon)
    for fn in ('floor', 'sqrt'):
        if not hasattr(paddle, fn):
            setattr(paddle, fn, getattr(torch, fn))
    shim_transpose = torch.Tensor.transpose

    def transpose(self, *args, perm=None):
        return self.permute(*perm) if perm is not None else shim_transpose(self, *args)
    torch.Tensor.transpose = transpose
    # the constructor's initial values are overwritten by the seed-defined state: passl/nn/init.py's trunc_normal_ (which
    # needs Tensor.scale_ and clip_(min=, max=), absent from the shim) is answered by torch's, not executed
    init = sys.modules['passl.nn.init']

    def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
        with torch.no_grad():
            return torch.nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)
    init.trunc_normal_ = trunc_normal_
    ns.convnext = importlib.import_module('passl.models.convnext')
    return ns, paddle


def run_case(ns, paddle, name, rate, write=True):
    model = ns.convnext.ConvNeXt(drop_path_rate=rate, **MU.MODEL)
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    state = MU.fixture_state(keys_shapes)
    with torch.no_grad():
        for k, v in sd.items():
            v.copy_(state[k])
    model.train()
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(sd)
    rates, keep_prob = MU.ladder(rate)
    droppers = [m for m in model.modules() if type(m).__name__ == 'DropPath']
    assert len(droppers) == len(keep_prob)
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
    attrs = ('beta1', s['beta1'], 'beta2', s['beta2'], 'epsilon', s['epsilon'], 'with_decay', True,
             'coeff', s['weight_decay'])
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
                ref_runner_v2._adamw_op(p, p.grad, s['lr'], m, v, b1p, b2p, None, None, None, None, None, None, None,
                                        *attrs)
            print(name, 'step', step, 'loss %.6f' % loss.item())
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
    if write:
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print('wrote', path, os.path.getsize(path), 'bytes')
    return out


def reference_keys(ns):
    """{model name: [[key, shape], ...]} of the small model and the five factories as the reference classes build them
    (their initialisers switched off: only names and shapes are read)."""
    init = sys.modules['passl.nn.init']
    init.trunc_normal_ = init.constant_ = lambda tensor, *a, **k: tensor
    C = ns.convnext
    models = {'small': lambda: C.ConvNeXt(**MU.MODEL)}
    for f in ('convnext_tiny', 'convnext_small', 'convnext_base', 'convnext_large', 'convnext_xlarge'):
        models[f] = getattr(C, f)
    return {n: [[k, list(v.shape)] for k, v in make().state_dict().items()] for n, make in models.items()}


def main(argv):
    """no argument: write the two files.  --check: run the reference again and compare with the committed files, array
    by array, exactly (exit status 1 on a difference); then print the reference's state_dict keys and shapes as one JSON
    line (tests/test_convnext_host.py reads both)."""
    assert ref_runner_v2.available(), 'needs the reference tree'
    ns, paddle = load_reference()
    check = '--check' in argv
    bad = []
    for name, rate in MU.CASES.items():
        out = run_case(ns, paddle, name, rate, write=not check)
        if check:
            have = MU.load(name)
            bad += ['%s: %s' % (name, k) for k in sorted(set(out) | set(have))
                    if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
    if check:
        import json
        print('DIFFERENT: %s' % bad if bad else 'fixtures equal the live reference run')
        print('KEYS ' + json.dumps(reference_keys(ns)))
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main(sys.argv[1:])
