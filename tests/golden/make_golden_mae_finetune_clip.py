"""Generate tests/golden/mae_ft_clip_small.npz by EXECUTING THE REFERENCE's fine-tuning sources WITH ITS GRADIENT CLIPPING —
the twin of make_golden_mae_finetune_lrd.py: same model, state, inputs (Generator().manual_seed(909)) and solver, N = 8,
3 steps, the groups of its run A (the v2 layer-decay rule on the backbone + the head as two groups: 13 groups), all
through the reference's optimizer passl/optimizer/adamw.py.

    python tests/golden/make_golden_mae_finetune_clip.py

passl/core/grad_clip.py is executed from the reference tree under the shim (oracle/paddle_shim.py); the few Paddle names it
needs and the shim lacks are added HERE, at run time, each as a one-line statement of the Paddle op (``_shim_for_clip``).
Three runs, each from the same state:
  N  no clipping.  Its losses must equal run A of mae_ft_lrd_small.npz (asserted).
  P  AdamW(groups, grad_clip=ClipGradByGlobalNorm(clip_norm=1.0)): the optimizer calls the object once per group
     (adamw.py:53-55) — one norm set per group.
  T  clip_grad_norm_(model.parameters(), 1.0) between backward and step() (main_finetune.py --clip_grad): one set over
     all parameters, coefficient min(1 / (norm + 1e-6), 1) whatever the norm.
Adam is invariant to a constant gradient scale, so parameters barely tell clipped from unclipped: the MOMENTS are stored.
Per run and step: the loss; exp_avg / exp_avg_sq element by element for the ELEMENTWISE tensors and their float64 norms for
the WATCH list; every set's norm and coefficient recomputed in float64 from the reference's (unclipped) gradients.
tests/grad_clip_util.check_golden states what the file must satisfy; it is asserted here before the file is written."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import ref_runner, ref_runner_v2       # noqa: E402
import grad_clip_util                                   # noqa: E402
import make_golden_mae_finetune_lrd as LRD         # noqa: E402

CLIP_NORM = 1.0
# the six tensors of the lrd fixture lie in groups that run P never clips (1-D parameters: group norms 0.1 - 0.9); the
# head's weight (2048 elements) lies in the group with the largest norm (3.8 - 4.3), clipped at every step
ELEMENTWISE = list(LRD.ELEMENTWISE) + ['head.fc_cls.weight']
WATCH = list(LRD.WATCH)


def _shim_for_clip():
    """What passl/core/grad_clip.py uses and the shim does not define  [Paddle-semantics], one statement each."""
    import paddle
    c_ops = paddle._legacy_C_ops
    if not hasattr(c_ops, 'squared_l2_norm'):
        c_ops.squared_l2_norm = lambda x: (x * x).sum().reshape(1)      # [Paddle-semantics] squared_l2_norm: sum(x^2), shape [1]
    if not hasattr(torch.Tensor, 'scale_'):
        torch.Tensor.scale_ = lambda self, scale: self.mul_(scale)       # [Paddle-semantics] Tensor.scale_: x *= scale, in place
    if not hasattr(paddle, 'clip'):
        paddle.clip = lambda x, min=None, max=None: torch.clamp(x, min=min, max=max)   # [Paddle-semantics] paddle.clip
    if not hasattr(paddle, 'sqrt'):
        paddle.sqrt = torch.sqrt                                         # [Paddle-semantics] paddle.sqrt
    if not hasattr(paddle, 'stack'):
        paddle.stack = lambda xs, axis=0: torch.stack(list(xs), dim=axis)              # [Paddle-semantics] paddle.stack
    if not hasattr(paddle, 'norm'):
        paddle.norm = lambda x, p=2.0: torch.linalg.vector_norm(x.reshape(-1), ord=p)  # [Paddle-semantics] paddle.norm (vector p-norm)
    ref_runner_v2._core_stub()
    return importlib.import_module('passl.core.grad_clip')


def _rule(norm, always_clip, clip_norm_max):
    """The coefficient of ClipGradByGlobalNorm in float64."""
    if not always_clip and norm <= CLIP_NORM:
        return 1.0
    c = CLIP_NORM / (norm + 1e-6)
    return c if clip_norm_max is None else min(c, clip_norm_max)


def run_one(run, ns, solver, lrd, builder, gc, out):
    model, keys_shapes = LRD.build(ns)
    groups = LRD.groups_of('A', model, lrd, builder)
    named = list(model.named_parameters())
    group_of = {}
    for gi, g in enumerate(groups):
        for p in g['params']:
            group_of[id(p)] = gi
    out['table_names'] = np.array([n for n, _p in named])
    out['group_of'] = np.array([group_of[id(p)] for _n, p in named], dtype=np.int64)
    kw = dict(LRD.SOLVER)
    if run == 'P':
        kw['grad_clip'] = gc.ClipGradByGlobalNorm(clip_norm=CLIP_NORM)
    opt = solver.adamw.AdamW(groups, **kw)
    ps = dict(named)
    hw = LRD.ARCH['img_size']
    gen = torch.Generator().manual_seed(909)
    for s in range(LRD.STEPS):
        x = torch.randn(LRD.N, 3, hw, hw, generator=gen)
        y = torch.randint(0, LRD.CLASSES, (LRD.N,), generator=gen)
        for p in model.parameters():
            p.grad = None
        res = model(x, y, mode='train')
        res['loss'].backward()
        pre = '%s_s%d_' % (run, s)
        # every set's norm from the UNCLIPPED gradients, float64: the groups (what P clips by) and all parameters (T)
        sq = np.zeros(len(groups), dtype=np.float64)
        for _n, p in named:
            sq[group_of[id(p)]] += float((p.grad.detach().double() ** 2).sum())
        gnorm, tnorm = np.sqrt(sq), float(np.sqrt(sq.sum()))
        out[pre + 'group_norm'] = gnorm
        out[pre + 'group_coef'] = np.array([_rule(v, False, None) for v in gnorm], dtype=np.float64)
        out[pre + 'global_norm'] = np.float64(tnorm)
        out[pre + 'global_coef'] = np.float64(_rule(tnorm, True, 1.0))
        if run == 'T':
            total = gc.clip_grad_norm_(list(model.parameters()), CLIP_NORM)
            assert abs(float(total) - tnorm) <= 1e-4 * tnorm
        opt.step()
        out[pre + 'loss'] = np.float64(res['loss'].item())
        for n in WATCH:
            st = opt.state[ps[n].name]
            out[pre + 'mnorm/' + n] = np.float64(st['exp_avg'].detach().double().norm().item())
            out[pre + 'vnorm/' + n] = np.float64(st['exp_avg_sq'].detach().double().norm().item())
        for n in ELEMENTWISE:
            st = opt.state[ps[n].name]
            assert ps[n].numel() <= 4096
            out[pre + 'm/' + n] = st['exp_avg'].detach().numpy().copy()
            out[pre + 'v/' + n] = st['exp_avg_sq'].detach().numpy().copy()
        print(run, 'step', s, 'loss %.6f' % out[pre + 'loss'], 'global norm %.4f' % tnorm,
              'group norms min %.3f max %.3f' % (gnorm.min(), gnorm.max()))
    return keys_shapes


def survey(out):
    for s in range(LRD.STEPS):
        print('step', s, 'N group norms', np.array2string(out['N_s%d_group_norm' % s], precision=3))
    names = [str(n) for n in out['table_names']]
    for n in ELEMENTWISE:
        g = int(out['group_of'][names.index(n)])
        print('%-40s group %2d' % (n, g), ' P vs N %s' % ['%.3f' % grad_clip_util.m_dist(out, 'P', 'N', s, n) for s in range(LRD.STEPS)],
              ' T vs N %s' % ['%.3f' % grad_clip_util.m_dist(out, 'T', 'N', s, n) for s in range(LRD.STEPS)],
              ' P vs T %s' % ['%.3f' % grad_clip_util.m_dist(out, 'P', 'T', s, n) for s in range(LRD.STEPS)])


if __name__ == '__main__':
    assert ref_runner.available() and ref_runner_v2.available(), 'needs the reference tree'
    ns = ref_runner.load()
    solver = ref_runner_v2.load_solver(ref_runner_v2.load())
    lrd, builder = LRD.load_rules()
    gc = _shim_for_clip()
    out = {}
    for run in grad_clip_util.RUNS:
        keys_shapes = run_one(run, ns, solver, lrd, builder, gc, out)
    ref = np.load(os.path.join(HERE, 'mae_ft_lrd_small.npz'))
    for s in range(LRD.STEPS):
        assert float(out['N_s%d_loss' % s]) == float(ref['A_s%d_loss' % s]), ('run N is not run A of the lrd fixture', s)
    out['meta'] = np.array([LRD.N, LRD.ARCH['img_size'], LRD.STEPS, LRD.CLASSES], dtype=np.int64)
    out['lr'] = np.float64(LRD.SOLVER['lr'])
    out['weight_decay'] = np.float64(LRD.SOLVER['weight_decay'])
    out['layer_decay'] = np.float64(LRD.LAYER_DECAY)
    out['clip_norm'] = np.float64(CLIP_NORM)
    out['watch'] = np.array(WATCH)
    out['elementwise'] = np.array(ELEMENTWISE)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    survey(out)
    grad_clip_util.check_golden(out)
    path = os.path.join(HERE, 'mae_ft_clip_small.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
