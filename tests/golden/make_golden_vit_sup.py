"""Generate tests/golden/vit_sup_small.npz by EXECUTING THE REFERENCE's two classes of the supervised ViT recipe on
torch-CPU through the paddle shim: passl/scheduler/lr_scheduler.py ViTLRScheduler (over the shim's statement of
paddle.optimizer.lr.LRScheduler) and passl/loss/celoss.py ViTCELoss.

    python tests/golden/make_golden_vit_sup.py          # its own process

One Paddle call of ViTCELoss is missing from the shim and is supplied HERE, not executed from the reference:
``F.binary_cross_entropy_with_logits(x, label, reduction='none')`` = max(x, 0) - x * label + log1p(exp(-|x|))
[Paddle-semantics: paddle/phi/kernels/cpu/sigmoid_cross_entropy_with_logits_kernel.cc], evaluated by torch's function of
the same name with the label cast to the logits' dtype.  Logits are float64, so the recorded losses are float64 values;
the label is smoothed by the reference's own line (in the float32 of F.one_hot's result).

Seed-defined inputs: logits ~ 4 N(0,1) from torch.Generator().manual_seed(77) with +-40 planted, labels from the same
generator; the schedules are pure functions of their arguments.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_runner_v2                                         # noqa: E402

# name -> constructor arguments; every schedule is stepped from its construction to two steps past T_max
SCHEDULES = {
    'cos_warm': dict(learning_rate=3e-3, step_each_epoch=5, epochs=4, decay_type='cosine', warmup_steps=6),
    'lin_warm': dict(learning_rate=3e-3, step_each_epoch=5, epochs=4, decay_type='linear', linear_end=1e-5,
                     warmup_steps=6),
    'cos_plain': dict(learning_rate=0.1, step_each_epoch=3, epochs=3, decay_type='cosine'),
    'lin_plain': dict(learning_rate=0.1, step_each_epoch=3, epochs=3, decay_type='linear', linear_end=0.01),
    'cos_warm_long': dict(learning_rate=1.0, step_each_epoch=4, epochs=2, decay_type='cosine', warmup_steps=7),
}
LOSSES = [(3, 5), (2, 1000), (2, 1001)]
EPSILONS = {'none': None, '1e-4': 1e-4}


def main():
    ns = ref_runner_v2.load_solver()
    import paddle.nn.functional as F
    import torch.nn.functional as TF
    assert not hasattr(F, 'binary_cross_entropy_with_logits'), 'the shim has it now: drop the stand-in below'
    F.binary_cross_entropy_with_logits = lambda logit, label, reduction='mean': \
        TF.binary_cross_entropy_with_logits(logit, label.to(logit.dtype), reduction=reduction)
    out = {'sched_args': np.array(json.dumps(SCHEDULES))}       # what each schedule was built with, for the test
    for name, kw in SCHEDULES.items():
        s = ns.lr_scheduler.ViTLRScheduler(**kw)
        T = kw['epochs'] * kw['step_each_epoch']
        lrs = [s.get_lr()]                      # after the base constructor's first step(): last_epoch 0
        assert s.last_epoch == 0
        for _ in range(T + 2):
            s.step()
            lrs.append(s.get_lr())
        out['sched/' + name] = np.asarray(lrs, dtype=np.float64)
        print(name, ['%.3e' % v for v in lrs[:8]], '...')
    gen = torch.Generator().manual_seed(77)
    for N, C in LOSSES:
        x = torch.randn(N, C, generator=gen, dtype=torch.float64) * 4
        y = torch.randint(0, C, (N,), generator=gen)
        x[0, int(y[0])] = -40.0                 # a confident miss, a confident hit and a confident false alarm
        x[1, int(y[1])] = 40.0
        x[0, (int(y[0]) + 1) % C] = 40.0
        out['loss/x_%dx%d' % (N, C)] = x.numpy().copy()
        out['loss/y_%dx%d' % (N, C)] = y.numpy().copy()
        for tag, eps in EPSILONS.items():
            xr = x.clone().requires_grad_(True)
            loss = ns.loss.celoss.ViTCELoss(epsilon=eps)(xr, y)['ViTCELoss']
            loss.backward()
            out['loss/value_%dx%d_%s' % (N, C, tag)] = np.float64(float(loss))
            out['loss/grad_%dx%d_%s' % (N, C, tag)] = xr.grad.numpy().copy()
            print('ViTCELoss', (N, C), tag, float(loss))
    path = os.path.join(HERE, 'vit_sup_small.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
