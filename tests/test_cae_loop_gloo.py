"""engine/loops/cae_pretrain_loop.py under data parallelism, on the CPU: two gloo processes drive ``train_one_epoch`` with
a stand-in for the model and for ``forward_backward`` (the product's calls HIP kernels; the loop around it is device
agnostic).  Parameters are broadcast once, ONE reducer is created and armed before every backward pass, the schedule is
set to the global step before the update, and the replicas end equal to one process that averages both ranks'
gradients."""
from types import SimpleNamespace

import torch

from test_dp_gloo import _spawn

N, STEPS, LR = 24, 3, 0.05


def _batches(rank):
    return [(torch.full((N,), float(1 + rank + 2 * i)), None, None) for i in range(STEPS)]


def _loop_case(rank, world):
    from passl_amd.engine.loops import cae_pretrain_loop as loop
    torch.manual_seed(100 + rank)                                     # replicas start DIFFERENT: param_sync must fix it
    flat, grads = torch.randn(N), torch.zeros(N)

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(flat)                         # the parameter IS the flat buffer
            self.w.grad = grads
            self.arena = SimpleNamespace(flat=self.w.data, grads=grads, param_slices=[(0, 8), (8, 16)], reducer=None)

    class Sched(object):
        def __init__(self):
            self.seen = []

        def step(self, it):
            self.seen.append(it)

    class SGD(object):
        def __init__(self, model):
            self.m, self.grad_scale, self._learning_rate = model, 1.0, Sched()

        def get_lr(self):
            return LR

        def step(self):
            if self.m.arena.reducer is not None:
                self.m.arena.reducer.finish()
            with torch.no_grad():
                self.m.w -= LR * self.grad_scale * self.m.w.grad

        def clear_grad(self):
            self.m.w.grad.zero_()

    def forward_backward(model, images, mask, labels, num_masked, weight):
        main, mse = ((model.w * images).sum() ** 2) * 1e-2, (model.w ** 2).sum() * 1e-3
        torch.autograd.backward([main, mse], [torch.ones(()), torch.tensor(weight)])
        return main, mse

    model = Toy()
    opt = SGD(model)
    data = _batches(rank)

    class Loader(list):
        dataset = SimpleNamespace(num_masked=3)
    args = SimpleNamespace(dual_loss_weight=2.0, print_freq=2, target_mode='random', dual_loss_type='mse')
    begins, orig_begin, orig_fb = [], loop.GradReducer.begin, loop.forward_backward
    loop.GradReducer.begin = lambda self: (begins.append(1), orig_begin(self))[1]
    loop.forward_backward = forward_backward
    try:
        out = loop.train_one_epoch(model, Loader(data), opt, 2, args, log=lambda *_: None)
    finally:
        loop.GradReducer.begin, loop.forward_backward = orig_begin, orig_fb
    assert len(begins) == STEPS and opt._learning_rate.seen == [2 * STEPS + i for i in range(STEPS)]
    assert model._passl_grad_reducer is model.arena.reducer and opt.grad_scale == 1.0 / world
    assert abs(out['loss'] - (out['loss_main'] + out['loss_aux'])) < 1e-9 and out['lr'] == LR
    return model.w.detach().clone()


def test_cae_pretrain_loop_averages_gradients_across_ranks():
    out = _spawn(_loop_case)
    assert torch.equal(out[0], out[1])                                # replicas stay identical
    torch.manual_seed(100)
    w = torch.randn(N)                                                # rank 0's start, broadcast
    for i in range(STEPS):
        g = torch.zeros(N)
        for rank in range(2):
            x = _batches(rank)[i][0]
            g += 2e-2 * (w * x).sum() * x + 2.0 * 2e-3 * w
        w = w - LR * g / 2                                            # mean over the two ranks
    assert torch.allclose(out[0], w, rtol=1e-5, atol=1e-6), (out[0], w)
