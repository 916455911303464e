"""A patched training step under a strict step plan (passl_amd/hip/replay.py): every launch of the step — the matching,
the merge and its gradient included — is the library's own, so the plan records with nothing foreign in it and its
replays equal the eager twin's steps bit for bit.  Each merging block adds three launches to a step: one matching, one
merge, one merge gradient (counted here at the entry points).  The fixture model's recorded step is 130 launches with
r = [4, 3, 0] and, as it happens, 130 with r = 0: the Linear and LayerNorm launches behind a merge see fewer rows (66 and
60 in place of 74) and their reductions need fewer passes.
With the trace off nothing in the pass waits for the device: it runs under torch's sync debug mode 'error'."""
import math

import pytest
import torch

import tome_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402

DEV = 'cuda'


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _model(r, dtype=torch.float32):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(1)
    model = PM.build_model(dict(dict(name='VisionTransformer', **MU.MODEL), tome=dict(r=r)))
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(MU.fixture_state(keys, 2), strict=False)
    return model.train()


def _optimizer(model):
    from passl_amd.solver.optimizer import AdamW
    s = MU.SOLVER
    return AdamW(s['lr'], beta1=s['beta1'], beta2=s['beta2'], epsilon=s['epsilon'], weight_decay=s['weight_decay'],
                 parameters=[p for _, p in model.named_parameters()])


def _run(monkeypatch, r, mode, steps=4):
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.loss.celoss import CELoss
    gen = torch.Generator().manual_seed(3)
    S = MU.MODEL['img_size']
    batches = [(torch.randn(MU.BATCH, 3, S, S, generator=gen).to(DEV),
                torch.randint(0, MU.MODEL['class_num'], (MU.BATCH,), generator=gen).to(DEV)) for _ in range(steps)]
    model = _model(r)
    opt, celoss = _optimizer(model), CELoss()
    calls = {}
    for name in ('tome_match', 'tome_merge_fwd', 'tome_merge_bwd'):
        def counted(*a, _f=getattr(ops, name), _n=name, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, counted)

    def full_step(x, y):
        loss = celoss(model(x), y)['CELoss']
        opt.clear_grad()
        loss.backward(ops.ones_like_cached(loss))
        opt.step()
        return dict(loss=loss)
    sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
    losses = []
    for x, y in batches:
        losses.append(sp.run(x, y)['loss'].detach().clone().reshape(1))
    torch.cuda.synchronize()
    info = None
    if mode == 'plan':
        assert sp.failed is None, sp.failed
        assert not sp.foreign, sp.foreign
        assert sp.captured and sp.replays >= 2
        info = dict(sp.info)
    flat = model.arena_q.flat[:model.arena_q.n_train].clone().cpu()
    return torch.cat(losses).cpu(), flat, info, dict(calls)     # (a later run's wrappers call this run's too)


def test_patched_step_records_with_nothing_foreign_and_replays_bit_identically(monkeypatch):
    le, fe, _, calls = _run(monkeypatch, list(MU.R), 'eager')
    torch.cuda.empty_cache()
    lp, fp, info, plan_calls = _run(monkeypatch, list(MU.R), 'plan')
    _, _, plain, plain_calls = _run(monkeypatch, 0, 'plan')
    print('step plan, r = %s: %s; r = 0: %s' % (MU.R, sorted(info.items()), sorted(plain.items())))
    assert torch.equal(_bits(le), _bits(lp)) and torch.equal(_bits(fe), _bits(fp))
    assert all(math.isfinite(float(v)) for v in lp) and float(lp[0]) != float(lp[-1])
    merging = sum(1 for r in MU.R if r > 0)
    # eager: every step calls the entry points; plan: the warm-up step and the recording step do, the replays do not
    assert calls == {n: 4 * merging for n in ('tome_match', 'tome_merge_fwd', 'tome_merge_bwd')}, calls
    assert plan_calls == {n: 2 * merging for n in ('tome_match', 'tome_merge_fwd', 'tome_merge_bwd')}, plan_calls
    assert plain_calls == {} and info['kernels'] > 100 and info['host_calls'] == 0 and info['node_syncs'] == 0


def test_no_sync_in_a_patched_pass_with_the_trace_off():
    from passl_amd.loss.celoss import CELoss
    model = _model(list(MU.R), torch.bfloat16)
    x, y = MU.batches()[0]
    x, y = x.to(DEV), y.to(DEV)
    celoss = CELoss()
    celoss(model(x), y)['CELoss'].backward()              # first pass: plans, cached index tensors
    torch.cuda.synchronize()
    assert 'trace' not in model._tome_info
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = celoss(model(x), y)['CELoss']
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
