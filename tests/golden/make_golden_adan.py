"""Generate tests/golden/adan_vectors.npz and tests/golden/adan_mae_ft_small.npz by EXECUTING THE REFERENCE's
passl/optimizer/adan.py under the shim (oracle/paddle_shim.py), on the CPU.

    python tests/golden/make_golden_adan.py

Two names adan.py imports and the shim lacks are supplied HERE, at run time (``load_adan``): ``passl.optimizer.Optimizer``
is the class of passl/optimizer/optimizer.py (the package's __init__ is bypassed by the loader), ``paddle.optimizer.adam``
an empty module (imported, never used).

adan_vectors.npz — five tensors of at most 1024 elements, two groups (weight decay 0.02 / 0, lr_scale 1 / 0.5), four
steps under a moving rate, once with the proximal decay and once with no_prox.  Every tensor of 16 elements or more
holds elements whose gradient is zero at every step, elements whose gradient is constant (difference zero after step
1), elements whose gradient flips its sign every step, and random ones; the gradient of ``scaled`` changes its scale by
1e3 between steps.  Stored per run, step and tensor: p and the four state tensors as the reference left them (fp32), and
``ref_err``: the reference's own largest deviation from the float64 rule (tests/adan_util.adan_rule), per buffer.

adan_mae_ft_small.npz — the model, state, inputs and step count of make_golden_mae_finetune_lrd.py with the reference's
Adan in place of its AdamW, one group; a plain run and one with ClipGradByGlobalNorm(clip_norm=1.0) executed from
passl/core/grad_clip.py (make_golden_mae_finetune_clip._shim_for_clip).  Stored per run and step: the loss, pnorm of the
WATCH parameters, p / exp_avg / exp_avg_diff / exp_avg_sq / pre_grad of the ELEMENTWISE ones, the set's norm and
coefficient recomputed in float64 from the unclipped gradients; per run the distance every watched parameter moved.

tests/adan_util.check_golden states what each file must satisfy; it is asserted before either file is written."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import ref_runner, ref_runner_v2       # noqa: E402
import adan_util as U                              # noqa: E402
import make_golden_mae_finetune_lrd as LRD         # noqa: E402
import make_golden_mae_finetune_clip as CLIP       # noqa: E402

STEPS = 4
# the rate is large on purpose: the two decay forms differ by about lr*wd*(lr*upd + lr*wd*p) per step, which must stand
# 100 x above the fp32 bound for the fixture to tell them apart (adan_util.check_golden); at the recipe's 1.5e-2 it does not
LRS = [0.30, 0.27, 0.36, 0.21]
GROUP_WD, GROUP_SCALE = [0.02, 0.0], [1.0, 0.5]
TENSORS = [('a', 1024, 0), ('b', 1000, 1), ('c', 260, 0), ('tiny', 4, 1), ('scaled', 512, 0)]
MODEL = dict(lr=1e-3, weight_decay=0.02)
CLIP_NORM = 1.0
STATE_KEYS = dict(m='exp_avg', d='exp_avg_diff', s='exp_avg_sq', pre='pre_grad')


def load_adan(ns):
    """-> the reference's passl.optimizer.adan module."""
    import paddle
    pkg = sys.modules['passl.optimizer']
    pkg.Optimizer = sys.modules['passl.optimizer.optimizer'].Optimizer     # what passl/optimizer/__init__.py exports
    if 'paddle.optimizer.adam' not in sys.modules:
        adam = types.ModuleType('paddle.optimizer.adam')                   # imported by adan.py, never used
        sys.modules['paddle.optimizer.adam'] = adam
        paddle.optimizer.adam = adam
    return importlib.import_module('passl.optimizer.adan')


def vector_inputs():
    gen = torch.Generator().manual_seed(2208)
    out = {}
    for name, n, _g in TENSORS:
        out['p0/' + name] = (torch.randn(n, generator=gen) * 4.0).numpy()
        base = torch.randn(n, generator=gen)
        for t in range(1, STEPS + 1):
            g = torch.randn(n, generator=gen)
            if n >= 16:
                k = n // 8
                g[:k] = 0.0                                                # zero at every step
                g[k:2 * k] = base[k:2 * k]                                 # constant across the steps
                g[2 * k:3 * k] = base[2 * k:3 * k] * (-1.0) ** t           # flips its sign every step
            if name == 'scaled':
                g = g * (1e-3 if t % 2 else 1.0)
            out['g_s%d/%s' % (t, name)] = g.numpy().copy()
    return out


def run_vectors(adan, out, run, no_prox):
    params = {name: torch.nn.Parameter(torch.from_numpy(out['p0/' + name].copy())) for name, _n, _g in TENSORS}
    groups = [{'params': [params[name] for name, _n, g in TENSORS if g == gi], 'weight_decay': GROUP_WD[gi],
               'lr_scale': GROUP_SCALE[gi]} for gi in range(2)]
    opt = adan.Adan(groups, lr=LRS[0], betas=U.BETAS, eps=U.EPS, no_prox=no_prox)
    f64 = {name: U.zero_state(out['p0/' + name]) for name, _n, _g in TENSORS}
    for t in range(1, STEPS + 1):
        for group in opt.param_groups:
            group['lr'] = LRS[t - 1]
        for name, _n, _g in TENSORS:
            params[name].grad = torch.from_numpy(out['g_s%d/%s' % (t, name)].copy())
        opt.step()
        for name, _n, gi in TENSORS:
            f64[name] = U.adan_rule(f64[name], out['g_s%d/%s' % (t, name)], t, LRS[t - 1] * GROUP_SCALE[gi], GROUP_WD[gi],
                                    U.BETAS, U.EPS, no_prox)
            st = opt.state[params[name]]
            got = dict(p=params[name].detach().numpy().copy(), **{b: st[k].detach().numpy().copy() for b, k in STATE_KEYS.items()})
            errs = []
            for b in U.BUFFERS:
                assert got[b].dtype == np.float32
                out['%s_s%d_%s/%s' % (run, t, b, name)] = got[b]
                errs.append(float(np.max(np.abs(got[b].astype(np.float64) - f64[name][b]))))
            out['%s_s%d_ref_err/%s' % (run, t, name)] = np.array(errs, dtype=np.float64)
    print(run, 'largest ref_err per buffer', [max(float(out['%s_s%d_ref_err/%s' % (run, t, n)][i]) for t in range(1, STEPS + 1)
                                                  for n, _s, _g in TENSORS) for i in range(5)])


def make_vectors(adan):
    out = vector_inputs()
    out['kind'] = np.array('vectors')
    out['names'] = np.array([n for n, _s, _g in TENSORS])
    out['group_of'] = np.array([g for _n, _s, g in TENSORS], dtype=np.int64)
    out['group_wd'] = np.array(GROUP_WD, dtype=np.float64)
    out['group_scale'] = np.array(GROUP_SCALE, dtype=np.float64)
    out['lr'] = np.array(LRS, dtype=np.float64)
    out['betas'] = np.array(U.BETAS, dtype=np.float64)
    out['eps'] = np.float64(U.EPS)
    out['steps'] = np.int64(STEPS)
    out['scaled'] = np.array('scaled')
    out['runs'] = np.array(['prox', 'noprox'])
    out['runs_no_prox'] = np.array([False, True])
    for run, no_prox in (('prox', False), ('noprox', True)):
        run_vectors(adan, out, run, no_prox)
    return out


def run_model(run, ns, adan, gc, out):
    model, keys_shapes = LRD.build(ns)
    named = list(model.named_parameters())
    ps = dict(named)
    kw = dict(lr=MODEL['lr'], betas=U.BETAS, eps=U.EPS, weight_decay=MODEL['weight_decay'])
    if run == 'clip':
        kw['grad_clip'] = gc.ClipGradByGlobalNorm(clip_norm=CLIP_NORM)
    opt = adan.Adan([p for _n, p in named], **kw)
    hw = LRD.ARCH['img_size']
    gen = torch.Generator().manual_seed(909)
    start = {n: ps[n].detach().double().clone() for n in LRD.WATCH}
    for s in range(LRD.STEPS):
        x = torch.randn(LRD.N, 3, hw, hw, generator=gen)
        y = torch.randint(0, LRD.CLASSES, (LRD.N,), generator=gen)
        for p in model.parameters():
            p.grad = None
        res = model(x, y, mode='train')
        res['loss'].backward()
        pre = '%s_s%d_' % (run, s)
        norm = float(np.sqrt(sum(float((p.grad.detach().double() ** 2).sum()) for _n, p in named)))
        coef = 1.0 if run == 'plain' or norm <= CLIP_NORM else CLIP_NORM / (norm + 1e-6)
        out[pre + 'set_norm'] = np.array([norm], dtype=np.float64)
        out[pre + 'set_coef'] = np.array([coef], dtype=np.float64)
        opt.step()
        out[pre + 'loss'] = np.float64(res['loss'].item())
        for n in LRD.WATCH:
            out[pre + 'pnorm/' + n] = np.float64(ps[n].detach().double().norm().item())
        for n in LRD.ELEMENTWISE:
            st = opt.state[ps[n]]
            out[pre + 'p/' + n] = ps[n].detach().numpy().copy()
            for b, k in STATE_KEYS.items():
                out[pre + b + '/' + n] = st[k].detach().numpy().copy()
        print(run, 'step', s, 'loss %.6f' % out[pre + 'loss'], 'norm %.4f coef %.4f' % (norm, coef))
    for n in LRD.WATCH:
        out['%s_move/%s' % (run, n)] = np.float64((ps[n].detach().double() - start[n]).norm().item())
    return keys_shapes


def make_model(ns, adan, gc):
    out = {'kind': np.array('model'), 'runs': np.array(list(U.MODEL_RUNS))}
    for run in U.MODEL_RUNS:
        keys_shapes = run_model(run, ns, adan, gc, out)
    out['meta'] = np.array([LRD.N, LRD.ARCH['img_size'], LRD.STEPS, LRD.CLASSES], dtype=np.int64)
    out['lr'] = np.float64(MODEL['lr'])
    out['weight_decay'] = np.float64(MODEL['weight_decay'])
    out['betas'] = np.array(U.BETAS, dtype=np.float64)
    out['eps'] = np.float64(U.EPS)
    out['clip_norm'] = np.float64(CLIP_NORM)
    out['watch'] = np.array(LRD.WATCH)
    out['elementwise'] = np.array(LRD.ELEMENTWISE)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    return out


if __name__ == '__main__':
    assert ref_runner.available() and ref_runner_v2.available(), 'needs the reference tree'
    ns = ref_runner.load()
    solver = ref_runner_v2.load_solver(ref_runner_v2.load())
    adan = load_adan(solver)
    gc = CLIP._shim_for_clip()
    vec = make_vectors(adan)
    print('vectors:', U.check_golden(vec))
    mod = make_model(ns, adan, gc)
    print('model:', U.check_golden(mod))
    for name, out in (('adan_vectors.npz', vec), ('adan_mae_ft_small.npz', mod)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 1 << 20
