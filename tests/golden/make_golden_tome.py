"""Generate tests/golden/tome_small.npz and tome_layers.npz by EXECUTING THE REFERENCE's token merging
(passl/models/utils/tome.py: bipartite_soft_matching, merge_wavg, ToMeBlock, ToMeAttention, parse_r, apply_patch) on the
reference's VisionTransformer (passl/models/vision_transformer.py) and CELoss, on torch-CPU in float64 through the
paddle shim (oracle/ref_runner_v2.py shows how the v2 tree is imported; make_golden_cait.load_reference supplies what
the ViT itself needs and is reused as it is).

    python tests/golden/make_golden_tome.py          # its own process
    python tests/golden/make_golden_tome.py --check  # run again and compare with the committed files, exactly

Supplied HERE, in this process only, because oracle/paddle_shim.py lacks them (restated assumptions [Paddle-semantics]):
  * ``Tensor.take_along_axis(axis, indices)`` = torch.take_along_dim;
  * ``Tensor.put_along_axis_(axis, indices, values, reduce='add')`` = scatter_add_ in place (without ``reduce``: scatter_);
  * indexing with a stepped slice (``x[..., 1::2, :]``) returns a COPY, as Paddle's strided_slice does, where torch
    returns a view: the reference writes into such a slice in place, which torch's autograd refuses on a view whose
    base it still needs;
  * ``Tensor.argsort(axis, descending)`` = torch.argsort (the fixture's maxima are distinct: stability is not used);
  * ``Tensor.sort(axis)`` and ``Tensor.max(axis)`` return the values only;
  * ``paddle.ones_like`` = torch.ones_like.
``max``, ``argmax`` and ``argsort`` also RECORD what they return while a recorder is installed: that is how the
per-layer scores and decisions get into the fixture without touching the reference's code.
``global_pool = False`` is set on the instance: the patched forward_features reads it and the plain ViT lacks it.

The model, state, inputs and solver are tests/tome_model_util.py's.  Seed rule (bf16 decisions): for state seed 0, 1, ...
each of the three recorded passes (the prop_attn evaluation and the forward of either training step, the second with
the parameters the reference's first AdamW step left) is run twice in float64, as it is and with the output of every
qkv Linear rounded to bf16; `change` = the largest difference of any score of a non-class row between the two, `gap` =
the smallest float64 gap a decision depends on (per merging layer and image: node_max of rank r - 1 minus rank r, and
top-1 minus top-2 of every merged row).  The first seed with gap >= 4 change over all three passes is taken; seed, gap
and change are stored.

tome_small.npz: seed, gap, change; r after the clamp and T per layer; per merging layer of both training steps (prop_attn False)
and of the prop_attn=True evaluation: scores, node_max, node_idx, unm_idx (sorted), src_idx, dst_idx; logits of both;
for prop_attn False two training steps: losses, every parameter gradient of step 0 and every parameter after two AdamW
steps (no-decay names of tome_model_util; large tensors sampled, tome_model_util.sample), recorded as float32.
tome_layers.npz: for tome_model_util.LAYER_CASES qkv, x, size -> the index tensors, merged x and new size."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import tome_model_util as MU                                              # noqa: E402
import make_golden_cait as MC                                             # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402

RECORD = []          # [(kind, tensor)] while recording


def install_tensor_methods():
    paddle = sys.modules['paddle']
    if not hasattr(paddle, 'ones_like'):
        paddle.ones_like = torch.ones_like
    T = torch.Tensor
    t_max, t_argmax, t_sort = T.max, T.argmax, T.sort

    def take_along_axis(self, axis, indices):
        return torch.take_along_dim(self, indices, dim=axis)

    def put_along_axis_(self, axis, indices, values, reduce=None):
        if reduce == 'add':
            return self.scatter_add_(axis, indices, values)
        assert reduce is None
        return self.scatter_(axis, indices, values)

    def argsort(self, axis=-1, descending=False):
        out = torch.argsort(self, dim=axis, descending=descending)
        RECORD.append(('argsort', out.detach().clone()))
        return out

    def sort(self, *args, axis=None, **kw):
        return t_sort(self, dim=axis).values if axis is not None else t_sort(self, *args, **kw)

    def tmax(self, *args, axis=None, **kw):
        if axis is None:
            return t_max(self, *args, **kw)
        RECORD.append(('scores', self.detach().clone()))
        out = t_max(self, dim=axis).values
        RECORD.append(('max', out.detach().clone()))
        return out

    def argmax(self, *args, axis=None, **kw):
        out = t_argmax(self, *args, **kw) if axis is None else torch.argmax(self, dim=axis)
        if axis is not None:
            RECORD.append(('argmax', out.detach().clone()))
        return out
    T.take_along_axis, T.put_along_axis_, T.argsort, T.sort, T.max, T.argmax = \
        take_along_axis, put_along_axis_, argsort, sort, tmax, argmax
    t_getitem = T.__getitem__

    def getitem(self, idx):
        out = t_getitem(self, idx)
        items = idx if isinstance(idx, tuple) else (idx,)
        if any(isinstance(i, slice) and i.step not in (None, 1) for i in items):
            out = out.clone()
        return out
    T.__getitem__ = getitem


def layers_of_record(rs):
    """RECORD of one forward -> per merging layer a dict of numpy arrays (the reference's own tensors)."""
    kinds = [k for k, _ in RECORD]
    n = sum(1 for r in rs if r > 0)
    assert kinds == ['scores', 'max', 'argmax', 'argsort'] * n, kinds
    out, it = [], iter(RECORD)
    for r in rs:
        if r <= 0:
            continue
        scores, nmax, nidx, edge = [next(it)[1] for _ in range(4)]
        src = edge[:, :r]
        out.append({'scores': scores.numpy().copy(), 'node_max': nmax.numpy().copy(), 'node_idx': nidx.numpy().copy(),
                    'unm_idx': edge[:, r:].sort(dim=1).values.numpy().copy(), 'src_idx': src.numpy().copy(),
                    'dst_idx': torch.gather(nidx, 1, src).numpy().copy(), 'r': r})
    return out


def smallest_gap(layers):
    g = np.inf
    for L in layers:
        r, nm, sc = L['r'], L['node_max'], L['scores']
        srt = -np.sort(-nm, axis=-1)
        g = min(g, float((srt[:, r - 1] - srt[:, r]).min()))
        if sc.shape[-1] > 1:
            top2 = np.sort(sc, axis=-1)[:, :, -2:]
            for b in range(sc.shape[0]):
                for i in L['src_idx'][b]:
                    g = min(g, float(top2[b, i, 1] - top2[b, i, 0]))
    return g


def build(ns, tome, seed, prop_attn):
    model = ns.vit.VisionTransformer(**MU.MODEL)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    state = MU.fixture_state(keys, seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(state[k])
    model.double()
    tome.apply_patch(model, prop_attn=prop_attn)
    model.global_pool = False
    model.r = list(MU.R)
    return model, keys


def schedule(tome, T):
    rs, t_in = [], []
    for r in tome.parse_r(MU.MODEL['depth'], list(MU.R)):
        t_in.append(T)
        r = min(r, (T - 1) // 2)
        rs.append(r)
        T -= r
    return rs, t_in, T


def forward_recorded(model, x, rs):
    del RECORD[:]
    out = model(x.double())
    layers = layers_of_record(rs)
    del RECORD[:]
    return out, layers


def forward_both(model, x, rs):
    """One forward as it is (its output and layers are returned) and one, without gradient, with the output of every qkv
    Linear rounded to bf16 -> (output, layers, gap, change) of the module docstring's seed rule."""
    out, exact = forward_recorded(model, x, rs)
    with torch.no_grad():
        hooks = [blk.attn.qkv.register_forward_hook(lambda m, i, o: o.float().bfloat16().double())
                 for blk in model.blocks]
        _, rounded = forward_recorded(model, x, rs)
        for h in hooks:
            h.remove()
    change = max(float(np.abs(a['scores'][:, 1:] - b['scores'][:, 1:]).max()) for a, b in zip(exact, rounded))
    return out, exact, smallest_gap(exact), change


def put_layers(out, prefix, layers):
    for i, L in enumerate(layers):
        for k, v in L.items():
            out['%s/layer%d/%s' % (prefix, i, k)] = np.asarray(v)


def run_seed(ns, tome, seed, rs):
    """Everything the fixture records for one state seed, and (gap, change) over its three recorded passes."""
    batches = MU.batches()
    out, gaps, changes = {}, [], []
    # prop_attn=True, evaluation
    model, keys = build(ns, tome, seed, True)
    model.eval()
    with torch.no_grad():
        logits, layers, g, c = forward_both(model, batches[0][0], rs)
    gaps.append(g)
    changes.append(c)
    out['prop/logits'] = logits.numpy().copy()
    put_layers(out, 'prop', layers)
    # prop_attn=False, two training steps
    model, keys = build(ns, tome, seed, False)
    model.train()
    params = dict(model.named_parameters())
    celoss = ns.loss.celoss.CELoss()
    s = MU.SOLVER
    skip = {n for n in params if any(nd in n for nd in MU.NO_DECAY)}
    moments = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in params.items()}
    for step, (x, y) in enumerate(batches):
        for p in params.values():
            p.grad = None
        logits, layers, g, c = forward_both(model, x, rs)
        gaps.append(g)
        changes.append(c)
        loss = celoss(logits, y)['CELoss']
        loss.backward()
        out['s%d_loss' % step] = np.float64(loss.item())
        put_layers(out, 's%d' % step, layers)
        if step == 0:
            out['s0_logits'] = logits.detach().numpy().copy()
            for k, p in params.items():
                out['s0_grad/' + k] = MU.sample(p.grad).float().numpy().copy()
        for k, p in params.items():
            m, v = moments[k]
            attrs = ('beta1', s['beta1'], 'beta2', s['beta2'], 'epsilon', s['epsilon'], 'with_decay', True,
                     'coeff', 0.0 if k in skip else s['weight_decay'])
            ref_runner_v2._adamw_op(p, p.grad, s['lr'], m, v, torch.tensor(s['beta1'] ** (step + 1)),
                                    torch.tensor(s['beta2'] ** (step + 1)), None, None, None, None, None, None, None,
                                    *attrs)
    for k, p in params.items():
        out['final/' + k] = MU.sample(p).float().numpy().copy()
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys])
    return out, min(gaps), max(changes)


def record_model(ns, tome):
    rs, t_in, t_final = schedule(tome, MU.TOKENS)
    assert rs == MU.R and t_final == MU.TOKENS - sum(MU.R)
    for seed in range(200):
        out, gap, change = run_seed(ns, tome, seed, rs)
        print('seed %d: gap %.3e, change under bf16 qkv %.3e, ratio %.2f' % (seed, gap, change, gap / change))
        if gap >= 4 * change:
            break
    else:
        raise AssertionError('no seed below 200 satisfies gap >= 4 change')
    print('losses', float(out['s0_loss']), float(out['s1_loss']))
    out.update({'seed': np.int64(seed), 'gap': np.float64(gap), 'change': np.float64(change),
                'r': np.asarray(rs, dtype=np.int64), 't_in': np.asarray(t_in, dtype=np.int64),
                't_final': np.int64(t_final)})
    return out


def record_layers(tome):
    out = {}
    gen = torch.Generator().manual_seed(1203)
    for n, (B, T, H, DH, C, r, prev) in enumerate(MU.LAYER_CASES):
        qkv = torch.randn(B, T, 3, H, DH, generator=gen).double()
        x = torch.randn(B, T, C, generator=gen).double()
        size = None
        if prev:                                        # the sizes the reference's own merge of T + 5 ones leaves
            pm, _ = tome.bipartite_soft_matching(torch.randn(B, T + 5, DH, generator=gen).double(), 5, True, False)
            _, size = tome.merge_wavg(pm, torch.zeros(B, T + 5, 1, dtype=torch.float64), None)
        del RECORD[:]
        metric = qkv[:, :, 1].permute(0, 2, 1, 3).mean(1)                  # k.mean(1) of ToMeAttention.forward
        merge, _ = tome.bipartite_soft_matching(metric, r, True, False)
        (L,) = layers_of_record([r])
        del RECORD[:]
        y, new_size = tome.merge_wavg(merge, x.clone(), None if size is None else size.clone())
        pre = 'case%d/' % n
        out[pre + 'qkv'], out[pre + 'x'] = qkv.numpy().copy(), x.numpy().copy()
        if size is not None:
            out[pre + 'size'] = size.numpy().copy()
        for k in ('node_max', 'node_idx', 'unm_idx', 'src_idx', 'dst_idx'):
            out[pre + k] = L[k]
        out[pre + 'y'], out[pre + 'new_size'] = y.numpy().copy(), new_size.numpy().copy()
    # parse_r as the reference computes it
    for tag, arg in (('int16', 16), ('dec16', (16, -1)), ('inc16', (16, 1)), ('half13', (13, -0.5)), ('list', [4, 3])):
        out['parse_r/' + tag] = np.asarray(tome.parse_r(12 if tag != 'list' else 3, arg), dtype=np.int64)
    return out


def main(argv):
    assert ref_runner_v2.available(), 'needs the reference tree'
    ns, _paddle = MC.load_reference()
    install_tensor_methods()
    ns.vit = sys.modules['passl.models.vision_transformer']
    tome = importlib.import_module('passl.models.utils.tome')
    check = '--check' in argv
    bad = []
    for name, out in ((MU.FIXTURE, record_model(ns, tome)), (MU.LAYERS, record_layers(tome))):
        path = os.path.join(HERE, name + '.npz')
        if check:
            have = MU.load(name)
            bad += ['%s: %s' % (name, k) for k in sorted(set(out) | set(have))
                    if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
        else:
            np.savez_compressed(path, **out)
            print('wrote', path, os.path.getsize(path), 'bytes')
    if check:
        print('DIFFERENT: %s' % bad if bad else 'fixtures equal the live reference run')
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main(sys.argv[1:])
