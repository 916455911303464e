"""Generate tests/golden/deit_small.npz, deit_long.npz and deit_layers.npz by EXECUTING THE REFERENCE's DeiT
(passl/models/deit.py: DeitVisionTransformer, DistilledVisionTransformer and the eight factories; Block / Attention /
Mlp / PatchEmbed / DropPath of passl/models/vision_transformer.py; passl/loss CELoss) on torch-CPU through the paddle
shim.  make_golden_cait.load_reference imports the v2 tree and supplies most of what the shim lacks; it is reused as it
is.

    python tests/golden/make_golden_deit.py          # its own process
    python tests/golden/make_golden_deit.py --check  # run again and compare with the committed files, exactly

The models are tests/deit_model_util.py's.  Recorded per case (key prefix '<case>/'): logits, loss and EVERY parameter
gradient of step 0, the loss of step 1, the parameters of at most ``FINAL_MAX`` elements after the two AdamW steps
(decay 0 for the names of the config's ``no_weight_decay_name``; no clipping, the recipe has none), with a rate the keep
table of each step in the product's layout (deit_model_util.keep_table, from the recorded draws of ``paddle.rand``), the
state_dict key list, the no-decay name list.
  deit_small   the 10-token model with drop_path_rate 0 ('dp0') and 0.5 ('dp5');
  deit_long    the 226-token plain model ('plain') and the 227-token distilled class ('dist'), rate 0;
  deit_layers  the state_dict keys and shapes of the eight factories, and a ``load_pretrained(finetune=True)`` of a
               3 x 3 position grid into a 5 x 5 model, plain and distilled: the source table, the loaded table, and
               whether the head (of another size) was kept.

Supplied HERE, in this process only, on top of make_golden_cait's pieces (restated assumptions [Paddle-semantics]):
  * ``paddle.shape(x)`` = x.shape;  ``paddle.transpose(x, perm)`` = permute;
  * ``zeros_``: deit.py:223, :227 name it without importing it (``passl.nn.init.zeros_`` is meant); initial values only,
    the state is overwritten;
  * ``Layer.add_parameter(name, p)`` = torch's register_parameter;
  * ``paddle.load(path)`` of a ``.pdparams`` file = the pickled dict of numpy arrays as tensors; ``Layer.set_dict`` =
    load_state_dict without strictness over the entries whose shape matches (Paddle warns about a tensor of another
    shape and skips it: the ``head_dist`` of another class count, which deit.py:156-160 does not remove);  ``os.path.exists`` is the real one: the file is
    written to a temporary directory;
  * ``nn.functional.interpolate(mode='bicubic', align_corners=False)`` = torch's (A = -0.75 in both)."""
import importlib
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import deit_model_util as MU                                              # noqa: E402
import make_golden_cait as GC                                             # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402


def load_reference():
    ns, paddle = GC.load_reference()
    nn = paddle.nn
    if not hasattr(paddle, 'shape'):
        paddle.shape = lambda x: x.shape
    if not hasattr(paddle, 'transpose'):
        paddle.transpose = lambda x, perm: x.permute(*perm)
    if not hasattr(nn.Layer, 'add_parameter'):
        nn.Layer.add_parameter = lambda self, name, p: self.register_parameter(name, p)
    if not hasattr(nn.Layer, 'set_dict'):
        def set_dict(self, sd):
            own = self.state_dict()
            return self.load_state_dict({k: v for k, v in sd.items() if k not in own or v.shape == own[k].shape},
                                        strict=False)
        nn.Layer.set_dict = set_dict

    def load(path):
        with open(path, 'rb') as f:
            return {k: torch.as_tensor(np.asarray(v)) for k, v in pickle.load(f).items()}
    paddle.load = load
    try:
        nn.functional.interpolate(torch.zeros(1, 1, 2, 2), size=(3, 3), mode='bicubic', align_corners=False)
    except Exception:
        nn.functional.interpolate = torch.nn.functional.interpolate
    ns.deit = importlib.import_module('passl.models.deit')
    ns.deit.zeros_ = sys.modules['passl.nn.init'].zeros_
    return ns, paddle


def set_state(layer, seed=2012):
    state = MU.fixture_state([(k, tuple(v.shape)) for k, v in layer.state_dict().items()], seed)
    with torch.no_grad():
        for k, v in layer.state_dict().items():
            v.copy_(state[k])
    return state


def no_decay_names(params):
    return [n for n in params if any(nd in n for nd in MU.NO_DECAY)]


def run_case(ns, paddle, tag, cls_name, args, rate):
    model = getattr(ns.deit, cls_name)(drop_path_rate=rate, **args)
    keys_shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    state = set_state(model)
    params = dict(model.named_parameters())
    assert sorted(state) == sorted(params), 'every parameter, and nothing else, has a seed-defined value'
    model.train()
    celoss = ns.loss.celoss.CELoss()
    draws, rand0 = [], paddle.rand

    def rand(shape, *a, **k):
        u = rand0(shape, *a, **k)
        draws.append(u.detach().clone().reshape(-1).numpy())
        return u
    paddle.rand = rand
    torch.manual_seed(5)                                  # the draws of paddle.rand
    moments = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in params.items()}
    s = MU.SOLVER
    skip = set(no_decay_names(params))
    out = {}
    try:
        for step, (x, y) in enumerate(MU.batches(args)):
            for p in params.values():
                p.grad = None
            del draws[:]
            logits = model(x)
            loss = celoss(logits, y)['CELoss']
            loss.backward()
            if rate > 0.:
                keep = MU.keep_table(draws, rate, args['depth'])
                assert np.all((keep == 0) | (keep == 1))
                out['s%d_keep' % step] = keep
                print(tag, 'step', step, 'keep', keep.tolist())
            else:
                assert not draws
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
            print(tag, 'step', step, 'loss %.6f' % loss.item())
    finally:
        paddle.rand = rand0
    for k, p in params.items():
        if p.numel() <= MU.FINAL_MAX:
            out['final/' + k] = p.detach().numpy().copy()
    if rate > 0.:
        k0 = out['s0_keep']
        assert (k0 == 0).any() and (k0 == 1).any(), 'step 0 must both drop and keep'
    out['rate'] = np.float64(rate)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    out['no_decay'] = np.array(no_decay_names(params))
    return {tag + '/' + k: v for k, v in out.items()}


def record_layers(ns):
    out = {}
    rows = []
    for f in MU.FACTORIES:
        for k, v in getattr(ns.deit, f)().state_dict().items():
            rows.append('%s|%s:%s' % (f, k, 'x'.join(map(str, v.shape))))
    # one byte string: an array of Python strings is stored at four bytes a character
    out['factory_keys'] = np.frombuffer('\n'.join(rows).encode(), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        for tag, cls_name in (('plain', 'DeitVisionTransformer'), ('dist', 'DistilledVisionTransformer')):
            src = getattr(ns.deit, cls_name)(**MU.POS_FROM)
            set_state(src, seed=11)
            path = os.path.join(tmp, tag)
            with open(path + '.pdparams', 'wb') as f:
                pickle.dump({k: v.detach().numpy() for k, v in src.state_dict().items()}, f, protocol=2)
            dst = getattr(ns.deit, cls_name)(**MU.POS_TO)
            set_state(dst, seed=12)
            head = dst.head.weight.detach().clone()
            dst.load_pretrained(path, finetune=True)
            out['pos/%s/from' % tag] = src.pos_embed.detach().numpy().copy()
            out['pos/%s/to' % tag] = dst.pos_embed.detach().numpy().copy()
            out['pos/%s/head_kept' % tag] = np.bool_(torch.equal(dst.head.weight.detach(), head))
            out['pos/%s/qkv_loaded' % tag] = np.bool_(torch.equal(dst.blocks[1].attn.qkv.weight.detach(),
                                                                  src.blocks[1].attn.qkv.weight.detach()))
            out['pos/%s/cls_loaded' % tag] = np.bool_(torch.equal(dst.cls_token.detach(), src.cls_token.detach()))
    return out


def main(argv):
    assert ref_runner_v2.available(), 'needs the reference tree'
    ns, paddle = load_reference()
    check = '--check' in argv
    bad = []
    for name in list(MU.CASES) + [MU.LAYERS]:
        if name == MU.LAYERS:
            out = record_layers(ns)
        else:
            out = {}
            for tag, (cls_name, args, rate) in MU.CASES[name].items():
                out.update(run_case(ns, paddle, tag, cls_name, args, rate))
        if check:
            have = MU.load(name)
            bad += ['%s: %s' % (name, k) for k in sorted(set(out) | set(have))
                    if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
        else:
            path = os.path.join(HERE, name + '.npz')
            np.savez_compressed(path, **out)
            print('wrote', path, os.path.getsize(path), 'bytes')
    if check:
        print('DIFFERENT: %s' % bad if bad else 'fixtures equal the live reference run')
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main(sys.argv[1:])
