"""Generate tests/golden/cae_small.npz, cae_masks.npz and cae_keys.json by EXECUTING THE REFERENCE's CAE
(passl/models/cae.py: CAEPretrain and everything under it; tasks/ssl/cae/util/masking_generator.py) on torch-CPU through
the paddle shim (oracle/ref_runner_v2.py shows how the v2 tree is imported).

    python tests/golden/make_golden_cae.py          # its own process
    python tests/golden/make_golden_cae.py --check  # run again, compare with the committed files, print the result

The two small models are tests/cae_model_util.py's, with their seed-defined state, inputs and masks; two training steps
each.  Recorded per model ('m1/', 'm2/'), large arrays as their first elements (cae_model_util.clip): the masks; the
first rows of logits, latent_pred and latent_target of step 0; loss_main, loss_aux and loss of both steps; EVERY
parameter gradient of step 0 with its maximum; every student and teacher parameter after the two steps.

The step is engine_pretrain.py:127-171 restated around the reference's model: labels = input_ids[bool_masked_pos],
loss = CrossEntropy(logits.float(), labels) + dual_loss_weight * mse_loss(latent.float(), latent_target.float()), the
gradient clip of NativeScaler (clip_grad_norm_: coef = min(max_norm / (norm + 1e-6), 1) over every gradient together)
and AdamW in the two groups of main_pretrain.py:519-541 (1-D, '.bias' and the skip list undecayed; 'teacher' skipped).

Supplied HERE, in this process only, where oracle/paddle_shim.py lacks them (restated assumptions
[Paddle-semantics]):
  * ``Tensor.transpose(perm)`` with a list = permute; ``paddle.einsum`` = torch's; ``Tensor.scale_(s)`` = mul_(s);
  * ``F.linear(x, weight, bias)`` with weight [in, out]: x @ weight + bias;
  * ``passl.nn.init.trunc_normal_`` / ``xavier_uniform_`` = torch's (initial values only: the state is overwritten);
  * AdamW: the statement of the Paddle ``adamw`` op in oracle/ref_runner_v2.py (``_adamw_op``), beta powers b^t.
"""
import importlib
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import cae_model_util as MU                                               # noqa: E402
from oracle import ref_runner_v2                                          # noqa: E402


def load_reference():
    """-> (the reference's passl.models.cae module, its masking_generator module, the paddle module)."""
    ref_runner_v2.load_solver()
    paddle = sys.modules['paddle']
    shim_transpose = torch.Tensor.transpose

    def transpose(self, *args, perm=None):
        if perm is None and len(args) == 1 and isinstance(args[0], (tuple, list)):
            perm = args[0]
        return self.permute(*perm) if perm is not None else shim_transpose(self, *args)
    torch.Tensor.transpose = transpose
    if not hasattr(paddle, 'einsum'):
        paddle.einsum = torch.einsum
    if not hasattr(torch.Tensor, 'scale_'):
        torch.Tensor.scale_ = lambda self, s: self.mul_(s)
    F = paddle.nn.functional

    def linear(x, weight, bias=None, name=None):
        y = x @ weight
        return y if bias is None else y + bias
    F.linear = linear
    init = sys.modules['passl.nn.init']

    def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
        with torch.no_grad():
            return torch.nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)

    def xavier_uniform_(tensor, *a, **k):
        with torch.no_grad():
            return torch.nn.init.xavier_uniform_(tensor)
    init.trunc_normal_ = trunc_normal_
    init.xavier_uniform_ = xavier_uniform_
    cae = importlib.import_module('passl.models.cae')
    spec = importlib.util.spec_from_file_location(
        'ref_masking_generator', os.path.join(ref_runner_v2.REF_ROOT, 'tasks', 'ssl', 'cae', 'util',
                                              'masking_generator.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return cae, mg, paddle


def norm_layer(paddle):
    from functools import partial
    return partial(paddle.nn.LayerNorm, epsilon=MU.NORM_EPS)


def reference_masks(mg):
    """{name: masks} of the reference's two generators for the seeds the host test replays."""
    out = {}
    random.seed(MU.MASK_SEED)
    g = mg.MaskingGenerator(MU.GRID, MU.NM, min_num_patches=4)
    out['block_6_14'] = np.stack([g() for _ in range(MU.STEPS * MU.BATCH)]).astype(np.int32)
    random.seed(5)
    g = mg.MaskingGenerator((14, 14), 75, max_num_patches=None, min_num_patches=16)       # pretrain.sh
    out['block_14_75'] = np.stack([g() for _ in range(8)]).astype(np.int32)
    np.random.seed(9)
    g = mg.RandomMaskingGenerator(14, 0.4)
    out['random_14_0.4'] = np.stack([g() for _ in range(4)]).astype(np.float64)
    return out


def set_state(model):
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    state = MU.fixture_state(keys_shapes)
    with torch.no_grad():
        for k, v in sd.items():
            if k in state:
                v.copy_(state[k])
    return keys_shapes


def run_model(cae, paddle, name, masks):
    args = MU.args_of(name)
    model = cae.CAEPretrain(norm_layer=norm_layer(paddle), args=args, **MU.MODEL_KW)
    set_state(model)
    model.train()
    named = {k: p for k, p in model.named_parameters()}
    student = {k: p for k, p in named.items() if 'teacher' not in k and p.requires_grad}
    teacher = {k: p for k, p in named.items() if 'teacher' in k and not k.endswith('pos_embed')}
    assert not any(p.requires_grad for p in teacher.values())
    assert 'encoder.pos_embed' not in student, 'the sin-cos table is fixed'
    s = MU.SOLVER
    no_decay, decay = MU.decay_groups([(k, tuple(p.shape)) for k, p in student.items()])
    wd = {k: 0.0 for k in no_decay}
    wd.update({k: s['weight_decay'] for k in decay})
    moments = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in student.items()}
    out = {}
    for step, (imgs, mask, labels) in enumerate(MU.batches(masks)):
        for p in student.values():
            p.grad = None
        logits, latent, latent_target = model(imgs, bool_masked_pos=mask)
        loss_main = torch.nn.functional.cross_entropy(logits.float(), labels)
        loss_aux = s['dual_loss_weight'] * torch.nn.functional.mse_loss(latent.float(), latent_target.detach().float())
        loss = loss_main + loss_aux
        loss.backward()
        for k, v in (('loss_main', loss_main), ('loss_aux', loss_aux), ('loss', loss)):
            out['s%d_%s' % (step, k)] = np.float64(v.item())
        if step == 0:
            out['s0_logits'] = logits.detach().numpy()[:MU.ROWS].copy()
            out['s0_latent_pred'] = latent.detach().numpy()[:, :MU.ROWS].copy()
            out['s0_latent_target'] = latent_target.detach().numpy()[:, :MU.ROWS].copy()
            for k, p in student.items():
                out['s0_grad/' + k] = MU.clip(p.grad.detach().numpy())
                out['s0_gmax/' + k] = np.float64(p.grad.detach().abs().max().item())
        norm = torch.sqrt(sum((p.grad.detach().double() ** 2).sum() for p in student.values())).float()
        coef = torch.clamp(s['clip_grad'] / (norm + 1e-6), max=1.0)
        out['s%d_grad_norm' % step] = np.float64(norm.item())
        assert float(coef) < 1.0, 'the clip must bind'
        for k, p in student.items():
            m, v = moments[k]
            attrs = ('beta1', s['beta1'], 'beta2', s['beta2'], 'epsilon', s['epsilon'], 'with_decay', wd[k] > 0,
                     'coeff', wd[k])
            ref_runner_v2._adamw_op(p, p.grad * coef, s['lr'], m, v, torch.tensor(s['beta1'] ** (step + 1)),
                                    torch.tensor(s['beta2'] ** (step + 1)), None, None, None, None, None, None, None,
                                    *attrs)
        print(name, 'step', step, 'loss %.6f = %.6f + %.6f, |g| %.4f' % (loss.item(), loss_main.item(), loss_aux.item(),
                                                                         norm.item()))
    for k, p in list(student.items()) + list(teacher.items()):
        out['final/' + k] = MU.clip(p.detach().numpy())
    out['no_decay'] = np.array(sorted(no_decay))
    return out


def reference_keys(cae, paddle):
    """{model name: [[key, shape], ...]} of the three factories and the two small models as the reference builds them
    (initialisers switched off: only names and shapes are read)."""
    init = sys.modules['passl.nn.init']
    for fn in ('trunc_normal_', 'constant_', 'xavier_uniform_', 'normal_', 'zeros_', 'ones_'):
        setattr(init, fn, lambda tensor, *a, **k: tensor)
    pretrain = dict(sincos_pos_emb=True, decoder_num_classes=8192, decoder_embed_dim=768, decoder_num_heads=12,
                    regressor_depth=4, num_decoder_self_attention=4, decoder_layer_scale_init_value=0.1, dual_path_ema=0.0)
    from types import SimpleNamespace
    kw = dict(drop_path_rate=0., use_abs_pos_emb=False, init_values=0.1)
    models = {n: (lambda n=n: getattr(cae, n)(args=SimpleNamespace(**pretrain), **kw))
              for n in ('cae_small_patch16_224_8k_vocab', 'cae_base_patch16_224_8k_vocab',
                        'cae_large_patch16_224_8k_vocab')}
    for name in MU.MODELS:
        models['cae_' + name] = lambda name=name: cae.CAEPretrain(norm_layer=norm_layer(paddle), args=MU.args_of(name),
                                                                  **MU.MODEL_KW)
    return {n: [[k, list(v.shape)] for k, v in make().state_dict().items()] for n, make in models.items()}


def main(argv):
    assert ref_runner_v2.available(), 'needs the reference tree'
    cae, mg, paddle = load_reference()
    check = '--check' in argv
    masks = reference_masks(mg)
    ours = MU.block_masks(MU.STEPS * MU.BATCH)
    assert np.array_equal(ours, masks['block_6_14'].reshape(len(ours), -1)), 'the product generator draws other masks'
    small = {}
    for name in MU.MODELS:
        small.update({'%s/%s' % (name, k): v for k, v in run_model(cae, paddle, name, ours).items()})
    small['masks'] = ours
    keys = reference_keys(cae, paddle)
    bad = []
    for fname, out in (('cae_small', small), ('cae_masks', masks)):
        if check:
            have = MU.load(fname)
            bad += ['%s: %s' % (fname, k) for k in sorted(set(out) | set(have))
                    if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
        else:
            path = os.path.join(HERE, fname + '.npz')
            np.savez_compressed(path, **out)
            print('wrote', path, os.path.getsize(path), 'bytes')
    kpath = os.path.join(HERE, 'cae_keys.json')
    if check:
        bad += ['cae_keys.json'] if json.load(open(kpath)) != keys else []
        print('DIFFERENT: %s' % bad if bad else 'fixtures equal the live reference run')
        sys.exit(1 if bad else 0)
    with open(kpath, 'w') as f:                          # one [key, shape] entry per line
        f.write('{\n' + ',\n'.join('%s: [\n%s\n]' % (json.dumps(n), ',\n'.join(json.dumps(e) for e in keys[n]))
                                   for n in sorted(keys)) + '\n}\n')
    print('wrote', kpath, os.path.getsize(kpath), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1:])
