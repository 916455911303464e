"""The CAE pre-training loop — reference tasks/ssl/cae/engine_pretrain.py:41-206 (``train_one_epoch``) with the
optimizer and schedule of tasks/ssl/cae/main_pretrain.py:519-552.  Like MAE's, the task does not go through
``passl.engine.Engine``: its script drives ``model(samples, bool_masked_pos)`` -> two losses -> clipped AdamW.

  * schedule: ``TimmCosine(lr, steps_per_epoch, epochs, decay_unit='step', eta_min=min_lr, warmup_epoch, warmup_prefix=
    True)``, set per ITERATION to the global step before the update (``optimizer.lr_step(it)``, :69-70);
  * loss = CrossEntropy(logits.float(), labels) + dual_loss_weight * mse_loss(latent.float(), latent_target.float())
    (:140-147).  The two device scalars are never added on the device: the backward pass starts from both, the second
    with the root gradient ``dual_loss_weight`` (one resident constant), and the logged sum is formed on the host;
  * optimizer: AdamW, betas (0.9, 0.999), the two groups of :519-541 — 1-D parameters, names ending in '.bias' and the
    skip list undecayed, everything with 'teacher' in its name skipped (the teacher is in no optimizer) — and
    ``ClipGradByGlobalNorm.like_clip_grad_norm_(clip_grad)``, NativeScaler's ``clip_grad_norm_`` over every gradient;
  * batches are ``(images, mask fp32 [B, L], labels int64 [B Nm])`` (datasets.synthetic.SyntheticMaskedTokens): the
    ``--target_mode random`` contract, ``input_ids`` come with the batch and the loader has gathered the labels.

Differences by design: bf16 compute needs no loss scaler; the loss values stay on the device between ``print_freq``
windows (the reference reads three ``.item()`` and synchronises the device every iteration, :161-163, 174) and a
non-finite loss is detected at the window's end; ``mlm_acc`` is not formed.  Refused: ``target_mode`` 'rgb' and
'clusterID' (no tokenizer is built), ``dual_loss_type`` 'kld'."""
import torch

from ...core.grad_clip import ClipGradByGlobalNorm
from ...core.sync_utils import GradReducer, collectives_active, param_sync
from ...hip import ops
from ...modeling.heads.clas_head import _SoftmaxCEFn
from ...models.cae import latent_loss
from ...solver.lr_scheduler import TimmCosine
from ...solver.optimizer import AdamW


def check_args(args):
    if getattr(args, 'target_mode', 'random') != 'random':
        raise NotImplementedError("target_mode %r: only 'random' (token ids come with the batch) is built; 'clusterID' "
                                  "needs the DALL-E tokenizer and 'rgb' the pixel targets" % (args.target_mode,))
    if getattr(args, 'dual_loss_type', 'mse') != 'mse':
        raise NotImplementedError("dual_loss_type %r: only 'mse' is built" % (args.dual_loss_type,))


def param_groups(model, weight_decay):
    """main_pretrain.py:519-541 -> [{no_decay, 0.}, {decay, weight_decay}] over the student's trainable parameters."""
    skip = model.no_weight_decay() if hasattr(model, 'no_weight_decay') else {}
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if 'teacher' in name or not p.requires_grad:
            continue
        (no_decay if (p.dim() == 1 or name.endswith('.bias') or name in skip) else decay).append(p)
    return [{'params': no_decay, 'weight_decay': 0.}, {'params': decay, 'weight_decay': weight_decay}]


def build_optimizer(model, args, steps_per_epoch):
    """-> (AdamW, TimmCosine) as main_pretrain.py:543-552 builds them."""
    check_args(args)
    sched = TimmCosine(float(args.lr), steps_per_epoch, args.epochs, decay_unit='step', eta_min=args.min_lr,
                       warmup_epoch=args.warmup_epochs, warmup_prefix=True)
    clip = getattr(args, 'clip_grad', None)
    opt = AdamW(sched, beta1=0.9, beta2=0.999, parameters=param_groups(model, args.weight_decay),
                grad_clip=ClipGradByGlobalNorm.like_clip_grad_norm_(clip) if clip else None)
    return opt, sched


_weights = {}


def _weight(value, like):
    key = (like.device, float(value))
    w = _weights.get(key)
    if w is None:
        w = _weights[key] = torch.full((1,), float(value), dtype=torch.float32, device=like.device)
    return w


def forward_backward(model, images, mask, labels, num_masked, dual_loss_weight):
    """One forward and backward pass -> (loss_main, mse): device scalars [1]; loss = loss_main + dual_loss_weight * mse."""
    logits, latent_pred, latent_target = model(images, mask, num_masked=num_masked)
    loss_main = _SoftmaxCEFn.apply(logits, labels.contiguous().view(-1))[0]
    mse = latent_loss(latent_pred, latent_target)
    torch.autograd.backward([loss_main, mse], [ops.ones_like_cached(loss_main), _weight(dual_loss_weight, mse)])
    return loss_main, mse


def _data_parallel(model, optimizer):
    if not collectives_active():
        return None
    reducer = getattr(model, '_passl_grad_reducer', None)
    if reducer is None:
        param_sync(model)
        reducer = model._passl_grad_reducer = GradReducer(model.arena, optimizer)
    return reducer


def train_one_epoch(model, data_loader, optimizer, epoch, args, start_steps=None, log=print):
    """args: dual_loss_weight, print_freq, max_train_step (optional), target_mode, dual_loss_type.  ``optimizer`` is
    ``build_optimizer``'s.  -> {'loss', 'loss_main', 'loss_aux': means over the epoch, 'lr': the last rate}."""
    check_args(args)
    model.train()
    print_freq = int(getattr(args, 'print_freq', 10))
    max_train_step = getattr(args, 'max_train_step', None)
    weight = float(args.dual_loss_weight)
    n_iter = len(data_loader)
    start_steps = n_iter * epoch if start_steps is None else start_steps
    num_masked = getattr(data_loader.dataset, 'num_masked', None)
    reducer = _data_parallel(model, optimizer)
    pending, sums, count, lr = [], [0.0, 0.0], 0, None

    def flush():
        nonlocal count
        if pending:
            vals = torch.stack([torch.cat([a.detach().reshape(1), b.detach().reshape(1)]) for a, b in pending]).cpu()
            if not bool(torch.isfinite(vals).all()):
                raise FloatingPointError('Loss is {}, stopping training'.format(vals.tolist()))
            sums[0] += float(vals[:, 0].sum())
            sums[1] += weight * float(vals[:, 1].sum())
            count += len(pending)
            del pending[:]

    for step, (images, mask, labels) in enumerate(data_loader):
        it = start_steps + step
        if max_train_step is not None and it >= max_train_step:
            log('step({}) >= max_train_step({}), training stops early.'.format(it, max_train_step))
            break
        optimizer._learning_rate.step(it)                      # optimizer.lr_step(it): the rate of THIS iteration
        lr = optimizer.get_lr()
        optimizer.clear_grad()
        if reducer is not None:
            reducer.begin()
        pending.append(forward_backward(model, images, mask, labels, num_masked, weight))
        optimizer.step()
        if (step + 1) % print_freq == 0 or step + 1 == n_iter:
            flush()
            n = max(count, 1)
            log('Epoch: [{}]  [{}/{}]  lr: {:.6f}  loss: {:.4f}  loss_main: {:.4f}  loss_aux: {:.4f}'.format(
                epoch, step + 1, n_iter, lr, (sums[0] + sums[1]) / n, sums[0] / n, sums[1] / n))
    flush()
    n = max(count, 1)
    return {'loss': (sums[0] + sums[1]) / n, 'loss_main': sums[0] / n, 'loss_aux': sums[1] / n, 'lr': lr}
