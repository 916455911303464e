"""build_lr_scheduler / build_optimizer — reference passl_v110/solver/builder.py:26-216."""
import copy

from ..utils.registry import Registry, build_from_config

LRSCHEDULERS = Registry('LRSCHEDULER')
OPTIMIZERS = Registry('OPTIMIZER')


def build_lr_scheduler(cfg, iters_per_epoch, batch_size=None, epochs=None):
    """passl_v110/solver/builder.py:26-42.  ``batch_size`` (global) / ``epochs``: only for the SimCLR key set below."""
    if cfg.name == 'CosineWarmup' and 'total_images' in cfg:
        # configs/simclr/simclr_r18_cifar10.yaml:106-113 spells ``name: CosineWarmup`` with the key set of
        # ``simclrCosineWarmup`` (learning_rate_scaling / total_images / warmup_epochs / start_lr / end_lr / T_max in
        # epochs) and carries no ``use_simclr_iters``.  The reference's own CosineWarmup.__init__ takes none of those
        # keys (lr_scheduler.py:78-86: build_from_config raises TypeError there; tests/test_oracle_simclr.py pins that
        # by running the reference's builder on the yaml).  It is resolved the way builder.py:54-66 resolves the
        # r50 recipe's block of the same keys, with the job's real global batch.
        if batch_size is None or epochs is None:
            raise ValueError('lr_scheduler CosineWarmup with total_images needs the global batch size and the epochs')
        cfg = copy.deepcopy(cfg)
        cfg.name = 'simclrCosineWarmup'
        return build_lr_scheduler_simclr(cfg, iters_per_epoch, batch_size, epochs, 0)
    if cfg.name in ('CosineWarmup', 'Cosine'):
        return build_from_config(cfg, LRSCHEDULERS)          # builder.py:39-40: passed through as written
    if cfg.name in ('CosineAnnealingDecay',):
        cfg.T_max *= iters_per_epoch          # yaml T_max is in epochs (builder.py:28-30)
        return build_from_config(cfg, LRSCHEDULERS)
    elif cfg.name == 'MultiStepDecay':
        cfg.milestones = [x * iters_per_epoch for x in cfg.milestones]
        return build_from_config(cfg, LRSCHEDULERS)
    elif cfg.name == 'LinearWarmup':
        cfg.learning_rate = build_lr_scheduler(cfg.learning_rate, iters_per_epoch)
        cfg.warmup_steps *= iters_per_epoch
        return build_from_config(cfg, LRSCHEDULERS)
    raise NotImplementedError(cfg.name)


def build_lr_scheduler_simclr(cfg, iters_per_epoch, batch_size, epochs, current_iter):
    """passl_v110/solver/builder.py:41-66 (``batch_size`` is the trainer's per-GPU batch x 8)."""
    import math
    if cfg.name == 'CosineAnnealingDecay':
        cfg.T_max *= iters_per_epoch
    elif cfg.name == 'MultiStepDecay':
        cfg.milestones = [x * iters_per_epoch for x in cfg.milestones]
    elif cfg.name == 'simclrCosineWarmup':
        cfg.step_each_epoch = iters_per_epoch
        cfg.epochs = epochs
        cfg.warmup_steps = int(round(cfg.warmup_epochs * cfg.total_images // batch_size))
        cfg.total_steps = cfg.total_images * epochs // batch_size + 1
        cfg.T_max = cfg.total_steps - cfg.warmup_steps
        cfg.current_iter = current_iter
        if cfg.learning_rate_scaling == 'linear':
            cfg.lr = cfg.end_lr * batch_size / 256.
        elif cfg.learning_rate_scaling == 'sqrt':
            cfg.lr = cfg.end_lr * math.sqrt(batch_size)
    return build_from_config(cfg, LRSCHEDULERS)


def build_optimizer(cfg, lr_scheduler, model_list=None):
    """passl_v110/solver/builder.py:162-216.  ``layer_decay`` < 1: parameter groups by the v110 rule (solver/lr_decay.py)
    over ``model_list[0]`` with ``num_layers = model_list[0].backbone.get_num_layers()``; ``exclude_from_weight_decay``:
    the Paddle names of the parameters whose state-dict name contains one of the strings get no decay (:203-214)."""
    cfg = copy.deepcopy(cfg)
    name = cfg.pop('name')
    layer_decay = float(cfg.pop('layer_decay')) if 'layer_decay' in cfg else 1.0
    if 'grad_clip' in cfg:
        raise NotImplementedError('grad_clip is not used by configs/moco and is not built')
    if layer_decay < 1.0:
        from .lr_decay import LayerDecayValueAssigner, get_parameter_groups
        num_layers = model_list[0].backbone.get_num_layers()
        assigner = LayerDecayValueAssigner(list(layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)))
        parameters = get_parameter_groups(cfg, model_list[0], get_num_layer=assigner.get_layer_id,
                                          get_layer_scale=assigner.get_scale)
    else:
        parameters = sum([list(m.parameters()) for m in model_list], []) if model_list else None
    if 'Lars' in name or 'Lamb' in name:
        cfg['parameter_list'] = parameters
    else:
        cfg['parameters'] = parameters
        if 'exclude_from_weight_decay' in cfg:
            from .optimizer import paddle_param_names
            ex_decay_cfg = cfg.pop('exclude_from_weight_decay')
            excluded = set()
            for model in model_list:
                pnames = paddle_param_names(model)
                excluded.update(pnames[id(p)] for n, p in model.named_parameters()
                                if any(nd in n for nd in ex_decay_cfg))
            cfg['apply_decay_param_fun'] = lambda pname: pname not in excluded
    return OPTIMIZERS.get(name)(lr_scheduler, **cfg)
