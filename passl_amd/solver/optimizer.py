"""Momentum-SGD over the flat parameter arena (one HIP launch per step).

Registered under the reference's name ``Momentum`` (passl_v110/solver/optimizer.py:24 registers
paddle.optimizer.Momentum) with Paddle's constructor spelling
``Momentum(learning_rate, momentum=0.9, parameters=None, weight_decay=None, ...)``.  A float
``weight_decay`` is L2 decay folded into the gradient of EVERY parameter (configs/moco has no
exclusion list): g += wd*p; v = mu*v + g; p -= lr*v  — the rule restated in-tree at
passl/optimizer/momentum.py:150-158.
"""
import torch

from ..hip import ops, streams
from ..core.grad_clip import ClipGradByGlobalNorm
from .builder import OPTIMIZERS
from .lr_scheduler import LRScheduler


def _load_flat_state(dst, sd, key):
    """Copy one flat optimizer-state vector from a checkpoint dict.  Values may be torch tensors or the
    numpy arrays the checkpoint pickle stores (hooks/checkpoint_hook.py); the arena layout is this
    code base's own (one vector per EncoderArena), so a size mismatch — e.g. a Paddle optimizer
    state with per-parameter accumulators — is reported instead of broadcasting garbage."""
    if key not in sd:
        raise KeyError('optimizer state has no %r (flat-arena layout expected; Paddle per-parameter '
                       'accumulator files are not interchangeable)' % key)
    src = torch.as_tensor(sd[key])
    if src.numel() != dst.numel():
        raise ValueError('optimizer state %r has %d elements, the arena holds %d'
                         % (key, src.numel(), dst.numel()))
    dst.copy_(src.reshape(dst.shape).to(dst.dtype))


def _grads_complete(arena):
    """Everything that writes this arena's gradients is ordered before the update kernel: outstanding gradient
    collectives (GradReducer.finish) and work on the side stream — weight gradients, the backward of a forked
    downsample branch (hip/streams.py)."""
    if arena.reducer is not None:
        arena.reducer.finish()
    if arena.grads is not None and arena.grads.is_cuda:
        streams.join(arena.grads.device)


class _DeviceHyper(object):
    """Step-dependent scalars of an optimizer — {lr, beta1^t, beta2^t, unused} — held in DEVICE memory and read by
    the update kernel when it runs (ops.*_dev): nothing about the schedule is frozen into a kernel launch, so the
    whole training step can be captured once in a HIP graph and replayed (hip/graph.py) while the reference's
    per-iteration schedule (passl_v110/hooks/lr_scheduler_hook.py:26-28) moves on.

    ``push_hyper()`` = one host-side update of the step state (``_host_values``) + one asynchronous H2D copy from a
    ring of pinned slots (the host may run several steps ahead of the GPU: a slot is re-used only after the copy
    that read it has completed).  ``step()`` calls it itself unless the caller already did (graph replay: the copy
    is stream-ordered in front of the graph launch, never part of the graph).

    ``_HYPER_WIDTH``: the floats of the block (4; Adan's is 8 — a third beta power and its first-step flag).
    ``_host_values`` returns the leading ones, the rest stays zero."""

    _RING = 16
    _HYPER_WIDTH = 4

    def _init_hyper(self, device):
        self._hyper_dev = torch.zeros(self._HYPER_WIDTH, dtype=torch.float32, device=device)
        self._hyper_host = None
        self._hyper_ev = [None] * self._RING
        self._hyper_slot = 0
        self._hyper_pushed = False

    def _host_values(self):
        """-> (lr, beta1^t, beta2^t); advances host-side step state (AdamW's t)."""
        return self.get_lr(), 0.0, 0.0

    def push_hyper(self):
        dev = self._hyper_dev
        vals = self._host_values()
        if dev.is_cuda:
            if self._hyper_host is None:
                self._hyper_host = torch.zeros(self._RING, self._HYPER_WIDTH, dtype=torch.float32).pin_memory()
            i = self._hyper_slot
            if self._hyper_ev[i] is not None:
                self._hyper_ev[i].synchronize()          # the copy that read this slot RING steps ago is done
            h = self._hyper_host[i]
            for k, x in enumerate(vals):
                h[k] = x
            dev.copy_(h, non_blocking=True)
            ev = self._hyper_ev[i] or torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev.device))
            self._hyper_ev[i] = ev
            self._hyper_slot = (i + 1) % self._RING
        else:
            for k, x in enumerate(vals):
                dev[k] = x
        self._hyper_pushed = True

    def set_lr(self, value):
        """paddle.optimizer.Optimizer.set_lr: a fixed rate from now on (refused while a scheduler drives the rate, as
        Paddle does)."""
        if isinstance(self._learning_rate, LRScheduler):
            raise RuntimeError("optimizer's learning rate can't be LRScheduler when invoke this API, because this "
                               'will lead to conflict.')
        self._learning_rate = float(value)

    def _hyper_for_step(self):
        if not self._hyper_pushed:
            self.push_hyper()
        self._hyper_pushed = False
        return self._hyper_dev


class _ArenaOptimizer(_DeviceHyper):
    """An optimizer over flat arenas: every listed trainable parameter lives in an EncoderArena, every parameter of
    such an arena is listed exactly once, and the state is a few flat vectors per arena (``_STATE``), saved and
    loaded under the keys ``<name>_<arena index>``.  A subclass adds its rule (``step``) and its configuration."""

    _STATE = ()        # ((state_dict key prefix, attribute: one flat vector per arena), ...)

    def _init_arenas(self, parameters):
        params = [p for p in (parameters or []) if p.requires_grad]
        arenas, seen = [], set()
        for p in params:
            a = getattr(p, '_passl_arena', None)
            if a is None:
                raise NotImplementedError('%s optimises parameters that live in an EncoderArena (flat buffer); '
                                          'got a free tensor' % type(self).__name__)
            if id(p) in seen:
                raise ValueError('a parameter appears more than once in the parameter list / groups')
            seen.add(id(p))
            if a not in arenas:
                arenas.append(a)
        for a in arenas:
            if sum(1 for p in params if p._passl_arena is a) != len(a.param_slices):
                raise NotImplementedError('optimising a subset of an arena is not supported')
        self._parameter_list = params
        self._arenas = arenas
        for _key, attr in self._STATE:
            setattr(self, attr, [torch.zeros_like(a.flat[:a.n_train]) for a in arenas])
        self.grad_scale = 1.0      # set by the DP reducer to 1/world_size (sum -> mean)
        self._init_hyper(arenas[0].device if arenas else torch.device('cpu'))

    # ---- paddle.optimizer API used by the hooks
    def get_lr(self):
        lr = self._learning_rate
        return float(lr()) if isinstance(lr, LRScheduler) else float(lr)

    def clear_grad(self, set_to_zero=True):
        for a in self._arenas:
            a.clear_grad()

    clear_gradients = clear_grad

    def state_dict(self):
        sd = {'%s_%d' % (key, i): x.detach().cpu()
              for key, attr in self._STATE for i, x in enumerate(getattr(self, attr))}
        if isinstance(self._learning_rate, LRScheduler):
            sd['LR_Scheduler'] = self._learning_rate.state_dict()
        return sd

    def set_state_dict(self, sd):
        for key, attr in self._STATE:
            for i, x in enumerate(getattr(self, attr)):
                _load_flat_state(x, sd, '%s_%d' % (key, i))
        if 'LR_Scheduler' in sd and isinstance(self._learning_rate, LRScheduler):
            self._learning_rate.set_state_dict(sd['LR_Scheduler'])


@OPTIMIZERS.register()
class Momentum(_ArenaOptimizer):
    type = 'momentum'
    _STATE = (('velocity', '_velocity'),)

    def __init__(self, learning_rate=0.001, momentum=0.9, parameters=None, use_nesterov=False,
                 weight_decay=None, grad_clip=None, multi_precision=False, rescale_grad=1.0,
                 name=None, use_master_param=None, lr_func=None):
        # v2 spelling (passl/optimizer/momentum.py:25-45): use_master_param asks for fp32 masters next to fp16
        # parameters — the arena's parameters ARE fp32 masters; lr_func (LRCallable groups) is not used by the recipes
        if use_nesterov:
            raise NotImplementedError('nesterov momentum is not used on the MoCo path')
        if grad_clip is not None or lr_func is not None:
            raise NotImplementedError('grad_clip / lr_func are not used on the MoCo path')
        self._learning_rate = learning_rate
        self._momentum = float(momentum)
        self._wd = float(weight_decay) if weight_decay else 0.0
        self._rescale = float(rescale_grad)
        self._init_arenas(parameters)

    @torch.no_grad()
    def step(self):
        hyper = self._hyper_for_step()
        for a, v in zip(self._arenas, self._velocity):
            _grads_complete(a)
            ops.momentum_sgd_dev(a.flat[:a.n_train], a.grads, v, hyper, self._momentum, self._wd,
                                 self.grad_scale * self._rescale)


def _paddle_auto_names(arena):
    """Dygraph auto-generated parameter names ('conv2d_3.w_0', 'batch_norm2d_1.b_0', 'linear_0.w_0')
    in construction order — what LarsMomentumOptimizer matches ``exclude_from_weight_decay``
    against (param.name, not the state_dict key)  [Paddle-semantics]."""
    from ..hip import nn as hnn
    counters, names, seen = {}, [], set()
    for mod in arena.module.modules():
        # the arena's own slots only, each once (EncoderArena skips excluded sub-layers and shared parameters)
        own = [n for n, p in mod._parameters.items()
               if p is not None and getattr(p, '_passl_arena', None) is arena and id(p) not in seen]
        seen.update(id(mod._parameters[n]) for n in own)
        if not own:
            continue
        if isinstance(mod, hnn.Conv2D):
            kind = 'conv2d'
        elif isinstance(mod, hnn.BatchNorm1D):
            kind = 'batch_norm1d'
        elif isinstance(mod, hnn._BatchNormBase):
            kind = 'batch_norm2d'
        elif isinstance(mod, hnn.Linear):
            kind = 'linear'
        else:
            kind = type(mod).__name__.lower()
        idx = counters.get(kind, 0)
        counters[kind] = idx + 1
        # a layer's own parameters count up per kind, biases apart (unique_name.generate(<layer>.w / .b)): weight / bias
        # are w_0 / b_0, a ViT's cls_token / pos_embed w_0 / w_1
        nw = nb = 0
        for n in own:
            if n == 'bias':
                names.append('%s_%d.b_%d' % (kind, idx, nb))
                nb += 1
            else:
                names.append('%s_%d.w_%d' % (kind, idx, nw))
                nw += 1
    return names


def paddle_param_names(model):
    """{id(parameter): Paddle auto-name} of every arena parameter of ``model`` (what ``p.name`` is in the reference's
    build_optimizer, passl_v110/solver/builder.py:209-213).  The names count per arena, like _paddle_auto_names."""
    out, arenas = {}, []
    params = list(model.parameters())
    for p in params:
        a = getattr(p, '_passl_arena', None)
        if a is not None and a not in arenas:
            arenas.append(a)
    names = {id(a): _paddle_auto_names(a) for a in arenas}
    for p in params:
        a = getattr(p, '_passl_arena', None)
        if a is not None:
            out[id(p)] = names[id(a)][p._passl_index]
    return out


@OPTIMIZERS.register()
class LarsMomentumOptimizer(_ArenaOptimizer):
    """paddle.fluid.optimizer.LarsMomentumOptimizer (registered by the reference at
    passl_v110/solver/optimizer.py:25, built with ``parameter_list=`` at solver/builder.py:198-201,
    driven through ``minimize(loss)`` / ``clear_gradients()`` by hooks/optimizer_hook.py:26-45)
    as a two-launch multi-tensor update over the flat arena (passl_hip_lars_momentum).

    Rule per parameter tensor (lars_momentum op)  [Paddle-semantics]:
        local_lr = lr * lars_coeff * |p| / (|g| + wd*|p| + epsilon)   if wd > 0, |p| > 0, |g| > 0
                 = lr                                                otherwise
        v = mu*v + local_lr*(g + wd*p);  p = p - v
    ``exclude_from_weight_decay``: wd = 0 for parameters whose *Paddle name* contains one of the
    strings — the yaml's ["scale","offset",".bias"] match none of the dygraph auto-names."""
    type = 'lars_momentum'
    _STATE = (('velocity', '_velocity'),)

    def __init__(self, learning_rate, momentum, lars_coeff=0.001, lars_weight_decay=0.0005,
                 parameter_list=None, regularization=None, grad_clip=None, name=None,
                 exclude_from_weight_decay=None, epsilon=0, multi_precision=False,
                 rescale_grad=1.0):
        if regularization is not None or grad_clip is not None:
            raise NotImplementedError('regularization / grad_clip are not used by configs/simclr')
        self._learning_rate = learning_rate
        self._momentum = float(momentum)
        self._coeff = float(lars_coeff)
        self._wd = float(lars_weight_decay)
        self._eps = float(epsilon)
        self._rescale = float(rescale_grad)
        self._exclude = list(exclude_from_weight_decay or [])
        self._init_arenas(parameter_list)
        self._tables = [self._build_table(a) for a in self._arenas]

    def _build_table(self, arena, chunk=4096):
        names = _paddle_auto_names(arena)
        assert len(names) == len(arena.param_slices)
        blk_off, blk_len, blk_seg, seg_wd = [], [], [], []
        self.param_names = names
        for si, ((off, n), name) in enumerate(zip(arena.param_slices, names)):
            seg_wd.append(0.0 if any(e in name for e in self._exclude) else self._wd)
            for c in range(0, n, chunk):
                blk_off.append(off + c)
                blk_len.append(min(chunk, n - c))
                blk_seg.append(si)
        dev = arena.device
        return dict(blk_off=torch.tensor(blk_off, dtype=torch.int64, device=dev),
                    blk_len=torch.tensor(blk_len, dtype=torch.int32, device=dev),
                    blk_seg=torch.tensor(blk_seg, dtype=torch.int32, device=dev),
                    seg_wd=torch.tensor(seg_wd, dtype=torch.float32, device=dev),
                    norms=torch.zeros(len(seg_wd) + len(blk_len), 2, dtype=torch.float32, device=dev))

    @torch.no_grad()
    def step(self):
        hyper = self._hyper_for_step()
        for a, v, t in zip(self._arenas, self._velocity, self._tables):
            _grads_complete(a)
            ops.lars_momentum_dev(a.flat[:a.n_train], a.grads, v, t, hyper, self._momentum, self._coeff,
                                  self._eps, self.grad_scale * self._rescale)

    def minimize(self, loss=None, startup_program=None, parameters=None, no_grad_set=None):
        """Dygraph ``minimize``: the gradients already exist (the hook called backward())."""
        self.step()


@OPTIMIZERS.register()
class MomentumLARC(LarsMomentumOptimizer):
    """passl/optimizer/momentum_larc.py:25-111 (the optimizer of the SimSiam linear-probe recipe,
    tasks/ssl/simsiam/configs/simsiam_resnet50_lp_in1k_1n8c_dp_fp32.yaml) as the multi-tensor LARS machinery with the
    LARC update (passl_hip_larc_momentum_dev).  Rule per parameter tensor:
        if |p| != 0 and |g| != 0:  a = trust_coefficient |p| / (|g| + |p| wd + eps)   [clip: a = min(a / lr, 1)]
                                   g = a (g + wd p)
        v = mu v + g;  p -= lr v          (a zero-norm tensor takes its raw gradient, without weight decay)
    Unlike LARS the learning rate multiplies the velocity, not the gradient: a schedule rescales the whole history.
    ``use_master_param``: parameters are fp32 masters here anyway."""
    type = 'momentum_larc'

    def __init__(self, learning_rate=0.0, momentum=0.9, weight_decay=0.0, trust_coefficient=0.02, clip=True,
                 eps=1e-8, use_master_param=True, grad_clip=None, parameters=None, lr_func=None, **args):
        if grad_clip is not None or lr_func is not None:
            raise NotImplementedError('grad_clip / lr_func are not used by the linear-probe recipes')
        super().__init__(learning_rate, momentum, lars_coeff=trust_coefficient, lars_weight_decay=weight_decay,
                         parameter_list=parameters, epsilon=eps)
        self._clip = bool(clip)

    @torch.no_grad()
    def step(self):
        hyper = self._hyper_for_step()
        for a, v, t in zip(self._arenas, self._velocity, self._tables):
            _grads_complete(a)
            ops.larc_momentum_dev(a.flat[:a.n_train], a.grads, v, t, hyper, self._momentum, self._coeff,
                                  self._eps, self._clip, self.grad_scale * self._rescale)


_GROUP_KEYS = ('params', 'weight_decay', 'learning_rate', 'lr_scale')


def _listed_parameters(parameters, default_wd):
    """A plain list or a list of group dicts -> [(parameter, multiplier, decay, group)] of the trainable ones (a plain
    list is group 0 with multiplier 1 and the optimizer's decay)."""
    parameters = list(parameters or [])
    if not any(isinstance(g, dict) for g in parameters):
        return [(p, 1.0, default_wd, 0) for p in parameters if p.requires_grad]
    if not all(isinstance(g, dict) for g in parameters):
        raise ValueError('parameters: a list of tensors or a list of group dicts, not a mixture')
    listed = []
    for gi, group in enumerate(parameters):
        unknown = [k for k in group if k not in _GROUP_KEYS]
        if unknown or 'params' not in group:
            raise ValueError('parameter group %d: keys %r (known: %r, params required)'
                             % (gi, sorted(group), _GROUP_KEYS))
        if 'learning_rate' in group and 'lr_scale' in group:
            raise ValueError('parameter group %d gives its multiplier twice (learning_rate and lr_scale)' % gi)
        scale = float(group.get('learning_rate', group.get('lr_scale', 1.0)))
        wd = group.get('weight_decay', None)
        wd = default_wd if wd is None else float(wd)
        if wd < 0:
            raise ValueError('parameter group %d: weight_decay must be >= 0, got %r' % (gi, wd))
        listed += [(p, scale, wd, gi) for p in group['params'] if p.requires_grad]
    return listed


def _arena_rows(names, listed, lr_ratio, apply_decay_param_fun, grad_clip):
    """One arena: its Paddle auto-names and its entries of ``listed`` -> (rows, sets) in arena order.  rows[i] = (name,
    multiplier, decay) after ``lr_ratio`` / ``apply_decay_param_fun``; sets[i] = the clip set of the parameter (its
    group under the 'group' scope, 0 under 'global'), -1 when it is left out of clipping or nothing is clipped."""
    rows, sets = [None] * len(names), [-1] * len(names)
    for p, scale, wd, gi in listed:
        name = names[p._passl_index]
        if grad_clip is not None and not grad_clip.excludes(p, name):
            sets[p._passl_index] = 0 if grad_clip.scope == 'global' else gi
        if lr_ratio is not None:
            scale = scale * float(lr_ratio(p))
        if apply_decay_param_fun is not None and not apply_decay_param_fun(name):
            wd = 0.0
        rows[p._passl_index] = (name, scale, wd)
    return rows, sets


def _slot_ends(param_slices, n_train):
    """Exclusive end of every parameter's slot: slot padding goes with the parameter in front of it."""
    return [off for off, _n in param_slices[1:]] + [n_train]


def _clip_runs(param_slices, n_train, sets):
    """-> [(start, end, set)]: the clipped slots of one arena, adjacent slots of equal set merged (the chunk table of
    ops.grad_clip_plan)."""
    runs = []
    for (start, _n), end, st in zip(param_slices, _slot_ends(param_slices, n_train), sets):
        if st < 0:
            continue
        if runs and runs[-1][1] == start and runs[-1][2] == st:
            runs[-1] = (runs[-1][0], end, st)
        else:
            runs.append((start, end, st))
    return runs


def _flat_or_segments(param_slices, n_train, rows, sets):
    """The launch of one arena.  ``sets``: None without a clip plan.  -> (flat, segments), one of them None:
    flat = (decay, set or None) when every multiplier is exactly 1.0 and all decays and sets are equal — the flat
    kernel, launch for launch what a plain list gets; segments = (seg_end, seg_scale, seg_wd, seg_set or None), adjacent
    parameters of equal (multiplier, decay, set) merged.  An arena none of whose parameters is clipped has no sets: it
    takes the unclipped launch."""
    if sets is not None and all(st < 0 for st in sets):
        sets = None
    if all(s == 1.0 for _n, s, _w in rows) and len({w for _n, _s, w in rows}) == 1 \
            and (sets is None or len(set(sets)) == 1):
        return (rows[0][2], None if sets is None else sets[0]), None
    seg_end, seg_scale, seg_wd, seg_set = [], [], [], []
    for end, (_name, scale, wd), st in zip(_slot_ends(param_slices, n_train), rows, sets or [None] * len(rows)):
        if seg_end and (seg_scale[-1], seg_wd[-1], seg_set[-1]) == (scale, wd, st):
            seg_end[-1] = end
        else:
            seg_end.append(end)
            seg_scale.append(scale)
            seg_wd.append(wd)
            seg_set.append(st)
    return None, (seg_end, seg_scale, seg_wd, None if sets is None else seg_set)


class _GroupedArenaOptimizer(_ArenaOptimizer):
    """An arena optimizer with ONE update launch per arena, parameter groups, global-norm clipping and a step count:
    what AdamW and Adan share.  A subclass adds its ``_STATE``, its ``_host_values`` (which advances ``_t``) and its
    ``_update``, the four launches of its rule.

    A float ``weight_decay`` decays EVERY trainable parameter (configs/mae/mae_vit_b_pretrain.yaml has no
    exclusion list; fixed sin-cos embeddings are buffers and are not touched).

    Parameter groups (ViT fine-tuning: solver/lr_decay.py, build_optimizer's ``layer_decay``): ``parameters`` may be a
    list of dicts {params, weight_decay (default: the optimizer's), learning_rate | lr_scale}.  The multiplier is
    spelled ``learning_rate`` in Paddle's groups (a group's learning_rate multiplies the optimizer's
    [Paddle-semantics]) and ``lr_scale`` in the v2 tree (passl/optimizer/optimizer.py:117-123); ``lr_ratio(param)``
    multiplies it; ``apply_decay_param_fun(name)`` — name = the Paddle auto-name (_paddle_auto_names) — switches the
    decay of a parameter off.  Every trainable parameter of an arena is listed exactly once.  The result is ONE table
    per arena (arena order, adjacent parameters with equal (multiplier, decay) merged; slot padding goes with the
    parameter in front of it) for the grouped kernel (ops.adamw_groups_table: AdamW's and Adan's kernels read the same
    table).  Multipliers all exactly 1.0 and decays all equal = the flat kernel, launch for launch what a plain list
    gets.  The table is configuration, not state: state_dict() holds the flat state vectors and the step count ``t``.

    ``grad_clip`` (core.grad_clip.ClipGradByGlobalNorm): the clip set of a parameter joins (multiplier, decay) in the
    merge, and ``_update`` states the choice of launch per arena once — flat or grouped, each with or without the
    coefficient.  ``step`` with clipping: every arena's gradients complete, the chunk sums (one launch per arena), one
    finalize for all sets, then the updates.  Nothing comes back to the host: the coefficients are read by the update
    kernels from device memory."""

    def _init_groups(self, learning_rate, parameters, weight_decay, grad_clip, lr_ratio=None,
                     apply_decay_param_fun=None):
        """Listed parameters -> rows -> runs -> launches -> device tables, and the clip plan over all arenas."""
        if grad_clip is not None and not isinstance(grad_clip, ClipGradByGlobalNorm):
            raise NotImplementedError('grad_clip: only core.grad_clip.ClipGradByGlobalNorm is built, got %r'
                                      % (type(grad_clip).__name__,))
        self._learning_rate = learning_rate
        self._wd = float(weight_decay) if weight_decay else 0.0
        if self._wd < 0:
            raise ValueError('weight_decay must be >= 0, got %r' % (weight_decay,))
        self._grad_clip = grad_clip
        self._t = 0
        listed = _listed_parameters(parameters, self._wd)
        self._init_arenas([p for p, _s, _w, _g in listed])
        arenas = self._arenas
        names = [_paddle_auto_names(a) for a in arenas]
        assert all(len(n) == len(a.param_slices) for n, a in zip(names, arenas))
        per_arena = [_arena_rows(n, [e for e in listed if e[0]._passl_arena is a], lr_ratio, apply_decay_param_fun,
                                 grad_clip) for n, a in zip(names, arenas)]
        self._param_table = [rows for rows, _sets in per_arena]    # per arena: [(auto-name, multiplier, decay)]
        self._param_sets = [sets for _rows, sets in per_arena]     # per arena: the clip set of every parameter
        runs = [_clip_runs(a.param_slices, a.n_train, sets) for a, sets in zip(arenas, self._param_sets)]
        launches = [_flat_or_segments(a.param_slices, a.n_train, rows, sets if any(runs) else None)
                    for a, (rows, sets) in zip(arenas, per_arena)]
        # device tables from here on
        self._clip = None              # ops.grad_clip_plan over all arenas, or None: nothing is clipped
        if any(runs):
            n_sets = 1 if grad_clip.scope == 'global' else max(g for _p, _s, _w, g in listed) + 1
            self._clip = ops.grad_clip_plan(runs, [a.n_train for a in arenas], n_sets, arenas[0].device)
        self._tables = []              # per arena: None (flat kernel with _flat_wd) or the device table
        self._flat_wd = []
        self._clip_coef = []           # per arena: the device float of its one set (flat clip launch) or None
        for a, (flat, segments) in zip(arenas, launches):
            if flat is not None:
                wd, st = flat
                table, coef = None, None if st is None else self._clip['out'][st, 1:]
            else:
                wd, coef = None, None
                seg_end, seg_scale, seg_wd, seg_set = segments
                if seg_set is None:
                    table = ops.adamw_groups_table(seg_end, seg_scale, seg_wd, a.n_train, a.device)
                else:
                    table = ops.adamw_groups_clip_table(seg_end, seg_scale, seg_wd, seg_set, a.n_train,
                                                        self._clip['n_sets'], a.device)
            self._tables.append(table)
            self._flat_wd.append(wd)
            self._clip_coef.append(coef)

    @property
    def grouped(self):
        """True when some arena takes the grouped launch (a multiplier != 1 or more than one decay)."""
        return any(t is not None for t in self._tables)

    def param_table(self):
        """[(name, lr multiplier, weight decay)] of every parameter in arena order (arena after arena); name = the
        Paddle auto-name ``apply_decay_param_fun`` was asked about."""
        return [row for rows in self._param_table for row in rows]

    def _update(self, i, hyper):
        """The update launch of arena i: flat or grouped, each with or without a clip coefficient."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self):
        hyper = self._hyper_for_step()
        clip, gc = self._clip, self._grad_clip
        if clip is None:
            for i, a in enumerate(self._arenas):
                _grads_complete(a)
                self._update(i, hyper)
            return
        for a in self._arenas:
            _grads_complete(a)
        for b, a in enumerate(self._arenas):
            ops.grad_sumsq(a.grads, clip, b, self.grad_scale)
        ops.grad_clip_finalize(clip, gc.clip_norm, gc.clip_norm_max, gc.always_clip)
        for i in range(len(self._arenas)):
            self._update(i, hyper)

    def grad_norms(self):
        """The device table [n_sets, 2] = {norm, coef} of the last step's sets (set = parameter group under the 'group'
        scope, one set under 'global'), without synchronising: a caller who logs it reads it when it likes.  None without
        clipping."""
        return None if self._clip is None else self._clip['out']

    def clip_sets(self):
        """[(name, set)] of every parameter in arena order; set -1 = left out of clipping (or no clipping at all)."""
        return [(row[0], st) for rows, sets in zip(self._param_table, self._param_sets) for row, st in zip(rows, sets)]

    def state_dict(self):
        return dict(super().state_dict(), t=self._t)

    def set_state_dict(self, sd):
        self._t = int(sd['t'])
        super().set_state_dict(sd)


@OPTIMIZERS.register()
class AdamW(_GroupedArenaOptimizer):
    """paddle.optimizer.AdamW (registered by the reference at passl_v110/solver/optimizer.py:22) as ONE
    launch over the flat arena.  adamw op  [Paddle-semantics]:
        p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
        p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps*sqrt(1-b2^t))
    Groups, ``lr_ratio`` / ``apply_decay_param_fun`` and ``grad_clip``: _GroupedArenaOptimizer."""
    type = 'adamw'
    _STATE = (('moment1', '_m'), ('moment2', '_v'))

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-08, parameters=None,
                 weight_decay=0.01, lr_ratio=None, apply_decay_param_fun=None, grad_clip=None,
                 lazy_mode=False, multi_precision=False, name=None, betas=None, eps=None,
                 use_master_param=None, exp_avg_force_fp32=None):
        # v2 spelling (passl/optimizer/adamw.py:24-50, the MoCo-v3 yaml): betas=(b1, b2), eps.  use_master_param /
        # exp_avg_force_fp32 ask for fp32 master weights and an fp32 first moment next to fp16 parameters: the
        # flat arena IS fp32 (weights and both moments; the compute-dtype copy is derived from it every step), so
        # both are always satisfied and the flags are accepted as no-ops.
        if betas is not None:
            beta1, beta2 = (float(b) for b in betas)
        if eps is not None:
            epsilon = eps
        self._b1, self._b2, self._eps = float(beta1), float(beta2), float(epsilon)
        self._init_groups(learning_rate, parameters, weight_decay, grad_clip, lr_ratio, apply_decay_param_fun)

    def _host_values(self):
        self._t += 1
        return self.get_lr(), self._b1 ** self._t, self._b2 ** self._t

    def _update(self, i, hyper):
        a, m, v, table, coef = self._arenas[i], self._m[i], self._v[i], self._tables[i], self._clip_coef[i]
        p = a.flat[:a.n_train]
        if table is None and coef is None:
            ops.adamw_dev(p, a.grads, m, v, hyper, self._b1, self._b2, self._eps, self._flat_wd[i], self.grad_scale)
        elif table is None:
            ops.adamw_clip_dev(p, a.grads, m, v, hyper, coef, self._b1, self._b2, self._eps, self._flat_wd[i],
                               self.grad_scale)
        elif 'seg_set' not in table:
            ops.adamw_groups_dev(p, a.grads, m, v, table, hyper, self._b1, self._b2, self._eps, self.grad_scale)
        else:
            ops.adamw_groups_clip_dev(p, a.grads, m, v, table, hyper, self._clip['out'], self._b1, self._b2, self._eps,
                                      self.grad_scale)


@OPTIMIZERS.register()
class Adan(_GroupedArenaOptimizer):
    """passl/optimizer/adan.py (arXiv 2208.06677; the optimizer of the reference's
    ViT_base_patch16_224_in1k_adan_1n8c_dp_fp16o2.yaml) as ONE launch over the flat arena and four flat state vectors
    (csrc/adan.hip), where the reference issues some twenty element-wise ops per parameter.  With gg the scaled,
    clipped gradient (adan.py:117-148, is_vanilla=False):
        diff = gg - pre_grad  (0 at t == 1);  m = b1 m + (1-b1) gg;  d = b2 d + (1-b2) diff;
        u = gg + b2 diff;  s = b3 s + (1-b3) u^2;  upd = (m/(1-b1^t) + b2 d/(1-b2^t)) / (sqrt(s)/sqrt(1-b3^t) + eps)
        p = (p - lr upd) / (1 + lr wd)        [no_prox: p = p (1 - lr wd) - lr upd];   pre_grad = gg
    The hyper block is 8 floats {lr, b1^t, b2^t, b3^t, first, 0, 0, 0}.  ``first`` (1.0 at t == 1) stands for the
    reference creating its state with pre_grad = grad.clone(); it is read on the device like the rate, so a step plan
    recorded at t == 1 replays correctly at t >= 2 — and a run resumed from a state_dict (t >= 1) never takes the
    first-step branch again.  ``param.grad`` keeps the unclipped gradient.
    Groups and ``grad_clip``: _GroupedArenaOptimizer.  ``use_master_param``: the arena IS fp32, a no-op.  Refused:
    ``is_vanilla`` (another state set; no recipe uses it) and ``lr_func`` groups."""
    type = 'adan'
    _STATE = (('exp_avg', '_m'), ('exp_avg_diff', '_d'), ('exp_avg_sq', '_s'), ('pre_grad', '_pre'))
    _HYPER_WIDTH = 8

    def __init__(self, learning_rate=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, weight_decay=0.0, no_prox=False,
                 grad_clip=None, use_master_param=None, is_vanilla=False, lr_func=None, parameters=None, lr=None):
        if lr is not None:
            learning_rate = lr
        if is_vanilla:
            raise NotImplementedError('Adan(is_vanilla=True) keeps another state set and is used by no recipe')
        if lr_func is not None:
            raise NotImplementedError('Adan(lr_func=...): LRCallable groups are not built')
        betas = tuple(float(b) for b in betas)
        if len(betas) != 3:
            raise ValueError('Adan takes three betas, got %r' % (betas,))
        if not 0.0 <= eps:                                       # adan.py:59-66
            raise ValueError('Invalid epsilon value: {}'.format(eps))
        for k, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError('Invalid beta parameter at index {}: {}'.format(k, b))
        self._b1, self._b2, self._b3 = betas
        self._eps = float(eps)
        self._no_prox = bool(no_prox)
        self._init_groups(learning_rate, parameters, weight_decay, grad_clip)

    def _host_values(self):
        self._t += 1
        t = self._t
        return self.get_lr(), self._b1 ** t, self._b2 ** t, self._b3 ** t, 1.0 if t == 1 else 0.0

    def _update(self, i, hyper):
        a, table, coef = self._arenas[i], self._tables[i], self._clip_coef[i]
        bufs = (a.flat[:a.n_train], a.grads, self._m[i], self._d[i], self._s[i], self._pre[i])
        cfg = (self._b1, self._b2, self._b3, self._eps)
        if table is None and coef is None:
            ops.adan_dev(*bufs, hyper, *cfg, self._flat_wd[i], self._no_prox, self.grad_scale)
        elif table is None:
            ops.adan_clip_dev(*bufs, hyper, coef, *cfg, self._flat_wd[i], self._no_prox, self.grad_scale)
        elif 'seg_set' not in table:
            ops.adan_groups_dev(*bufs, table, hyper, *cfg, self._no_prox, self.grad_scale)
        else:
            ops.adan_groups_clip_dev(*bufs, table, hyper, self._clip['out'], *cfg, self._no_prox, self.grad_scale)
