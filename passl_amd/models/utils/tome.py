"""``passl.models.utils.tome`` — token merging (ToMe) for the v2 ``VisionTransformer`` / ``MAEVisionTransformer`` on the
MI355X HIP path.

Public names are the reference's (passl/models/utils/tome.py): ``parse_r`` :198-224, ``bipartite_soft_matching``
:28-118, ``merge_wavg`` :121-133, ``apply_patch`` :275-302::

    from passl.models.utils import tome
    tome.apply_patch(model)            # prop_attn=True for off-the-shelf evaluation
    model.r = 16                       # or (16, -1), or a list per layer

What differs from the reference is where the work runs.  The reference returns closures over index tensors; here the
matching is one kernel launch on the block's own qkv projection (csrc/tome.hip: the metric ``k.mean(1)``, the scores,
the ranking and the output rows never leave the workgroup), its result a ``MergePlan`` around ``dest`` int32 [B, T], and
the merge a gather over ``dest`` with a gather as its gradient.  Per-layer ``r_i`` and token counts ``T_i`` are host
arithmetic on ``T`` and the schedule: nothing is read back from the device during a pass.

Not built: ``class_token=False`` / ``distill_token=True`` (every model here has exactly the class token); the
size-weighted global pool (``global_pool=True`` is outside this repository's ViTs); ``unmerge`` (no user in the
reference's ViT path); ``prop_attn=True`` with gradients enabled (the reference keeps proportional attention for
off-the-shelf evaluation, tome.py:279-280; the kernel has no backward); element-wise dropout or stochastic depth
together with ``r > 0`` in training mode (their masks are keyed by row position, which merging changes; no recipe
combines them)."""
from typing import List, Tuple, Union

import torch

from ...hip import nn, ops
from ...modules.vit import Block
from ..vision_transformer import VisionTransformer

__all__ = ['parse_r', 'bipartite_soft_matching', 'merge_wavg', 'apply_patch', 'MergePlan', 'token_schedule']


def parse_r(num_layers: int, r: Union[List[int], Tuple[int, float], int]) -> List[int]:
    """A constant r, an (r, inflection) pair or a list per layer -> the list per layer (the reference's arithmetic)."""
    inflect = 0
    if isinstance(r, list):
        if len(r) < num_layers:
            r = r + [0] * (num_layers - len(r))
        return list(r)
    elif isinstance(r, tuple):
        r, inflect = r

    min_val = int(r * (1.0 - inflect))
    max_val = 2 * r - min_val
    step = (max_val - min_val) / (num_layers - 1)

    return [int(min_val + step * i) for i in range(num_layers)]


def token_schedule(T, rs):
    """-> (r_i after the clamp of tome.py:53 with the class token protected, T_i entering block i, T after the last)."""
    r_out, t_in = [], []
    for r in rs:
        t_in.append(T)
        r = max(min(int(r), ops.tome_max_r(T)), 0)
        r_out.append(r)
        T -= r
    return r_out, t_in, T


class MergePlan:
    """One block's matching: ``dest`` int32 [B, T] = the output row of every token; ``node_max`` / ``node_idx`` (the
    best score and partner of every even token) when asked for."""

    __slots__ = ('dest', 'node_max', 'node_idx', 'B', 'T', 'r')

    def __init__(self, dest, node_max, node_idx, B, T, r):
        self.dest, self.node_max, self.node_idx, self.B, self.T, self.r = dest, node_max, node_idx, B, T, r


def bipartite_soft_matching(qkv, r, B, T, H, DH, class_token=True, distill_token=False, want_nodes=False):
    """Balanced bipartite matching on the K slice of ``qkv`` [B*T, 3*H*DH] -> a MergePlan, or None when nothing is merged
    (r <= 0 after the clamp)."""
    if distill_token or not class_token:
        raise NotImplementedError('bipartite_soft_matching: only class_token=True, distill_token=False is built')
    r = min(int(r), ops.tome_max_r(T))
    if r <= 0:
        return None
    with torch.no_grad():
        res = ops.tome_match(qkv.detach(), B, T, H, DH, r, want_nodes=want_nodes)
    dest, nmax, nidx = res if want_nodes else (res, None, None)
    return MergePlan(dest, nmax, nidx, B, T, r)


def merge_wavg(plan, x, size=None, want_log=False):
    """Size-weighted average of the rows ``x`` [B*T, C] over the plan -> (x [B*(T-r), C], size fp32 [B, T-r]) and with
    ``want_log`` also log(size).  ``size`` None = all ones."""
    if plan is None:
        raise ValueError('merge_wavg needs a plan (bipartite_soft_matching returned None: nothing to merge)')
    return nn.tome_merge(x, size, plan.dest, plan.B, plan.T, plan.r, want_log=want_log)


class ToMeBlock(Block):
    """Block with the merge between the attention and the MLP (tome.py:143-162)."""

    def forward_tome(self, x, B, T, r, size, log_size, info):
        attn = self.attn
        h, xr = self.norm1.fork(x)
        qkv = attn.qkv(h)
        a = nn.attention(qkv, B, T, attn.num_heads, attn.head_dim, attn.scale, causal=attn.causal,
                         key_bias=log_size if info['prop_attn'] else None)
        x = attn.proj(a, residual=xr)
        if r > 0:
            trace = info.get('trace')
            plan = bipartite_soft_matching(qkv, r, B, T, attn.num_heads, attn.head_dim, info['class_token'],
                                           info['distill_token'], want_nodes=trace is not None)
            if trace is not None:
                trace.append((plan.dest, plan.node_max, plan.node_idx))
            res = merge_wavg(plan, x, size, want_log=info['prop_attn'])
            x, size = res[0], res[1]
            log_size = res[2] if info['prop_attn'] else None
            T -= plan.r
        h, xr = self.norm2.fork(x)
        return self.mlp(h, residual=xr), size, log_size, T


def make_tome_class(transformer_class):
    class ToMeVisionTransformer(transformer_class):
        """forward_features with a token count that shrinks by r_i after the attention of block i."""

        def forward_features(self, x):
            info = self._tome_info
            rs = parse_r(len(self.blocks), self.r)
            info['r'] = rs
            info['size'] = None
            if not any(r > 0 for r in rs):
                return super().forward_features(x)            # r = 0: the unpatched path, launch for launch
            if self.training and (self.drop_rate > 0. or any(b.drop > 0. or b.drop_path > 0. for b in self.blocks)):
                raise NotImplementedError('token merging with r > 0 in training mode needs drop_rate = 0 and no '
                                          'stochastic depth (their masks are keyed by row position)')
            if info['prop_attn'] and torch.is_grad_enabled():
                raise NotImplementedError('prop_attn=True is for evaluation under torch.no_grad(): proportional '
                                          'attention has no backward (train with prop_attn=False)')
            x, _, B, L = self.embed_tokens(x, self.cls_token, self.pos_embed)
            x = self.pos_drop(x)
            r_i, _, T_final = token_schedule(L + 1, rs)
            T, size, log_size = L + 1, None, None
            for blk, r in zip(self.blocks, r_i):
                x, size, log_size, T = blk.forward_tome(x, B, T, r, size, log_size, info)
            assert T == T_final
            info['size'] = size
            cls_rows = self.identity_ids(B, T_final - 1, x.device)[1]      # the class row of image b is b * T_final
            return self.cls_features(x, cls_rows, self.norm)

    ToMeVisionTransformer.__name__ = 'ToMe' + transformer_class.__name__
    return ToMeVisionTransformer


def apply_patch(model: VisionTransformer, prop_attn: bool = False):
    """Applies ToMe to this transformer.  Afterward, set r using ``model.r``.  ``state_dict()`` is unchanged.

    ``prop_attn=True`` (proportional attention) is for evaluating models off the shelf; for training set it False."""
    if not isinstance(model, VisionTransformer):
        raise NotImplementedError('apply_patch: %s is not a passl.models VisionTransformer / MAEVisionTransformer'
                                  % type(model).__name__)
    if getattr(model, 'global_pool', False):
        raise NotImplementedError('apply_patch: the size-weighted global pool is not built')
    if getattr(model, 'dist_token', None) is not None:
        raise NotImplementedError('apply_patch: a distillation token is not built')
    if any(blk.attn.causal for blk in model.blocks):
        raise NotImplementedError('apply_patch: a causal tower is not a ToMe target')
    if hasattr(model, '_tome_info'):
        model._tome_info['prop_attn'] = bool(prop_attn)
        return model
    model.__class__ = make_tome_class(model.__class__)
    model.r = 0
    model._tome_info = {
        'r': model.r,
        'size': None,
        'prop_attn': bool(prop_attn),
        'class_token': model.cls_token is not None,
        'distill_token': False,
    }
    for blk in model.blocks:
        blk.__class__ = ToMeBlock
        blk._tome_info = model._tome_info
    return model
