"""Parameter groups for ViT fine-tuning: layer-wise learning-rate decay and the no-weight-decay sets.

Two rules exist in the reference, and they differ; both are restated here and feed ``solver.optimizer.AdamW``:

  v2 rule   ``param_groups_lrd`` / ``get_layer_id_for_vit`` — tasks/ssl/mae/util/lr_decay.py:23-90, called from
            tasks/ssl/mae/main_finetune.py:478-484.  Ladder of ``num_layers + 1`` multipliers,
            ``layer_decay ** (num_layers - id)`` with ``num_layers = len(blocks) + 1``: the embeddings (id 0) get
            ``layer_decay ** num_layers``, block i gets id i + 1, everything else (final norm, head) the top id =
            multiplier 1.  No decay for 1-D parameters and for the names of ``no_weight_decay_list`` (the recipe passes
            pos_embed / cls_token / dist_token).  Group key ``lr_scale``.
  v110 rule ``get_parameter_groups`` / ``LayerDecayValueAssigner`` / ``get_num_layer_for_vit`` —
            passl_v110/solver/builder.py:91-159, driven by build_optimizer's ``layer_decay`` (:181-192).  Ladder of
            ``num_layers + 2`` multipliers, ``layer_decay ** (num_layers + 1 - id)`` with
            ``num_layers = backbone.get_num_layers()`` (= len(blocks)): everything that is neither embedding nor block
            gets id ``len(ladder) - 1`` = multiplier 1.  No decay for 1-D parameters, names ending in ``.bias`` and the
            skip list — ``pos_embed`` and ``cls_token`` ARE decayed unless listed.  Group key ``learning_rate``
            (a Paddle group's learning_rate multiplies the optimizer's  [Paddle-semantics]).

With len(blocks) = L both ladders give block i the multiplier layer_decay ** (L - i) and the embeddings
layer_decay ** (L + 1); the rules differ in the decay of pos_embed / cls_token only (given the recipe's list).

The multipliers are computed with the reference's own Python expressions, so they are the same Python floats.
"""


def _trainable(p):
    return p.requires_grad


def get_layer_id_for_vit(name, num_layers):
    """v2 rule: depth index of a parameter of the ViT.  ``name`` is relative to the ViT (no ``backbone.`` prefix)."""
    if name in ('cls_token', 'pos_embed') or name.startswith('patch_embed'):
        return 0
    if name.startswith('blocks'):
        return int(name.split('.')[1]) + 1
    return num_layers


def _strip_backbone(name):
    return name[len('backbone.'):] if name.startswith('backbone.') else name


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=.75, num_layers=None):
    """v2 rule -> [{'lr_scale', 'weight_decay', 'params'}], groups in order of first appearance.

    ``model`` is the ViT or a wrapper that holds it as ``backbone`` (MAE_FINETUNE): a leading ``backbone.`` is stripped
    before names are matched, so the wrapper's head lands at the top id — the reference called on the ViT, with the head
    added at multiplier 1."""
    if num_layers is None:
        vit = getattr(model, 'backbone', model)
        num_layers = len(vit.blocks) + 1
    scales = [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
    listed = set(no_weight_decay_list)
    groups = {}
    for full_name, p in model.named_parameters():
        if not _trainable(p):
            continue
        name = _strip_backbone(full_name)
        no_decay = p.ndim == 1 or name in listed
        layer_id = get_layer_id_for_vit(name, num_layers)
        key = (layer_id, no_decay)
        if key not in groups:
            groups[key] = {'lr_scale': scales[layer_id], 'weight_decay': 0. if no_decay else weight_decay,
                           'params': []}
        groups[key]['params'].append(p)
    return list(groups.values())


def get_num_layer_for_vit(var_name, num_max_layer):
    """v110 rule: depth index of a parameter of a model that holds the ViT as ``backbone``."""
    if var_name in ('backbone.cls_token', 'backbone.mask_token', 'backbone.pos_embed'):
        return 0
    if var_name.startswith('backbone.patch_embed'):
        return 0
    if var_name.startswith('backbone.blocks'):
        return int(var_name.split('.')[2]) + 1
    return num_max_layer - 1          # relative position bias, final norm, head


class LayerDecayValueAssigner(object):
    """The ladder of multipliers and the name -> depth index map that goes with its length."""

    def __init__(self, values):
        self.values = values

    def get_scale(self, layer_id):
        return self.values[layer_id]

    def get_layer_id(self, var_name):
        return get_num_layer_for_vit(var_name, len(self.values))


def get_parameter_groups(cfg, model, skip_list=(), get_num_layer=None, get_layer_scale=None):
    """v110 rule -> [{'weight_decay', 'params', 'learning_rate'}], groups in order of first appearance.
    ``cfg['weight_decay']`` is the decay of the decayed groups."""
    weight_decay = cfg['weight_decay']
    groups = {}
    for name, p in model.named_parameters():
        if not _trainable(p):
            continue
        no_decay = len(p.shape) == 1 or name.endswith('.bias') or name in skip_list
        layer_id = get_num_layer(name) if get_num_layer is not None else None
        key = (layer_id, no_decay)
        if key not in groups:
            scale = get_layer_scale(layer_id) if get_layer_scale is not None else 1.
            groups[key] = {'weight_decay': 0. if no_decay else weight_decay, 'params': [], 'learning_rate': scale}
        groups[key]['params'].append(p)
    return list(groups.values())


def table_by_name(model, groups):
    """[(state-dict name, multiplier, weight decay)] in ``model.named_parameters()`` order for a list of groups of
    either spelling — what the log prints and the tests compare."""
    of = {}
    for g in groups:
        scale = g.get('learning_rate', g.get('lr_scale', 1.0))
        for p in g['params']:
            of[id(p)] = (scale, g['weight_decay'])
    return [(n,) + of[id(p)] for n, p in model.named_parameters() if id(p) in of]
