"""``Model`` — reference passl/models/base_model.py:25-40: a Layer with ``load_pretrained`` / ``save``; here also what
the models over one flat arena (``arena_q``) share: the arena follows weights written from outside."""
import torch

from ..hip import nn as hnn
from ..modules.vit import trunc_normal_
from ..utils.checkpoint import save_pdparams


class Model(hnn.Layer):
    def load_pretrained(self, path, rank=0, finetune=False):
        raise Exception('NotImplementedError, you must overwrite load_pretrained method in subclass.')

    def save(self, path, local_rank=0, rank=0):
        save_pdparams(self, path, rank)

    def sync_runtime_state(self):
        """After weights were written from outside (checkpoint, pre-trained file, broadcast): the compute-dtype operands
        of ``arena_q`` follow them.  A model without an arena of its own (the plain ResNet, ``ArchModel``) has nothing to
        do; one with more runtime state overrides this."""
        arena = getattr(self, 'arena_q', None)
        if arena is not None:
            arena.refresh()

    def load_state_dict(self, state_dict, strict=True):
        r = super().load_state_dict(state_dict, strict=strict)
        self.sync_runtime_state()
        return r


class ClassifierModel(Model):
    """timm's ``get_classifier`` / ``reset_classifier`` for a model with ``head`` / ``num_features`` / ``global_pool``
    whose parameters all live in ``arena_q``.  ``GLOBAL_POOLS``: the pools the model's constructor allows."""

    GLOBAL_POOLS = ('', 'avg')

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=None):
        """A new trunc-normal(0.02) head of ``num_classes`` (None for 0); the arena is laid out again over the new
        parameter set."""
        self.num_classes = num_classes
        if global_pool is not None:
            assert global_pool in self.GLOBAL_POOLS
            self.global_pool = global_pool
        self.head = None
        if num_classes > 0:
            self.head = hnn.Linear(self.num_features, num_classes)
            with torch.no_grad():
                trunc_normal_(self.head.weight, std=.02)
                self.head.bias.zero_()
        self.arena_q = hnn.EncoderArena(self, trainable=True)
