"""CELoss — reference passl/loss/celoss.py:22-56, returned as ``{"CELoss": loss}``.

Integer labels without ``epsilon``: mean softmax cross entropy, one kernel (csrc/clas.hip: row log-sum-exp, the label's
score and the top-1 / top-5 ranks in one pass; backward = softmax - one_hot scaled by the incoming gradient).
``epsilon`` (label smoothing, celoss.py:30-46): the smoothed target (1 - eps) onehot + eps / C comes from
``ops.mixup_target`` with lam = 1 for integer labels, or is (1 - eps) t + eps / C of a given soft label; then the
soft-target cross-entropy of csrc/mixup.hip.  A soft label [N, C] without ``epsilon`` (mixup / cutmix targets, :48-49)
goes to that kernel as it is.  tasks/ssl/mae/util/loss.py's LabelSmoothingCrossEntropy is the same number as
``CELoss(epsilon)`` and SoftTargetCrossEntropy the same as ``CELoss()`` on a soft label."""
import torch
from torch.autograd import Function

from ..hip import nn as hnn
from ..hip import ops
from ..modeling.heads.clas_head import _SoftCEFn, _SoftmaxCEFn


class CELoss(hnn.Layer):
    """Softmax Cross entropy loss"""

    def __init__(self, epsilon=None):
        super().__init__()
        if epsilon is not None:
            assert epsilon >= 0 and epsilon <= 1, 'epsilon must be in [0, 1]'
        self.epsilon = epsilon

    def forward(self, x, label):
        if isinstance(x, dict):
            x = x['logits']
        x = x.float()
        class_num = x.shape[-1]
        soft = label.dim() > 1 and label.shape[-1] == class_num
        if self.epsilon is not None:
            if soft:
                target = label.float() * (1. - self.epsilon) + self.epsilon / class_num
            else:
                target = ops.mixup_target(label.contiguous().long().view(-1), class_num, 1., self.epsilon)
            loss, _acc1, _acc5 = _SoftCEFn.apply(x, target)
        elif soft:
            loss, _acc1, _acc5 = _SoftCEFn.apply(x, label.float())
        else:
            loss, _acc1, _acc5 = _SoftmaxCEFn.apply(x, label.contiguous().long().view(-1))
        return {'CELoss': loss.reshape(())}


class _SigmoidCEFn(Function):
    """mean_i sum_c BCE-with-logits(x_ic, t_ic), t = t_on at the label and t_off elsewhere (csrc/clas.hip): one row
    kernel + the fixed-order finish forward, one element kernel backward.  No dense target is built."""

    @staticmethod
    def forward(ctx, scores, labels, t_on, t_off):
        ctx.set_materialize_grads(False)
        scores = scores.contiguous()
        ctx.save_for_backward(scores, labels)
        ctx.targets = (t_on, t_off)
        return ops.sigmoid_ce_fwd(scores, labels, t_on, t_off)

    @staticmethod
    def backward(ctx, gloss):
        scores, labels = ctx.saved_tensors
        if gloss is None:
            return None, None, None, None
        return ops.sigmoid_ce_bwd(scores, labels, gloss.contiguous().float(), *ctx.targets), None, None, None


class ViTCELoss(hnn.Layer):
    """ViT style sigmoid cross entropy loss — reference passl/loss/celoss.py:58-95, returned as ``{"ViTCELoss": loss}``:
    binary cross entropy with logits against ``onehot * (1 - epsilon) + epsilon`` (the ViT style of label smoothing:
    epsilon is added to every class, not divided among them), summed over the classes, mean over the batch.  Integer
    labels only; ``type='softmax'`` is used by no recipe and is not built."""

    def __init__(self, epsilon=None, type='sigmoid'):
        super().__init__()
        assert type in ['sigmoid', 'softmax'], "type must be 'sigmoid' or 'softmax'."
        if type != 'sigmoid':
            raise NotImplementedError("ViTCELoss(type='softmax') is not built on the HIP path (no recipe uses it)")
        if epsilon is not None:
            assert epsilon >= 0 and epsilon <= 1, 'epsilon must be in [0, 1]'
        self.type = type
        self.epsilon = epsilon
        self.targets = ops.sigmoid_ce_targets(epsilon)

    def forward(self, x, label):
        if isinstance(x, dict):
            x = x['logits']
        x = x.float()
        if label.dim() > 1 and label.shape[-1] == x.shape[-1]:
            raise NotImplementedError('ViTCELoss on a dense [N, C] label is not built (integer class ids only)')
        loss = _SigmoidCEFn.apply(x, label.contiguous().long().view(-1), *self.targets)
        return {'ViTCELoss': loss.reshape(())}
