"""CELoss — reference passl/loss/celoss.py:22-56, returned as ``{"CELoss": loss}``.

Integer labels without ``epsilon``: mean softmax cross entropy, one kernel (csrc/clas.hip: row log-sum-exp, the label's
score and the top-1 / top-5 ranks in one pass; backward = softmax - one_hot scaled by the incoming gradient).
``epsilon`` (label smoothing, celoss.py:30-46): the smoothed target (1 - eps) onehot + eps / C comes from
``ops.mixup_target`` with lam = 1 for integer labels, or is (1 - eps) t + eps / C of a given soft label; then the
soft-target cross-entropy of csrc/mixup.hip.  A soft label [N, C] without ``epsilon`` (mixup / cutmix targets, :48-49)
goes to that kernel as it is.  tasks/ssl/mae/util/loss.py's LabelSmoothingCrossEntropy is the same number as
``CELoss(epsilon)`` and SoftTargetCrossEntropy the same as ``CELoss()`` on a soft label."""
import torch

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
