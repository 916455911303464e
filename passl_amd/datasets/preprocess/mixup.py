"""Mixup / CutMix of a device-resident batch — reference passl_v110/datasets/preprocess/mixup.py:108-276 (class Mixup,
after timm) and build_mixup, passl_v110/datasets/preprocess/builder.py:37-57.

The reference mixes on the host (framework CPU tensors; a Python loop builds the one-hot matrix row by row).  Here a
step is two launches of csrc/mixup.hip — ``ops.batch_mix`` and ``ops.mixup_target`` — and no host tensor work: the
parameters (mix or not, mixup or CutMix, lambda, the box) are drawn on the host from numpy IN THE REFERENCE'S ORDER
(_params_per_batch :183-199, rand_bbox :40-61, cutmix_bbox_and_lam :91-105) and travel as plain kernel arguments, so
with equal seeds this class and the reference's mix identically.

Where the reference's class does not run, this one does something defined:
  * ``mode='elem'`` / ``mode='pair'`` raise ValueError in the reference (``x, lam = self._mix_elem(x)`` unpacks a
    [B, 1] tensor): NotImplementedError here, as is ``cutmix_minmax``.
  * ``prob < 1``: the reference raises TypeError on every step that draws no mixing (``_mix_batch`` returns the float
    ``1.``).  Here such a step returns ``x`` itself and the smoothed one-hot target (lam = 1).
  * An odd batch is refused as in mixup.py:267.
The input batch is never written (the synthetic loaders reuse their resident batches): the mixed batch is a new tensor."""
import numpy as np
import torch

from ...hip import ops


class Mixup:
    """``rng``: a ``numpy.random.RandomState``; None = the global ``numpy.random``, which is what the reference uses."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, rng=None):
        if cutmix_minmax is not None:
            raise NotImplementedError('Mixup(cutmix_minmax=...) is not built: use cutmix_alpha')
        if mode != 'batch':
            raise NotImplementedError("Mixup(mode=%r): only 'batch' is built (the reference's 'elem' / 'pair' raise "
                                      'ValueError in __call__)' % (mode,))
        if not (mixup_alpha > 0. or cutmix_alpha > 0.):
            raise ValueError('one of mixup_alpha > 0., cutmix_alpha > 0. should be true')
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = None
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True          # set to False to disable mixing (mixup.py:151)
        self.rng = rng

    def draw(self, img_shape):
        """The parameters of one step, drawn on the host without touching a device: ``(use_cutmix, lam, box)``;
        ``box`` = (yl, yh, xl, xh) for CutMix, else None; ``lam`` (a Python float) is already corrected to the clipped
        box.  An unmixed step (``prob`` < 1 or ``mixup_enabled`` False) is ``(False, 1.0, None)``.  The order of the
        draws is the reference's: rand() < prob; rand() < switch_prob; beta(a, a); randint(0, H); randint(0, W)."""
        rng = np.random if self.rng is None else self.rng
        lam, use_cutmix = 1., False
        if self.mixup_enabled and rng.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = bool(rng.rand() < self.switch_prob)
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = rng.beta(self.mixup_alpha, self.mixup_alpha)
            else:
                use_cutmix = True
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam_mix)
        if lam == 1.:
            return False, 1., None
        if not use_cutmix:
            return False, lam, None
        img_h, img_w = img_shape[-2:]
        ratio = np.sqrt(1 - lam)
        cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
        cy = rng.randint(0, img_h)
        cx = rng.randint(0, img_w)
        yl = int(np.clip(cy - cut_h // 2, 0, img_h))
        yh = int(np.clip(cy + cut_h // 2, 0, img_h))
        xl = int(np.clip(cx - cut_w // 2, 0, img_w))
        xh = int(np.clip(cx + cut_w // 2, 0, img_w))
        if self.correct_lam:
            lam = float(1. - (yh - yl) * (xh - xl) / float(img_h * img_w))
        return True, lam, (yl, yh, xl, xh)

    def __call__(self, x, target):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        use_cutmix, lam, box = self.draw(x.shape)
        labels = target.contiguous().long().view(-1)
        if lam == 1. and box is None:
            return x, ops.mixup_target(labels, self.num_classes, 1., self.label_smoothing)
        x = ops.batch_mix(x.contiguous(), lam, box)
        return x, ops.mixup_target(labels, self.num_classes, lam, self.label_smoothing)


def build_mixup(cfg):
    """``dataset.batch_transforms`` -> Mixup or None (reference build_mixup, preprocess/builder.py:37-57: the first
    entry of the list; active when mixup_alpha > 0 or cutmix_alpha > 0).  Unlike the reference's builder, which drops
    them and so always mixes with label_smoothing 0.1 over 1000 classes, ``label_smoothing`` / ``num_classes`` /
    ``correct_lam`` of the block are passed on when given."""
    if not cfg:
        return None
    cfg = dict(cfg[0])
    name = cfg.pop('name', 'Mixup')
    if name == 'LVViTMixup':
        raise NotImplementedError('LVViTMixup (token labelling) is not built')
    if name != 'Mixup':
        raise KeyError('unknown batch transform %r' % (name,))
    if cfg.get('cutmix_minmax', '') in ('', None):
        cfg.pop('cutmix_minmax', None)
    if not (cfg.get('mixup_alpha', 0.) > 0 or cfg.get('cutmix_alpha', 0.) > 0. or 'cutmix_minmax' in cfg):
        return None
    return Mixup(**cfg)
