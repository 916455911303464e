"""Restatement of what csrc/mixup.hip computes, in numpy / torch on the CPU — shared by tests/test_mixup_host.py,
tests/test_mixup_gpu.py and tests/golden/make_golden_mixup.py (which checks it bit for bit against the reference's
Mixup before it writes a fixture)."""
import numpy as np
import torch

# the recipe block of configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml
RECIPE = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1., switch_prob=0.5, mode='batch')
PARAM_SEEDS = list(range(12))
SECOND_CALL_SEEDS = [0, 2]                 # two consecutive calls on one stream are recorded for these
FT_SEEDS = [0, 2]                          # step 0 mixes under numpy seed 0 (mixup), step 1 under seed 2 (CutMix)
FT_TOL_F32 = dict(loss=1e-3, feat=1e-3, grad=2e-3, param=1e-4)              # tests/test_mae_gpu.py, unchanged
FT_TOL_BF16 = dict(loss=3e-2, feat=6e-2, grad=8e-2, param=1e-2)


def batch_mix_ref(x, lam=1.0, box=None):
    """fp32 NCHW torch CPU tensor -> mixed copy.  Mixup: fl(fl(x * f32(lam)) + fl(x.flip(0) * f32(1 - lam))), the
    subtraction in double (torch rounds a Python scalar to the tensor's dtype before an elementwise product, and its
    CPU kernels do not contract the two products and the sum).  CutMix: x.flip(0) inside the box."""
    assert x.dtype == torch.float32
    if box is not None:
        yl, yh, xl, xh = box
        out = x.clone()
        out[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        return out
    a = torch.tensor(np.float32(lam))
    b = torch.tensor(np.float32(1.0 - float(lam)))
    return x * a + x.flip(0) * b


def mixup_target_ref(labels, num_classes, lam=1.0, eps=0.0):
    """mixup_target of the reference in float64 (numpy int labels [N] -> [N, C])."""
    labels = np.asarray(labels)
    off = eps / num_classes
    on = 1. - eps + off
    y1 = np.full((len(labels), num_classes), off)
    y2 = np.full((len(labels), num_classes), off)
    y1[np.arange(len(labels)), labels] = on
    y2[np.arange(len(labels)), labels[::-1]] = on
    return y1 * lam + y2 * (1. - lam)


def soft_ce_ref(scores, target):
    """float64 torch on the CPU: (loss, acc1, acc5, dscores for d loss = 1); accuracy against the first arg-max of the
    target, ranks counted as csrc/clas.hip does (ties resolve to the lower index)."""
    s = scores.detach().double().cpu().requires_grad_(True)
    t = target.detach().double().cpu()
    loss = torch.sum(-t * torch.log_softmax(s, dim=-1), dim=-1).mean()
    loss.backward()
    sn, tn = s.detach().numpy(), t.numpy()
    lab = tn.argmax(axis=1)                                  # numpy: the first maximum
    sl = sn[np.arange(len(lab)), lab][:, None]
    j = np.arange(sn.shape[1])[None, :]
    rank = ((sn > sl) | ((sn == sl) & (j < lab[:, None]))).sum(axis=1)
    return float(loss.detach()), 100.0 * float((rank < 1).mean()), 100.0 * float((rank < 5).mean()), s.grad
