"""Global-norm gradient clipping as CONFIGURATION (passl/core/grad_clip.py:30-139 restated).

The reference's ``ClipGradByGlobalNorm`` is a callable that its optimizers run once per parameter group
(passl/optimizer/adamw.py:53-55): it sums the squared gradients of the group's parameters, and scales the gradients in
place when the norm exceeds ``clip_norm``.  Here the object only carries the numbers: AdamW (solver/optimizer.py) turns it
into a chunk table once and runs the rule on the device every step (hip/ops.py grad_sumsq / grad_clip_finalize and the
clip variants of the update) — the norm never reaches the host.  For one set S of parameters

    norm(S) = sqrt(sum over S of (g * grad_scale)^2)                                    (fp32, one fixed order)
    coef(S) = 1                                                if not always_clip and norm <= clip_norm
            = min(clip_norm / (norm + 1e-6), clip_norm_max or inf)   otherwise

and the update uses (g * grad_scale) * coef.  A non-finite norm gets no special case: it is "not <=" and its coefficient
propagates, as in the reference.  ``param.grad`` is NOT rewritten (the reference scales it in place).

``scope`` chooses the sets: 'group' (the reference's optimizers: one set per parameter group handed to the optimizer, a
plain parameter list being one group) or 'global' (one set over every listed parameter: what ``clip_grad_norm_(model.
parameters(), max_norm)`` in front of a grouped optimizer does, tasks/ssl/mae/main_finetune.py --clip_grad).  A parameter
whose Paddle auto-name contains an entry of ``no_clip_list``, or with ``need_clip = False``, is in no set."""
import math

SCOPES = ('group', 'global')


class ClipGradByGlobalNorm(object):
    def __init__(self, clip_norm=1.0, clip_norm_max=None, always_clip=False, no_clip_list=[], scope='group'):
        clip_norm = float(clip_norm)
        if not (clip_norm > 0 and math.isfinite(clip_norm)):
            raise ValueError('clip_norm must be a positive finite number, got %r' % (clip_norm,))
        if clip_norm_max is not None:
            clip_norm_max = float(clip_norm_max)
            if not clip_norm_max > 0:
                raise ValueError('clip_norm_max must be positive (or None), got %r' % (clip_norm_max,))
        if scope not in SCOPES:
            raise ValueError('scope must be one of %r, got %r' % (SCOPES, scope))
        if isinstance(no_clip_list, str):
            raise ValueError('no_clip_list is a list of name fragments, got the string %r' % (no_clip_list,))
        self.clip_norm = clip_norm
        self.clip_norm_max = clip_norm_max
        self.always_clip = bool(always_clip)
        self.no_clip_list = [str(n) for n in no_clip_list]
        self.scope = scope

    @classmethod
    def like_clip_grad_norm_(cls, max_norm, no_clip_list=[]):
        """``clip_grad_norm_(parameters, max_norm)`` (grad_clip.py:95-139: coef = clip(max_norm / (norm + 1e-6), max=1)
        over all parameters together, applied whatever the norm) is the same rule with always_clip, clip_norm_max = 1
        and the global scope."""
        return cls(clip_norm=max_norm, clip_norm_max=1.0, always_clip=True, no_clip_list=no_clip_list, scope='global')

    def excludes(self, param, name):
        """Is ``param`` (Paddle auto-name ``name``) left out of every norm?"""
        return getattr(param, 'need_clip', True) is False or any(n in name for n in self.no_clip_list)

    def __repr__(self):
        return ('ClipGradByGlobalNorm(clip_norm=%r, clip_norm_max=%r, always_clip=%r, no_clip_list=%r, scope=%r)'
                % (self.clip_norm, self.clip_norm_max, self.always_clip, self.no_clip_list, self.scope))


GRAD_CLIPS = {'ClipGradByGlobalNorm': ClipGradByGlobalNorm}


def build_grad_clip(cfg):
    """{name: ClipGradByGlobalNorm, clip_norm: ...} -> the object (passl/optimizer/__init__.py:130-133: ``name``
    defaults to ClipGradByGlobalNorm)."""
    cfg = dict(cfg)
    name = cfg.pop('name', 'ClipGradByGlobalNorm')
    if name not in GRAD_CLIPS:
        raise NotImplementedError('grad_clip %r is not built (known: %s)' % (name, ', '.join(sorted(GRAD_CLIPS))))
    return GRAD_CLIPS[name](**cfg)
