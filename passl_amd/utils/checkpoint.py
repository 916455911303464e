"""Checkpoint / weight-exchange helpers.

File format = a pickled dict of numpy arrays, the layout of the reference's ``save`` helper
(passl_v110/hooks/checkpoint_hook.py:23-50) and of ``paddle.save`` for a dygraph ``state_dict``
(which adds the bookkeeping key ``StructuredToParameterName@@``  [Paddle-semantics]).  Because
``state_dict()`` here uses the reference's key names and logical shapes, a published ``.pdparams``
loads without any transposition."""
import os
import pickle

import numpy as np
import torch

PADDLE_META_KEYS = ('StructuredToParameterName@@',)


def load_pickle(path):
    with open(path, 'rb') as f:
        obj = pickle.load(f, encoding='latin1')
    if isinstance(obj, dict):
        for k in PADDLE_META_KEYS:
            obj.pop(k, None)
    return obj


def to_numpy(obj):
    if torch.is_tensor(obj):
        t = obj.detach().cpu()
        return t.float().contiguous().numpy() if t.is_floating_point() else t.numpy()
    if isinstance(obj, dict):
        return {k: to_numpy(v) for k, v in obj.items()}
    return obj


def to_tensors(sd):
    return {k: torch.as_tensor(np.asarray(v)) if isinstance(v, (np.ndarray, np.generic)) else v
            for k, v in sd.items()}


def load_state_into(model, state_dict, strict=False):
    """state_dict: name -> numpy array (or tensor).  A bare backbone dict (as written by
    tools/extract_weight.py --remove_prefix) can be loaded into ``model.backbone``."""
    sd = to_tensors(state_dict)
    return model.load_state_dict(sd, strict=strict)


def load_lenient(module, state_dict, logger=None, what='weights'):
    """Paddle's ``set_state_dict`` policy: load what matches, WARN per missing / unexpected key, and
    refuse a file in which nothing matched (a wrong key prefix would otherwise "load" successfully and
    leave the model on its random init)."""
    import logging
    logger = logger or logging.getLogger('passl')
    sd = to_tensors(state_dict)
    own = module.state_dict()
    matched = [k for k in sd if k in own]
    if own and not matched:
        raise ValueError('%s: none of the %d keys matches the model (first file key %r, first model '
                         'key %r) - wrong prefix?' % (what, len(sd), next(iter(sd), None),
                                                      next(iter(own), None)))
    res = module.load_state_dict(sd, strict=False)
    for k in res.missing_keys:
        logger.warning('%s: %s is not found in the provided dict.' % (what, k))
    for k in res.unexpected_keys:
        logger.warning('%s: skip loading for %s (not in the model).' % (what, k))
    return res


def dump_pdparams(state, path):
    """``state``: name -> numpy array, written as ``<path>.pdparams`` (pickle protocol 2, as paddle.save does)."""
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path + '.pdparams', 'wb') as f:
        pickle.dump(state, f, protocol=2)


def save_pdparams(model, path, rank=0):
    """``Model.save``: rank 0 writes ``model.state_dict()`` to ``<path>.pdparams``.  -> the written dict (None on the
    other ranks), for the models that write a second file from it."""
    if rank != 0:
        return None
    state = to_numpy(dict(model.state_dict()))
    dump_pdparams(state, path)
    return state


def read_pdparams(path, bare_ok=False):
    """``Model.load_pretrained``'s file: ``<path>.pdparams`` as in the reference; with ``bare_ok`` a ``path`` that
    exists is taken as it is (a v110 checkpoint or an extracted-weights file given with its extension)."""
    fn = path if bare_ok and os.path.exists(path) else path + '.pdparams'
    if not os.path.exists(fn):
        raise ValueError('Model pretrain path {} does not exists.'.format(fn if bare_ok else path))
    return load_pickle(fn)


def load_pdparams(model, path, what='pretrained model', bare_ok=False):
    """read_pdparams + load_lenient, then ``model.sync_runtime_state()`` where the model has one (flat arenas that mirror
    the parameters)."""
    res = load_lenient(model, read_pdparams(path, bare_ok), what=what)
    sync = getattr(model, 'sync_runtime_state', None)
    if sync is not None:
        sync()
    return res
