"""``passl.models.convmae`` — ConvMAE (reference passl/models/convmae/__init__.py:15-16)."""
from .conv_mae import *        # noqa: F401,F403
from .conv_vit import *        # noqa: F401,F403
