from .mixup import Mixup, build_mixup
