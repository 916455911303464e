from .mixup import Mixup, build_mixup
from .random_erasing import RandomErasing, build_random_erasing
