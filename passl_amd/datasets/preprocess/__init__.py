from .mixup import Mixup, build_mixup
from .random_erasing import RandomErasing, build_random_erasing
from .crop import (DeviceCropPipeline, MAERandCropImage, NormalizeImage, RandCropImage, RandFlipImage,
                   RandomHorizontalFlip, ToCHWImage, build_crop_pipeline)
