from .mixup import Mixup, build_mixup
from .random_erasing import RandomErasing, build_random_erasing
from .crop import (DeviceCropPipeline, MAERandCropImage, NormalizeImage, RandCropImage, RandFlipImage,
                   RandomHorizontalFlip, ToCHWImage, build_crop_pipeline)
from .view_aug import (BYOLSolarize, ColorJitter, DeviceViewPipeline, GaussianBlur, RandomApply, RandomGrayscale,
                       SimCLRGaussianBlur, TwoViewsTransform, build_two_views, build_view_pipeline)
