from .builder import BACKBONES, build_backbone
from .resnet import ResNet, BottleneckBlock
from .resnetsimclr import ResNetsimclr, ResNetCifar
from .mae import MAE, MAE_ViT
from .vision_transformer import VisionTransformer
from .clip import CLIP
from .convmae import ConvMAE            # (last: imports passl_amd.models.convmae, which imports this package's builder)
