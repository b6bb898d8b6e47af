from .convnext import ConvNeXt
from .maxvit import MaxViT
from .mobile_vit import MobileViT
from .vit import ViT
