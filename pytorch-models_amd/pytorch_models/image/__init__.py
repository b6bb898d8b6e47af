from .convnext import ConvNeXt
from .detr import DETR, DETRPipeline
from .maxvit import MaxViT
from .mobile_vit import MobileViT
from .vit import ViT
