from .fpn import FPN, LastLevelP6, LastLevelP6P7
from .vovnet import VoVNet, build_fcos_vovnet_fpn_backbone, build_vovnet_backbone
from .mobilenet import MobileNetV2, build_fcos_mobilenetv2_fpn_backbone, build_mnv2_backbone, build_mobilenetv2_fpn_backbone
from .resnet import ResNet, build_fcos_resnet_fpn_backbone, build_resnet_backbone, build_resnet_fpn_backbone
