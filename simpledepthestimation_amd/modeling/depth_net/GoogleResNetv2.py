"""GoogleResNetv2 = bare-shortcut ResNet-18 encoder + transposed-convolution decoder + softplus (reference:
detectron2/modeling/depth_net/GoogleResNetv2.py:L80-215), the depth net of projects/MotionLearning/configs/resnet18_waymo.yaml.

The encoder is the ResNet skeleton GoogleResNet uses (layers/resnet_encoder.py, ``shortcut_norm=False``) under the v2 file's names; the decoder's five
UpsampleBlocks up-sample with ConvTranspose2d(3, stride 2, padding 1, output_padding 1) + ReLU (hip.nn.conv_transpose2d) instead of bilinear x2 + conv.
State-dict keys equal the reference's (``encoder.conv1.weight``, ``encoder.layer2.0.downsample.weight``, ``decoder.blocks.0.upconv.weight`` of shape
[512,256,3,3], ``decoder.out_conv.bias``, ``decoder.scale`` with LEARN_SCALE), so its checkpoints load with ``strict=True``.  Noise, flip, size checks
and the forward pass are GoogleResNet's (GoogleDepthNet).  The reference's max-pool shortcut (stride change at equal width, L56-57) never occurs in
ResNet-18 and is not built.
"""
from ...layers.google_resnet import GoogleDepthDecoderV2, GoogleResnetEncoderV2
from .build import DEPTH_NET_REGISTRY
from .GoogleResNet import GoogleDepthNet


@DEPTH_NET_REGISTRY.register()
class GoogleResNetv2(GoogleDepthNet):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        dn = cfg.MODEL.DEPTH_NET
        version = dn.ENCODER_NAME
        assert version is not None, "DispResNet needs a version"
        num_layers = int(str(version)[:2])       # the first two characters are the number of layers ("18??" in resnet18_waymo.yaml)
        assert num_layers in [18], "ResNet version {} not available".format(num_layers)
        norm_layer = self._configure(cfg)
        self.encoder = GoogleResnetEncoderV2(norm_layer)
        self.decoder = GoogleDepthDecoderV2(learn_scale=bool(dn.LEARN_SCALE))
        self._collect_norms()
        # inject_z speaks the reference's module names (``encoder.bn1``): drop the wrapper level, as the state dict does
        self._rand_norms = [(n.replace("encoder.encoder.", "encoder.", 1), m) for n, m in self._rand_norms]
