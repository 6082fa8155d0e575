"""ResNet v1.5 with weight standardisation and group normalisation (reference models/resnet_v1_5_wsgn.py:5-160).

The bottleneck network of resnet_v1_5.py / resnet_v1_5_dilated.py with every convolution standardised (conv_layer(ws=True,
biased=False): mcn_ws_* in front of the per-use cast) and every norm a 32-group group norm under the scope 'bn' (the reference keeps
the batch-norm scope name, so 'block_1/res_0/conv_1/bn/gamma' addresses the same parameter); zero-initialised gamma on the last norm of
a unit, 1x1/stride projection shortcut when the width changes, VALID max-pool shortcut otherwise, per-stage dilation with the
multi-grid factors.  group_norm is called directly: normalization(norm_type='group') is not dispatched (convnet.py).  The class names
are the reference's and clash with the batch-norm family's, so the package exports this module, not its classes.
"""
from .resnet_v1_5_dilated import ResNetDilated

NUM_GROUPS = 32


class ResNet(ResNetDilated):
    """Base model: ResNet-50 layout, no dilation."""

    def _init_params(self, **kwargs):
        super()._init_params(**kwargs)
        self.dilations = [None, 1, 1, 1, 1]

    def conv_layer(self, x, kernel, stride, out_channels=None, **kw):
        """every convolution of the family is standardised (models/resnet_v1_5_wsgn.py:41, 102-126); the logits stay an fc_layer"""
        kw.setdefault('ws', True)
        return super().conv_layer(x, kernel, stride, out_channels, **kw)

    def _norm(self, x, **kw):
        return self.group_norm(x, num_groups=NUM_GROUPS, shift=True, scale=True, scope='bn', **kw)


class ResNet50(ResNet):
    pass


class ResNet101(ResNet):
    def _init_params(self, **kwargs):
        super()._init_params(**kwargs)
        self.res_units = [None, 3, 4, 23, 3]


class ResNet50OS16(ResNet):
    def _init_params(self, **kwargs):
        super()._init_params(**kwargs)
        self.dilations = [None, 1, 1, 1, 2]


class ResNet101OS16(ResNet):
    def _init_params(self, **kwargs):
        super()._init_params(**kwargs)
        self.res_units = [None, 3, 4, 23, 3]
        self.dilations = [None, 1, 1, 1, 2]
