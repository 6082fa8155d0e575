"""ResNet with Convolutional Block Attention Modules (reference models/resnet_v2_d_cbam.py; https://arxiv.org/abs/1807.06521).

ResNet-v2-D — three 3x3 stem convolutions, pre-activation batch norm, average-pool shortcuts, biased 1x1 projections — with a CBAM
behind every residual unit, under the reference's scope and variable names ('block_1/res_0/channel_mask/fc1/weights',
'.../spatial_mask/conv/weights', '.../spatial_mask/conv/biases', ...).  The raw TF calls of the model file are the stand-ins of
ConvNet: global_avgmax_pool (the two reduce ops of _channel_mask as one [2N, C] tensor, so that the fc layers shared through
reuse_variables() run once over both halves), pair_sigmoid, and cbam_attention (x * channel_mask * spatial_mask with the product never
stored).  Not built: feature_reduction (the experimental 'comp' layer) and the dilated variant.
"""
from .convnet import ConvNet


class ResNetCBAM(ConvNet):
    def _init_params(self, **kwargs):
        self.channels = [64, 256, 512, 1024, 2048]
        self.kernels = [3, 3, 3, 3, 3]
        self.strides = [2, 1, 2, 2, 2]
        self.res_units = [None, 3, 4, 6, 3]

        self.cam_ratio = 8
        self.sam_kernel = 7

        self.block_activations = False

        self.initial_drop_rate = kwargs.get('initial_drop_rate', 0.0)
        self.final_drop_rate = kwargs.get('final_drop_rate', 0.0)

    def _build_model(self):
        d = dict()
        channels, kernels, strides, res_units = self.channels, self.kernels, self.strides, self.res_units
        num_blocks = min(len(channels), len(kernels), len(strides), len(res_units))

        self._curr_block = 0
        x = self.X
        with self.variable_scope('block_0'):
            for j, (s, c) in enumerate([(strides[0], channels[0] // 2), (1, channels[0] // 2), (1, channels[0])]):
                scope = 'conv_{}'.format(j)
                with self.variable_scope(scope):
                    x = self.conv_layer(x, kernels[0], s, c, padding='SAME', biased=False)
                    d['block_0/' + scope] = x
                    x = self.batch_norm(x, shift=True, scale=True, scope='bn')
                    d['block_0/' + scope + '/bn'] = x
                    x = self.relu(x, name='relu')
                    d['block_0/' + scope + '/relu'] = x
            d['block_-1'] = x
            x = self.max_pool(x, 3, 2, padding='SAME')
            d['block_0'] = x

        for i in range(1, num_blocks):
            self._curr_block = i
            dr = self.initial_drop_rate + (self.final_drop_rate - self.initial_drop_rate) * i / (num_blocks - 1)
            for j in range(res_units[i]):
                x = self._res_unit(x, kernels[i], strides[i] if j == 0 else 1, channels[i], d, drop_rate=dr, name='block_{}/res_{}'.format(i, j))
            if self.block_activations:
                with self.variable_scope('block_{}/act'.format(i)):
                    x = self.batch_norm(x, shift=True, scale=True, scope='bn')
                    x = self.relu(x, name='relu')
            d['block_{}'.format(i)] = x

        if self.backbone_only is False:
            if self.feature_reduction > 1:
                raise NotImplementedError('feature_reduction (the experimental compression layer) is outside the built path')
            self._curr_block = None
            with self.variable_scope('block_None'):
                with self.variable_scope('logits'):
                    if not self.block_activations:
                        x = self.batch_norm(x, shift=True, scale=True, scope='bn')
                        d['logits/bn'] = x
                        x = self.relu(x, name='relu')
                        d['logits/relu'] = x
                    x = self.global_avg_pool(x)
                    d['logits/avgpool'] = x
                    x = self.dropout(x, rate=self.dropout_rate_features)
                    x = self.fc_layer(x, self.num_classes)
                    d['logits'] = x
                    d['pred'] = self.softmax(x)
        return d

    def _res_unit(self, x, kernel, stride, out_channels, d, drop_rate=0.0, name='res_unit'):
        in_channels = x.shape[-1]
        if not isinstance(stride, (list, tuple)):
            stride = [stride, stride]
        elif len(stride) == 1:
            stride = [stride[0], stride[0]]

        with self.variable_scope(name):
            skip = self.avg_pool(x, stride, stride, 'SAME') if (stride[0] > 1 or stride[1] > 1) else x
            if in_channels != out_channels:
                with self.variable_scope('conv_skip'):
                    skip = self.conv_layer(skip, 1, 1, out_channels, padding='SAME')
            d[name + '/branch'] = skip

            with self.variable_scope('conv_0'):
                x = self.batch_norm(x, shift=True, scale=True, scope='bn')
                d[name + '/conv_0/bn'] = x
                x = self.conv_layer(x, 1, 1, out_channels // 4, padding='SAME', biased=False)
                d[name + '/conv_0'] = x

            with self.variable_scope('conv_1'):
                x = self.batch_norm(x, shift=True, scale=True, scope='bn')
                d[name + '/conv_1/bn'] = x
                x = self.relu(x, name='relu')
                d[name + '/conv_1/relu'] = x
                x = self.conv_layer(x, kernel, stride, out_channels // 4, padding='SAME', biased=False)
                d[name + '/conv_1'] = x

            with self.variable_scope('conv_2'):
                x = self.batch_norm(x, shift=True, scale=True, zero_scale_init=True, scope='bn')
                d[name + '/conv_2/bn'] = x
                x = self.relu(x, name='relu')
                d[name + '/conv_2/relu'] = x
                x = self.conv_layer(x, 1, 1, out_channels, padding='SAME')
                d[name + '/conv_2'] = x

            channel_mask = self._channel_mask(x, self.cam_ratio, name='channel_mask')
            d[name + '/channel_mask'] = channel_mask
            x, spatial_mask = self.cbam_attention(x, channel_mask, self.sam_kernel, scope='spatial_mask')
            d[name + '/spatial_mask'] = spatial_mask

            x = self.stochastic_depth(x, skip, drop_rate=drop_rate)
            d[name] = x
        return x

    def _channel_mask(self, x, reduction, name='channel_mask'):
        in_channels = x.shape[-1]
        with self.variable_scope(name):
            pools = self.global_avgmax_pool(x)                   # [2N, C]: spatial_mean rows, then spatial_max rows
            with self.variable_scope('fc1'):
                h = self.fc_layer(pools, in_channels // reduction)
            h = self.relu(h, name='relu')
            with self.variable_scope('fc2'):
                h = self.fc_layer(h, in_channels)
            return self.pair_sigmoid(h)


class ResNetCBAM50(ResNetCBAM):
    def _init_params(self, **kwargs):
        super()._init_params(**kwargs)
        self.res_units = [None, 3, 4, 6, 3]


class ResNetCBAM101(ResNetCBAM):
    def _init_params(self, **kwargs):
        super()._init_params(**kwargs)
        self.res_units = [None, 3, 4, 23, 3]
