"""The CBAM attention tail through the layer API (reference models/resnet_v2_d_cbam.py:159-211): conv -> conv -> channel mask (shared MLP over the
[2N, C] mean / max rows) -> spatial mask -> add(skip) against torch-CPU float64 autograd (amax / mean split ties as TensorFlow does) — shared by
the GPU test (tests/test_gpu_cbam.py) and, run as a script with MCN_LIB_PATH naming libmcn_cpu.so, by tests/test_cbam_abi.py."""
import numpy as np


def _model(M, **kw):
    class Net(M.ConvNet):
        def _init_params(self, **kwargs):
            pass

        def _build_model(self):
            d = dict()
            self._curr_block = 0
            with self.variable_scope('block_0'):
                with self.variable_scope('c0'):
                    a = self.conv_layer(self.X, 3, 1, 16, biased=False)
                with self.variable_scope('c1'):
                    x = self.conv_layer(a, 1, 1, 16)
                with self.variable_scope('channel_mask'):
                    h = self.global_avgmax_pool(x)
                    with self.variable_scope('fc1'):
                        h = self.relu(self.fc_layer(h, 4))
                    with self.variable_scope('fc2'):
                        cm = self.pair_sigmoid(self.fc_layer(h, 16))
                x, d['spatial_mask'] = self.cbam_attention(x, cm, 7, scope='spatial_mask')
                x = self.stochastic_depth(x, a)
            d['block_0'] = x
            return d
    return Net([9, 11, 3], 10, batch_size=3, backbone_only=True, num_gpus=1, **kw)


def _reference(vals, x, dy=None):
    """float64 torch: output and spatial mask, and with dy the gradient of sum(out * dy) for every variable"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in vals.items()}
    p = 'block_0/'
    x0 = torch.tensor((x.astype(np.float64) - 0.5) * 2.0).permute(0, 3, 1, 2)
    a = F.conv2d(x0, t[p + 'c0/weights'].permute(3, 2, 0, 1), padding=1)
    u = F.conv2d(a, t[p + 'c1/weights'].permute(3, 2, 0, 1), t[p + 'c1/biases'])
    mlp = lambda v: F.relu(v @ t[p + 'channel_mask/fc1/weights'] + t[p + 'channel_mask/fc1/biases']) @ t[p + 'channel_mask/fc2/weights'] + t[p + 'channel_mask/fc2/biases']
    cm = torch.sigmoid(mlp(u.mean((2, 3))) + mlp(u.amax((2, 3))))
    xp = u * cm[:, :, None, None]
    s = torch.cat([xp.mean(1, keepdim=True), xp.amax(1, keepdim=True)], 1)
    sm = torch.sigmoid(F.conv2d(s, t[p + 'spatial_mask/conv/weights'].permute(3, 2, 0, 1), t[p + 'spatial_mask/conv/biases'], padding=3))
    out = (xp * sm + a).permute(0, 2, 3, 1)
    if dy is None:
        return out.detach().numpy(), sm.permute(0, 2, 3, 1).detach().numpy()
    (out * torch.tensor(dy.astype(np.float64))).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}


def run_case(M, check, **model_kw):
    import torch
    model = _model(M, **model_kw)
    names = [getattr(fn, '__name__', '') for fn, _ in model._train_low.fwd.calls]
    assert [n for n in names if 'cbam' in n or 'pool' in n or 'pair' in n] == ['mcn_global_avgmax_pool_fwd', 'mcn_pair_sigmoid_fwd', 'mcn_cbam_chpool_fwd', 'mcn_cbam_apply_fwd'], names
    assert names.count('mcn_fc_fwd') == 2 and 'mcn_channel_scale_fwd' not in names, names       # the shared MLP runs ONCE over both halves
    rng = np.random.default_rng(5)
    p = 'block_0/'
    shapes = {p + 'c0/weights': (3, 3, 3, 16), p + 'c1/weights': (1, 1, 16, 16), p + 'c1/biases': (16,), p + 'channel_mask/fc1/weights': (16, 4),
              p + 'channel_mask/fc1/biases': (4,), p + 'channel_mask/fc2/weights': (4, 16), p + 'channel_mask/fc2/biases': (16,),
              p + 'spatial_mask/conv/weights': (7, 7, 2, 1), p + 'spatial_mask/conv/biases': (1,)}
    assert {k: v.shape for k, v in model.variables.items()} == shapes
    draw = lambda: {k: (rng.standard_normal(s) * (0.5 if len(s) == 1 else 0.3)).astype(np.float32) for k, s in shapes.items()}
    ema, vals = draw(), draw()
    model.set_variables(ema)                            # EMA shadows := ema ...
    model.set_variables(vals, reset_state=False)        # ... masters := vals
    x = rng.random((3, 9, 11, 3)).astype(np.float32)
    dy = rng.standard_normal((3, 9, 11, 16)).astype(np.float32)
    model.feed(x, np.zeros(3, np.float32))
    out = model.d['block_0']
    ref, grads_ref = _reference(vals, x, dy)
    model.forward(train=True)
    check(model.fetch(out), ref, 'float32', 'cbam net forward')
    out.grad.copy_(torch.as_tensor(dy).to(out.grad.device))
    model.backward()
    grads = model.get_variables('grad')
    for k in shapes:
        check(grads[k], grads_ref[k], 'float32', 'gradient of ' + k, rel=1e-4)
    model.forward(train=False)                          # inference: the same kernels on the EMA shadows
    ref, sm_ref = _reference(ema, x)
    check(model.fetch(out), ref, 'float32', 'cbam net inference')
    check(model.fetch(model.d['spatial_mask']), sm_ref, 'float32', 'spatial mask (inference)')


if __name__ == '__main__':
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import myconvnet_amd as M
    from myconvnet_amd import _ffi
    from test_gpu_ops import check
    assert _ffi.IS_CPU_LIB, 'run with MCN_LIB_PATH=<repo>/myconvnet_amd/libmcn_cpu.so'
    run_case(M, check, device='cpu')
    print('cbam layer case ok')
