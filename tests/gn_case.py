"""ConvNet.group_norm through the layer API (reference convnet.py:1928-2013): conv -> gn -> relu -> conv -> gn -> add(first block) -> relu against
torch-CPU float64 autograd (F.conv2d + F.group_norm) — shared by the GPU test (tests/test_gpu_gn.py) and, run as a script with MCN_LIB_PATH naming
libmcn_cpu.so, by the host-code case of tests/test_gn_abi.py."""
import numpy as np


def _model(M, **kw):
    class Net(M.ConvNet):
        def _init_params(self, **kwargs):
            pass

        def _build_model(self):
            d = dict()
            self._curr_block = 0
            with self.variable_scope('block_0'):
                with self.variable_scope('u1'):
                    x = self.conv_layer(self.X, 3, 1, 16, biased=False)
                    x = self.group_norm(x, num_groups=8)
                    a = self.relu(x)
                with self.variable_scope('u2'):
                    x = self.conv_layer(a, 3, 1, 16)
                    x = self.group_norm(x, num_groups=4)
                    x = self.stochastic_depth(x, a)
                    x = self.relu(x)
            d['block_0'] = x
            return d
    return Net([9, 11, 3], 10, batch_size=3, backbone_only=True, num_gpus=1, **kw)


def _reference(vals, x, dy=None):
    """float64 torch: output, and with dy the gradient of sum(out * dy) for every variable"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in vals.items()}
    conv = lambda a, w, b=None: F.conv2d(a, w.permute(3, 2, 0, 1), b, padding=1)
    x0 = torch.tensor((x.astype(np.float64) - 0.5) * 2.0).permute(0, 3, 1, 2)
    a = F.relu(F.group_norm(conv(x0, t['block_0/u1/weights']), 8, t['block_0/u1/gn/gamma'], t['block_0/u1/gn/beta'], eps=1e-3))
    u = F.group_norm(conv(a, t['block_0/u2/weights'], t['block_0/u2/biases']), 4, t['block_0/u2/gn/gamma'], t['block_0/u2/gn/beta'], eps=1e-3)
    out = F.relu(u + a).permute(0, 2, 3, 1)
    if dy is None:
        return out.detach().numpy()
    (out * torch.tensor(dy.astype(np.float64))).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}


def run_case(M, check, **model_kw):
    import torch
    model = _model(M, **model_kw)
    names = [getattr(fn, '__name__', '') for fn, _ in model._train_low.fwd.calls]
    assert names.count('mcn_gn_fwd') == 2 and not {'mcn_relu_fwd', 'mcn_add_relu_fwd', 'mcn_act_fwd_p'} & set(names), names
    rng = np.random.default_rng(11)
    shapes = {'block_0/u1/weights': (3, 3, 3, 16), 'block_0/u1/gn/gamma': (16,), 'block_0/u1/gn/beta': (16,), 'block_0/u2/weights': (3, 3, 16, 16),
              'block_0/u2/biases': (16,), 'block_0/u2/gn/gamma': (16,), 'block_0/u2/gn/beta': (16,)}
    assert {k: v.shape for k, v in model.variables.items()} == shapes
    draw = lambda: {k: ((0.5 + rng.random(s)) if k.endswith('gamma') else rng.standard_normal(s) * (0.3 if len(s) == 4 else 0.5)).astype(np.float32)
                    for k, s in shapes.items()}
    ema, vals = draw(), draw()
    model.set_variables(ema)                            # EMA shadows := ema ...
    model.set_variables(vals, reset_state=False)        # ... masters := vals
    x = rng.random((3, 9, 11, 3)).astype(np.float32)
    dy = rng.standard_normal((3, 9, 11, 16)).astype(np.float32)
    model.feed(x, np.zeros(3, np.float32))
    out = model.d['block_0']
    ref, grads_ref = _reference(vals, x, dy)
    model.forward(train=True)
    check(model.fetch(out), ref, 'float32', 'gn net forward')
    out.grad.copy_(torch.as_tensor(dy).to(out.grad.device))
    model.backward()
    grads = model.get_variables('grad')
    for k in shapes:
        check(grads[k], grads_ref[k], 'float32', 'gradient of ' + k, rel=1e-4)
    model.forward(train=False)                          # inference: same kernel, EMA shadows of gamma / beta (and of the conv weights)
    check(model.fetch(out), _reference(ema, x), 'float32', 'gn net inference')


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
    print('group norm layer case ok')
