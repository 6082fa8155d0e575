"""conv_layer(ws=True) through the layer API (reference convnet.py:1410-1419): conv 3x3 (ws) -> gn -> relu -> conv 1x1 (ws) -> gn -> add -> relu against torch-CPU
float64 autograd with the standardisation written out — shared by the GPU test (tests/test_gpu_ws.py) and, run as a script with MCN_LIB_PATH naming
libmcn_cpu.so, by the host-code case of tests/test_ws_abi.py."""
import numpy as np

SHAPES = {'block_0/u1/weights': (3, 3, 3, 16), 'block_0/u1/gn/gamma': (16,), 'block_0/u1/gn/beta': (16,), 'block_0/u2/weights': (1, 1, 16, 16),
          'block_0/u2/gn/gamma': (16,), 'block_0/u2/gn/beta': (16,)}


def _model(M, **kw):
    class Net(M.ConvNet):
        def _build_model(self):
            self._curr_block = 0
            with self.variable_scope('block_0'):
                with self.variable_scope('u1'):
                    x = self.conv_layer(self.X, 3, 1, 16, biased=False, ws=True)
                    x = self.group_norm(x, num_groups=8)
                    a = self.relu(x)
                with self.variable_scope('u2'):
                    x = self.conv_layer(a, 1, 1, 16, biased=False, ws=True)
                    x = self.group_norm(x, num_groups=4)
                    x = self.stochastic_depth(x, a)
                    x = self.relu(x)
            return {'a': a, 'block_0': x}
    return Net([9, 11, 3], 10, batch_size=3, backbone_only=True, num_gpus=1, **kw)


def _reference(vals, x, dtype, dy=None, masks=None):
    """float64 torch: output, and with dy the gradient of sum(out * dy) for every variable.  A 2-byte run rounds w_hat (not w) to the storage type.  `masks`: the
    ReLU decisions the device stored (NHWC booleans), so that an activation within rounding of zero cannot turn into a gradient error (as tests/test_gpu_gn.py)"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in vals.items()}

    def std_w(w):
        d = w - w.mean(dim=(0, 1, 2), keepdim=True)
        wh = d / (d.pow(2).mean(dim=(0, 1, 2), keepdim=True).sqrt() + 1e-5)
        if dtype != 'float32':                              # straight-through rounding: the value the conv reads, the gradient of the fp32 expression
            wh = wh + (wh.detach().to(getattr(torch, dtype)).double() - wh.detach())
        return wh.permute(3, 2, 0, 1)
    relu = (lambda v, k: v * torch.tensor(masks[k].astype(np.float64)).permute(0, 3, 1, 2)) if masks else (lambda v, k: F.relu(v))
    x0 = torch.tensor((x.astype(np.float64) - 0.5) * 2.0).permute(0, 3, 1, 2)
    if dtype != 'float32':
        x0 = x0.to(getattr(torch, dtype)).double()
    a = relu(F.group_norm(F.conv2d(x0, std_w(t['block_0/u1/weights']), padding=1), 8, t['block_0/u1/gn/gamma'], t['block_0/u1/gn/beta'], eps=1e-3), 'a')
    u = F.group_norm(F.conv2d(a, std_w(t['block_0/u2/weights'])), 4, t['block_0/u2/gn/gamma'], t['block_0/u2/gn/beta'], eps=1e-3)
    out = relu(u + a, 'out').permute(0, 2, 3, 1)
    if dy is None:
        return out.detach().numpy()
    (out * torch.tensor(dy.astype(np.float64))).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}


def run_case(M, check, dtype='float32', **model_kw):
    import torch
    model = _model(M, half_precision=dtype != 'float32', **model_kw)
    names = lambda prog: [getattr(fn, '__name__', '') for fn, _ in prog.calls]
    for low in (model._train_low, model._eval_low):     # one batched call, in front of the pair rebuild and the pack (libmcn_cpu.so has no pack)
        pre = names(low.prepack)
        assert pre.count('mcn_ws_fwd_run') == 1 and pre[0] == 'mcn_ws_fwd_run' and pre.count('mcn_conv2d_pack_run') == (0 if M._ffi.IS_CPU_LIB else 1), pre
    assert names(model._train_low.bwd).count('mcn_ws_bwd') == 2
    assert {k: v.shape for k, v in model.variables.items()} == SHAPES
    rng = np.random.default_rng(5)
    draw = lambda: {k: ((0.5 + rng.random(s)) if k.endswith('gamma') else rng.standard_normal(s) * (0.3 if len(s) == 4 else 0.5) + (0.2 if len(s) == 4 else 0.0))
                    .astype(np.float32) for k, s in SHAPES.items()}
    ema, vals = draw(), draw()
    model.set_variables(ema), model.set_variables(vals, reset_state=False)        # EMA shadows := ema, then masters := vals
    x, dy = rng.random((3, 9, 11, 3)).astype(np.float32), rng.standard_normal((3, 9, 11, 16)).astype(np.float32)
    model.feed(x, np.zeros(3, np.float32))
    out = model.d['block_0']
    model.forward(train=True)
    check(model.fetch(out), _reference(vals, x, dtype), dtype, 'ws net forward')
    _, grads_ref = _reference(vals, x, dtype, dy, masks={'a': model.fetch(model.d['a']) > 0, 'out': model.fetch(out) > 0})
    out.grad.copy_(torch.as_tensor(dy).to(out.grad.device))
    model.backward()
    grads = model.get_variables('grad')
    for k in SHAPES:
        check(grads[k], grads_ref[k], dtype, 'gradient of ' + k, rel=1e-4 if dtype == 'float32' else None)
    model.forward(train=False)                          # inference: w_hat from the EMA shadows
    check(model.fetch(out), _reference(ema, x, dtype), dtype, 'ws net inference')


if __name__ == '__main__':
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import myconvnet_amd as M
    from test_gpu_ops import check
    assert M._ffi.IS_CPU_LIB, 'run with MCN_LIB_PATH=<repo>/myconvnet_amd/libmcn_cpu.so'
    for dt in ('float32', 'bfloat16'):
        run_case(M, check, dtype=dt, device='cpu')
    print('weight standardisation layer case ok')
