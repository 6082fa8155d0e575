"""Transposed convolution: the float64 reference (the gather formula of include/mcn.h written as a scatter over taps, gradients by torch autograd)
and one small layer case — strided conv down -> transposed_conv_layer(5, 2) -> batch_norm -> relu -> transposed_conv_layer(3, 2, biased) to the
logits of a per-pixel loss, two Nesterov steps (the second runs on filters whose swapped and packed copies the prepack program must have refreshed) — shared by
the GPU test (tests/test_gpu_deconv.py) and, run as a script with MCN_LIB_PATH naming libmcn_cpu.so, by tests/test_deconv_abi.py."""
import numpy as np


def same_pads_before(o, k, s):
    return max((-(-o // s) - 1) * s + k - o, 0) // 2


def deconv_ref(x, w, bias, strides, out_hw, pads):
    """torch float64, NHWC: y[oy, ox] += x[iy, ix] @ w[r, q] at oy = iy * SH + r - padT, ox = ix * SW + q - padL, cropped to out_hw"""
    import torch
    n, h, wd, _ = x.shape
    kh, kw, _, cb = w.shape
    (sh, sw), (oh, ow), (pt, pl) = strides, out_hw, pads
    full = x.new_zeros((n, max((h - 1) * sh + kh, pt + oh), max((wd - 1) * sw + kw, pl + ow), cb))
    for r in range(kh):
        for q in range(kw):
            full[:, r:r + (h - 1) * sh + 1:sh, q:q + (wd - 1) * sw + 1:sw] += x @ w[r, q]
    y = full[:, pt:pt + oh, pl:pl + ow]
    return y + bias if bias is not None else y


def deconv_ref_grads(x, w, bias, dy, strides, out_hw, pads):
    """(y, dx, dw, dbias) in float64 numpy"""
    import torch
    t = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (x, w, bias)]
    y = deconv_ref(t[0], t[1], t[2], strides, out_hw, pads)
    (y * torch.tensor(np.asarray(dy, np.float64))).sum().backward()
    return (y.detach().numpy(),) + tuple(a.grad.numpy() for a in t)


SHAPES = {'block_0/down/weights': (3, 3, 3, 16), 'block_0/up1/weights': (5, 5, 16, 8), 'block_0/up1/bn/gamma': (8,), 'block_0/up1/bn/beta': (8,),
          'block_0/up2/weights': (3, 3, 8, 5), 'block_0/up2/biases': (5,)}
CLASSES, BASE_LR = 5, 10.0           # lr = BASE_LR * 3 / 256: large enough that a filter copy left at its step-0 value shows in step 1


def _model(M, **kw):
    class Net(M.ConvNet):
        def _init_params(self, **kwargs):
            pass

        def _build_model(self):
            self._curr_block = 0
            with self.variable_scope('block_0'):
                x = self.conv_layer(self.X, 3, 2, 16, biased=False, scope='down')                    # 9 x 11 -> 5 x 6
                with self.variable_scope('up1'):
                    u = self.transposed_conv_layer(x, 5, 2, 8, biased=False, output_shape=(9, 11))   # odd explicit size
                    x = self.relu(self.batch_norm(u))
                x = self.transposed_conv_layer(x, 3, 2, CLASSES, scope='up2')                        # 18 x 22, biased: per-pixel logits
            return {'up1': u, 'logits': x}
    return Net([9, 11, 3], CLASSES, batch_size=3, num_gpus=1, **kw)


def _net(t, x):
    """float64 torch: (first transposed convolution's output, logits), NHWC"""
    import torch
    import torch.nn.functional as F
    p = 'block_0/'
    x0 = torch.tensor((x.astype(np.float64) - 0.5) * 2.0).permute(0, 3, 1, 2)
    a = F.conv2d(x0, t[p + 'down/weights'].permute(3, 2, 0, 1), stride=2, padding=1).permute(0, 2, 3, 1)
    u = deconv_ref(a, t[p + 'up1/weights'], None, (2, 2), (9, 11), (same_pads_before(9, 5, 2), same_pads_before(11, 5, 2)))
    b = F.relu(F.batch_norm(u.permute(0, 3, 1, 2), None, None, t[p + 'up1/bn/gamma'], t[p + 'up1/bn/beta'], training=True, eps=1e-3)).permute(0, 2, 3, 1)
    return u, deconv_ref(b, t[p + 'up2/weights'], t[p + 'up2/biases'], (2, 2), (18, 22), (same_pads_before(18, 3, 2), same_pads_before(22, 3, 2)))


def _ref_step(st, x, y):
    """One step of the float64 restatement on st = dict(params, accum, ema, step): (loss, gradients); loss, Nesterov update and EMA as oracle/ops.py"""
    import torch
    from oracle import ops as O
    t = {k: torch.tensor(v, requires_grad=True) for k, v in st['params'].items()}
    _, logits = _net(t, x)
    onehot = O.seg_one_hot_labels(y.astype(np.float64), CLASSES, dtype=np.float64).reshape(-1, CLASSES)
    _, sm_loss, _, dlogits = O.softmax_xent_fwd_bwd(logits.detach().numpy().reshape(-1, CLASSES), onehot)
    (logits * torch.tensor(dlogits.reshape(tuple(logits.shape)))).sum().backward()
    grads = {k: v.grad.numpy() for k, v in t.items()}
    loss = float(sm_loss) + O.l2_reg_loss([v for k, v in st['params'].items() if k.endswith('/weights')], 1e-4)
    d = O.ema_decay(0.99, st['step'])
    for k in st['params']:
        st['params'][k], st['accum'][k], st['ema'][k] = O.sgd_nesterov_step(st['params'][k], grads[k], st['accum'][k], BASE_LR * 3 / 256.0, 0.9,
                                                                            l2=1e-4 if k.endswith('/weights') else 0.0, ema=st['ema'][k], ema_d=d)
    st['step'] += 1
    return loss, grads


def run_case(M, check, **model_kw):
    model = _model(M, **model_kw)
    names = lambda prog: [getattr(fn, '__name__', '') for fn, _ in prog.calls]
    assert names(model._train_low.fwd).count('mcn_deconv2d_fwd') == 2
    bwd = names(model._train_low.bwd)
    assert bwd.count('mcn_deconv2d_dgrad') == 2 and bwd.count('mcn_deconv2d_wgrad') == 2, bwd
    pre = names(model._train_low.prepack)                 # swapped copies (and the packed operands, GPU only) in front of the batched conv pack
    assert pre.count('mcn_filter_swap_io') == 2 and pre.count('mcn_deconv2d_pack') == (0 if M._ffi.IS_CPU_LIB else 2), pre
    if not M._ffi.IS_CPU_LIB:
        assert pre.index('mcn_conv2d_pack_run') > max(i for i, n in enumerate(pre) if n == 'mcn_filter_swap_io'), pre
    got = {k: v.shape for k, v in model.variables.items() if not k.endswith(('/mu', '/sigma'))}
    assert got == SHAPES, got
    rng = np.random.default_rng(5)
    vals = {k: ((0.5 + rng.random(s)) if k.endswith('gamma') else rng.standard_normal(s) * (0.2 if len(s) == 4 else 0.5)).astype(np.float32) for k, s in SHAPES.items()}
    model.set_variables(vals)                             # masters and EMA shadows
    opt = M.MomentumOptimizer(model, None, None, base_learning_rate=BASE_LR, steps_per_epoch=1, learning_warmup_epochs=0.0)
    f64 = lambda d: {k: np.asarray(v, np.float64) for k, v in d.items()}
    st = dict(params=f64(vals), accum={k: np.zeros(s) for k, s in SHAPES.items()}, ema=f64(vals), step=0)
    for step in range(2):
        x = rng.random((3, 9, 11, 3)).astype(np.float32)
        y = rng.integers(0, CLASSES + 1, (3, 18, 22)).astype(np.float32)                        # 0 = ignored pixel
        before = {k: v.copy() for k, v in st['params'].items()}
        model.feed(x, y)
        loss = opt._step(None)[0]
        rloss, rgrads = _ref_step(st, x, y)
        assert abs(loss - rloss) <= 1e-4 * abs(rloss), (step, loss, rloss)
        grads, now = model.get_variables('grad'), model.get_variables('data')
        for k in SHAPES:
            check(grads[k], rgrads[k], 'float32', 'step {}: gradient of {}'.format(step, k), rel=1e-4)
            check(now[k] - before[k], st['params'][k] - before[k], 'float32', 'step {}: update of {}'.format(step, k), rel=1e-4)
    model.feed(x, y)
    model.forward(train=False)                            # inference: the same kernel on the EMA shadows, packed by the eval lowering's own prepack
    import torch
    with torch.no_grad():
        u_ref = _net({k: torch.tensor(v) for k, v in st['ema'].items()}, x)[0].numpy()
    check(model.fetch(model.d['up1']), u_ref, 'float32', 'deconv net inference on the EMA shadows')


if __name__ == '__main__':
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import myconvnet_amd as M
    from test_gpu_ops import check
    assert M._ffi.IS_CPU_LIB, 'run with MCN_LIB_PATH=<repo>/myconvnet_amd/libmcn_cpu.so'
    run_case(M, check, device='cpu')
    print('deconv layer case ok')
