"""norm_type='grouped_batch' through the layer API (reference convnet.py:2176-2376): ResNet-18 at 1/8 width, every normalisation a
grouped batch norm of 8 channels per group, against a torch-CPU float64 restatement (moments over N x H x W x 8, biased variance) —
shared by the GPU test (tests/test_gpu_gbn.py) and, run as a script with MCN_LIB_PATH naming libmcn_cpu.so, by the host-code case of
tests/test_gbn_abi.py."""
import numpy as np

P, EPS, MOM = 8, 1e-3, 0.99
UNITS = [(i, j, 1 if (i == 1 or j) else 2) for i in range(1, 5) for j in range(2)]         # (block, unit, stride)


def _reference(vals, stats, x, labels, train, masks=None):
    """float64 torch.  train: (pred, gradients of the mean cross-entropy, {mu / sigma name: batch statistic}); else pred from the moving
    statistics.  `masks`: the ReLU decisions the device stored, so that an activation within rounding of zero is not a gradient error."""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in vals.items()}
    batch = {}

    def conv(a, scope, stride):
        w = t[scope + '/weights'].permute(3, 2, 0, 1)
        k = w.shape[-1]
        pad = max((-(-a.shape[-1] // stride) - 1) * stride + k - a.shape[-1], 0)               # TF 'SAME': the odd pixel goes to the bottom / right
        return F.conv2d(F.pad(a, (pad // 2, pad - pad // 2, pad // 2, pad - pad // 2)), w, stride=stride)

    def norm(a, scope):
        n, c, h, w = a.shape
        if train:
            g = a.reshape(n, c // P, P, h, w)
            mean, var = g.mean(dim=(0, 2, 3, 4), keepdim=True), g.var(dim=(0, 2, 3, 4), unbiased=False, keepdim=True)
            xh = ((g - mean) / (var + EPS).sqrt()).reshape(a.shape)
            batch[scope + '/mu'] = mean.detach().reshape(-1, 1).expand(-1, P).reshape(-1).numpy()
            batch[scope + '/sigma'] = var.detach().reshape(-1, 1).expand(-1, P).reshape(-1).numpy()
        else:
            mu, sg = (torch.tensor(np.asarray(stats[scope + '/' + k], np.float64)).reshape(1, c, 1, 1) for k in ('mu', 'sigma'))
            xh = (a - mu) / (sg + EPS).sqrt()
        return xh * t[scope + '/gamma'].reshape(1, c, 1, 1) + t[scope + '/beta'].reshape(1, c, 1, 1)

    def relu(a, key):
        return a * torch.tensor(masks[key].astype(np.float64)).permute(0, 3, 1, 2) if masks else F.relu(a)

    a = torch.tensor((x.astype(np.float64) - 0.5) * 2.0).permute(0, 3, 1, 2)
    a = relu(norm(conv(a, 'block_0/conv_0', 2), 'block_0/conv_0/bn'), 'block_0/conv_0/relu')
    a = F.max_pool2d(F.pad(a, (0, 1, 0, 1), value=-1e30), 3, 2)
    for i, j, s in UNITS:
        u = 'block_{}/res_{}'.format(i, j)
        skip = norm(conv(a, u + '/conv_skip', s), u + '/conv_skip/bn') if u + '/conv_skip/weights' in t else a
        a = relu(norm(conv(a, u + '/conv_0', s), u + '/conv_0/bn'), u + '/conv_0/relu')
        a = relu(norm(conv(a, u + '/conv_1', 1), u + '/conv_1/bn') + skip, u)
    logits = a.mean(dim=(2, 3)) @ t['block_None/logits/weights'] + t['block_None/logits/biases']
    pred = F.softmax(logits, dim=1).detach().numpy()
    if not train:
        return pred
    F.cross_entropy(logits, torch.tensor(labels.astype(np.int64))).backward()
    return pred, {k: v.grad.numpy() for k, v in t.items()}, batch


def run_case(M, check, **model_kw):
    model = M.ResNet18([32, 32, 3], 10, batch_size=4, width_div=8, norm_type='grouped_batch', num_gpus=1, **model_kw)
    norms = [n for n in model.graph.nodes if n.op in ('bn', 'gn', 'gbn')]
    assert len(norms) == 20 and all(n.op == 'gbn' and n.attrs['cpg'] == P for n in norms), [(n.op, n.attrs.get('cpg')) for n in norms]
    assert all(n.attrs.get('act', 0) == M._ffi.ACT_RELU or n.attrs['scope'].endswith('conv_skip/bn') for n in norms)      # relu absorbed ...
    assert sum(n.attrs.get('skip') is not None for n in norms) == 8 and not [n for n in model.graph.nodes if n.op in ('relu', 'add')]      # ... and every add
    names = lambda prog: [getattr(fn, '__name__', '') for fn, _ in prog.calls]
    assert names(model._train_low.fwd).count('mcn_gbn_fwd_train') == 20 and names(model._train_low.bwd).count('mcn_gbn_bwd') == 20
    assert names(model._eval_low.fwd).count('mcn_bn_fwd_infer') == 20 and not [k for k in names(model._train_low.fwd) if k.startswith('mcn_bn_')]
    rng = np.random.default_rng(23)
    kinds = {k: v.kind for k, v in model.variables.items()}
    draw = lambda: {k: ((0.5 + rng.random(v.shape)) if kinds[k] == 'gamma' else rng.standard_normal(v.shape) * (0.3 if kinds[k] == 'weight' else 0.5)).astype(np.float32)
                    for k, v in model.variables.items() if kinds[k] in ('weight', 'bias', 'gamma', 'beta')}
    stats0 = {k: ((0.5 + rng.random(v.shape)) if kinds[k] == 'sigma' else rng.standard_normal(v.shape) * 0.2).astype(np.float32)
              for k, v in model.variables.items() if kinds[k] in ('mu', 'sigma')}
    ema, vals = draw(), draw()
    model.set_variables(dict(ema, **stats0))            # EMA shadows (moving statistics included) := ema, stats0 ...
    model.set_variables(vals, reset_state=False)        # ... masters := vals
    x, labels = rng.random((4, 32, 32, 3)).astype(np.float32), np.array([3, 0, 9, 3], np.float32)
    model.feed(x, labels)
    model.forward(train=False)
    check(model.fetch(model.pred), _reference(ema, stats0, x, labels, False), 'float32', 'evaluation: moving statistics')
    model.forward(train=True)
    units = ['block_{}/res_{}'.format(i, j) for i, j, _ in UNITS]
    masks = {k: model.fetch(model.d[k]) > 0 for k in ['block_0/conv_0/relu'] + units + [u + '/conv_0/relu' for u in units]}
    pred_ref, grads_ref, batch = _reference(vals, None, x, labels, True, masks)
    check(model.fetch(model.pred), pred_ref, 'float32', 'training forward')
    model.backward()
    grads = model.get_variables('grad')
    for k in vals:
        check(grads[k], grads_ref[k], 'float32', 'gradient of ' + k, rel=1e-4)
    after = model.get_variables('data')
    for k in stats0:                                    # m*old + (1-m)*batch, the batch variance BIASED
        check(after[k], MOM * stats0[k].astype(np.float64) + (1.0 - MOM) * batch[k], 'float32', 'running ' + k, rel=1e-5)


if __name__ == '__main__':
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import myconvnet_amd as M
    from test_gpu_ops import check
    assert M._ffi.IS_CPU_LIB, 'run with MCN_LIB_PATH=<repo>/myconvnet_amd/libmcn_cpu.so'
    run_case(M, check, device='cpu')
    print('grouped batch norm layer case ok')
