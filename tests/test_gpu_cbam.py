"""The CBAM attention tail on the MI355X (myconvnet_amd/csrc/cbam.hip, reference models/resnet_v2_d_cbam.py:159-211) through the C-ABI against a
float64 NumPy restatement of the formulas in include/mcn.h, and through ConvNet.cbam_attention (tests/cbam_case.py).  Every entry point is compared
on the inputs it was given: the stages behind the first take the device's own (already checked) s / sm, as the C-ABI does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_ops import check  # noqa: E402

# (N, H, W, C, K): each the smallest shape that reaches one way of going wrong
CASES = [(2, 5, 7, 24, 7),        # 3 or 6 chunks per pixel, not a power of two; odd HW; the window is larger than the image
         (2, 9, 8, 64, 3),        # several pixels per wave; the small stencil; cm = 1 (ties certain)
         (1, 3, 3, 1024, 7),      # more chunks than one wave has lanes
         (2, 20, 33, 16, 7)]      # several bands per image (halos cross band edges); several row slices in the pools


def cbam_device(x, cm, a, w, b, dy, dpool, K, dtype):
    """every entry point once, in forward / backward order; all outputs as host arrays"""
    import torch
    from abi_util import DEV, MDT, TDT, dev, host, stream, workspace
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    n, h, wd, c = x.shape
    md = MDT[dtype]
    nan = lambda shape, dt=TDT[dtype]: torch.full(shape, float('nan'), dtype=dt, device=DEV)
    xd, cmd, ad, dyd, dpd, wv, bv = dev(x, dtype), dev(cm, dtype), dev(a, dtype), dev(dy, dtype), dev(dpool, dtype), dev(w), dev(b)
    o = dict(pools=nan((2, n, c)), cm_pair=nan((n, c)), da=nan((2 * n, c)), s=nan((n, h, wd, 2)), sm=nan((n, h, wd)), y=nan(x.shape), dx0=nan(x.shape),
             dcm=nan((n, c)), dw=nan((K, K, 2, 1), torch.float32), db=nan((1,), torch.float32), ties=nan((n, c), torch.float32))
    p = {k: t.data_ptr() for k, t in o.items()}
    ws = workspace(max(lib.mcn_cbam_workspace_bytes(n, h, wd, c, K), lib.mcn_global_avgmax_pool_workspace_bytes(n, h * wd, c)))
    wsa = (ws.data_ptr(), ws.numel() * 4, stream())
    _ffi.check(lib.mcn_global_avgmax_pool_fwd(xd.data_ptr(), p['pools'], n, h * wd, c, md, *wsa))
    _ffi.check(lib.mcn_pair_sigmoid_fwd(ad.data_ptr(), p['cm_pair'], n, c, md, stream()))
    _ffi.check(lib.mcn_pair_sigmoid_bwd(dyd.data_ptr(), p['cm_pair'], p['da'], n, c, md, stream()))          # (the first [N][C] of dy stand in for dcm)
    _ffi.check(lib.mcn_cbam_chpool_fwd(xd.data_ptr(), cmd.data_ptr(), p['s'], n, h * wd, c, md, stream()))
    _ffi.check(lib.mcn_cbam_apply_fwd(xd.data_ptr(), cmd.data_ptr(), p['s'], wv.data_ptr(), bv.data_ptr(), p['sm'], p['y'], n, h, wd, c, K, md, stream()))
    _ffi.check(lib.mcn_cbam_bwd(dyd.data_ptr(), xd.data_ptr(), cmd.data_ptr(), p['s'], p['sm'], wv.data_ptr(), p['pools'], p['dx0'], p['dcm'], p['dw'], p['db'],
                                p['ties'], 1.0, n, h, wd, c, K, md, *wsa))
    o['dx'] = o['dx0'].clone()
    _ffi.check(lib.mcn_global_avgmax_pool_bwd(dpd.data_ptr(), xd.data_ptr(), p['pools'], p['ties'], o['dx'].data_ptr(), 1, n, h * wd, c, md, stream()))
    return {k: host(t) for k, t in o.items()}


def _taps(K):
    return [(i, j) for i in range(K) for j in range(K)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'float16'])
def test_cbam_fwd_bwd(dtype, case):
    from abi_util import lp_round
    n, h, wd, c, K = case
    P, hw = K // 2, h * wd
    r = lambda v: lp_round(v, dtype)
    rng = np.random.default_rng(c + h)
    x = rng.integers(-8, 9, (n, h, wd, c)) / 4.0                               # a coarse grid: ties of both maxima
    cm = np.ones((n, c)) if case == CASES[1] else rng.integers(1, 5, (n, c)) / 4.0
    a, dy, dpool = r(rng.standard_normal((2 * n, c))), r(rng.standard_normal(x.shape)), r(rng.standard_normal((2, n, c)))
    w = (rng.standard_normal((K, K, 2, 1)) * 0.3).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(1).astype(np.float32).astype(np.float64)
    got = cbam_device(x, cm, a, w, b, dy, dpool, K, dtype)

    # forward
    check(got['pools'][0], r(x.mean((1, 2))), dtype, 'pooled means')
    np.testing.assert_array_equal(got['pools'][1], x.max((1, 2)), err_msg='pooled maxima')
    cmp_ = r(1.0 / (1.0 + np.exp(-(a[:n] + a[n:]))))
    check(got['cm_pair'], cmp_, dtype, 'pair sigmoid')
    check(got['da'], np.tile(r(dy.reshape(-1, c)[:n] * got['cm_pair'] * (1.0 - got['cm_pair'])), (2, 1)), dtype, 'pair sigmoid backward')
    xp = r(x * cm[:, None, None, :])
    check(got['s'][..., 0], r(xp.mean(-1)), dtype, 'channel mean')
    np.testing.assert_array_equal(got['s'][..., 1], xp.max(-1), err_msg='channel max')
    s, wq = got['s'].astype(np.float64), r(w)[..., 0]
    sp = np.pad(s, ((0, 0), (P, P), (P, P), (0, 0)))
    t = b[0] + sum((sp[:, i:i + h, j:j + wd] * wq[i, j]).sum(-1) for i, j in _taps(K))
    check(got['sm'], r(1.0 / (1.0 + np.exp(-r(t)))), dtype, 'spatial mask')
    sm = got['sm'].astype(np.float64)
    check(got['y'], r(xp * sm[..., None]), dtype, 'y')

    # backward: equal split among ties
    ind, ind2 = xp == s[..., 1:], x == x.max((1, 2), keepdims=True)
    ties, ties2 = ind.sum(-1, keepdims=True), ind2.sum((1, 2), keepdims=True)
    assert ties.max() > 1 and ties2.max() > 1, 'the inputs must tie both maxima'
    dt = (dy * xp).sum(-1) * sm * (1.0 - sm)
    dtp = np.pad(dt, ((0, 0), (P, P), (P, P)))
    dw = np.stack([(dt[..., None] * sp[:, i:i + h, j:j + wd]).sum((0, 1, 2)) for i, j in _taps(K)]).reshape(K, K, 2, 1)
    ds = sum(dtp[:, 2 * P - i:2 * P - i + h, 2 * P - j:2 * P - j + wd, None] * wq[i, j] for i, j in _taps(K))
    dxp = dy * sm[..., None] + ds[..., :1] / c + ind * ds[..., 1:] / ties
    check(got['dw'], dw, 'float32', 'dw', rel=1e-4)
    check(got['db'], dt.sum().reshape(1), 'float32', 'db', rel=1e-4)
    check(got['dcm'], r((dxp * x).sum((1, 2))), dtype, 'dcm')
    check(got['dx0'], r(dxp * cm[:, None, None, :]), dtype, 'dx before the pool gradient')
    np.testing.assert_array_equal(got['ties'], ties2.reshape(n, c), err_msg='tie counts of the spatial maxima')
    check(got['dx'], r(got['dx0'] + dpool[0][:, None, None, :] / hw + ind2 * dpool[1][:, None, None, :] / ties2), dtype, 'dx')

    again = cbam_device(x, cm, a, w, b, dy, dpool, K, dtype)
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k + ': a repeated call differs')


def test_cbam_through_the_layer_api():
    import myconvnet_amd as M
    import cbam_case
    cbam_case.run_case(M, check)
