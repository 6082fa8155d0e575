"""Grouped batch normalisation on the MI355X (myconvnet_amd/csrc/gbn.hip: mcn_gbn_fwd_train / mcn_gbn_bwd, reference convnet.py:2176-2376) through
the C-ABI against a float64 NumPy restatement of the formulas in include/mcn.h, and through norm_type='grouped_batch' (tests/gbn_case.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_ops import check  # noqa: E402

EPS, MOM = 1e-3, 0.9
# (N, H, W, C, P): each the smallest shape that reaches one way of going wrong
CASES = [(2, 5, 7, 16, 8),        # a group = one 2-byte chunk / two fp32 chunks; M = 70 is odd against row-lane counts and unrolls
         (3, 4, 4, 32, 4),        # two groups per 2-byte chunk, one per fp32 chunk
         (2, 3, 3, 64, 2),        # several groups per chunk in every type
         (2, 3, 3, 2048, 32),     # a group spans 4-8 chunk columns; more columns than one workgroup holds
         (2, 40, 40, 64, 8),      # many row partials to merge
         (4, 1, 1, 64, 64)]       # P == C, the 2-D [B, C] shape


def gbn_ref(x, gamma, beta, P, eps):
    m, c = x.shape
    xg = x.reshape(m, c // P, P)
    mean, var = xg.mean(axis=(0, 2), keepdims=True), xg.var(axis=(0, 2), keepdims=True)      # biased
    inv = 1.0 / np.sqrt(var + eps)
    xh = ((xg - mean) * inv).reshape(m, c)
    return xh * gamma + beta, mean.reshape(-1), var.reshape(-1), inv.reshape(-1), xh


def gbn_bwd_ref(dz, xh, inv, gamma, P):
    m, c = dz.shape
    t, xg = (dz * gamma).reshape(m, c // P, P), xh.reshape(m, c // P, P)
    dx = inv.reshape(1, -1, 1) * (t - t.mean(axis=(0, 2), keepdims=True) - xg * (t * xg).mean(axis=(0, 2), keepdims=True))
    return dx.reshape(m, c), (dz * xh).sum(axis=0), dz.sum(axis=0)


def gbn_device(x, gamma, beta, skip, dy, running, P, act, dtype, want_params=True):
    """mcn_gbn_fwd_train then mcn_gbn_bwd (ReLU mask from the stored y) on the device; every output as a host array"""
    import torch
    from abi_util import DEV, MDT, TDT, dev, host, stream, workspace
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    m, c = x.shape
    p = lambda t: t.data_ptr() if t is not None else 0
    xd, dyd = dev(x, dtype), dev(dy, dtype)
    sd = dev(skip, dtype) if skip is not None else None
    gd, bd = (dev(gamma), dev(beta)) if gamma is not None else (None, None)
    nan = lambda shape, dt: torch.full(shape, float('nan'), dtype=dt, device=DEV)
    y, dx = nan(x.shape, TDT[dtype]), nan(x.shape, TDT[dtype])
    dsk = nan(x.shape, TDT[dtype]) if skip is not None else None
    sm, si, bm, bv = nan((c // P,), torch.float32), nan((c // P,), torch.float32), nan((c,), torch.float32), nan((c,), torch.float32)
    rm, rv = dev(running[0]), dev(running[1])
    dg, db = (nan((c,), torch.float32), nan((c,), torch.float32)) if want_params else (None, None)
    ws = workspace(lib.mcn_gbn_workspace_bytes(m, c, P))
    _ffi.check(lib.mcn_gbn_fwd_train(xd.data_ptr(), p(gd), p(bd), p(sd), y.data_ptr(), sm.data_ptr(), si.data_ptr(), bm.data_ptr(), bv.data_ptr(), rm.data_ptr(),
                                     rv.data_ptr(), MOM, m, c, P, EPS, act, MDT[dtype], ws.data_ptr(), ws.numel() * 4, stream()))
    _ffi.check(lib.mcn_gbn_bwd(dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), p(gd), p(bd), sm.data_ptr(), si.data_ptr(), dx.data_ptr(), p(dsk), p(dg), p(db), 1.0,
                               m, c, P, act, MDT[dtype], ws.data_ptr(), ws.numel() * 4, stream()))
    out = dict(y=y, save_mean=sm, save_invstd=si, batch_mean=bm, batch_var=bv, running_mean=rm, running_var=rv, dx=dx, dskip=dsk, dgamma=dg, dbeta=db)
    return {k: host(t) for k, t in out.items() if t is not None}


def _inputs(case, dtype, seed=0):
    from abi_util import lp_round
    n, h, w, c, P = case
    m = n * h * w
    rng = np.random.default_rng(seed + c + h)
    r = lambda *s: lp_round(rng.standard_normal(s), dtype)
    x = lp_round(rng.standard_normal((m, c)) * 2.0 + 3.0, dtype)               # non-zero mean: exercises the shifted sums
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return x, f32(0.5 + rng.random(c)), f32(rng.standard_normal(c)), r(m, c), r(m, c), (f32(rng.standard_normal(c)), f32(0.5 + rng.random(c)))


@pytest.mark.parametrize('variant', ['plain', 'add_relu', 'swish'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'float16'])
def test_gbn_fwd_bwd(dtype, case, variant):
    from myconvnet_amd import _ffi
    P = case[4]
    x, gamma, beta, skip, dy, running = _inputs(case, dtype)
    skip = skip if variant == 'add_relu' else None
    act = {'plain': _ffi.ACT_NONE, 'add_relu': _ffi.ACT_RELU, 'swish': _ffi.ACT_SWISH}[variant]
    got = gbn_device(x, gamma, beta, skip, dy, running, P, act, dtype)
    z, mean, var, inv, xh = gbn_ref(x, gamma, beta, P, EPS)
    sig = 1.0 / (1.0 + np.exp(-z))
    y_ref = {'plain': z, 'add_relu': np.maximum(z + (0.0 if skip is None else skip), 0.0), 'swish': z * sig}[variant]
    check(got['y'], y_ref, dtype, 'y')
    tile = lambda a: np.repeat(a, P)
    for k, ref in (('save_mean', mean), ('save_invstd', inv), ('batch_mean', tile(mean)), ('batch_var', tile(var)),
                   ('running_mean', MOM * running[0] + (1.0 - MOM) * tile(mean)), ('running_var', MOM * running[1] + (1.0 - MOM) * tile(var))):
        check(got[k], ref, 'float32', k, rel=1e-5)
    # ReLU: the mask the device stored, near-ties cannot turn into gradient errors
    dz = {'plain': dy, 'add_relu': dy * (got['y'] > 0), 'swish': dy * sig * (1.0 + z * (1.0 - sig))}[variant]
    dx_ref, dgamma_ref, dbeta_ref = gbn_bwd_ref(dz, xh, inv, gamma, P)
    check(got['dx'], dx_ref, dtype, 'dx')
    if skip is not None:
        check(got['dskip'], dz, dtype, 'dskip')
    check(got['dgamma'], dgamma_ref, 'float32', 'dgamma', rel=1e-4)
    check(got['dbeta'], dbeta_ref, 'float32', 'dbeta', rel=1e-4)
    again = gbn_device(x, gamma, beta, skip, dy, running, P, act, dtype)
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k + ': a repeated call differs')


def test_gbn_without_parameters():
    """gamma = beta = NULL (scale=False / shift=False) and dgamma = dbeta = NULL (frozen block: only dx is wanted)"""
    x, _, _, _, dy, running = _inputs(CASES[0], 'float32')
    P = CASES[0][4]
    got = gbn_device(x, None, None, None, dy, running, P, 0, 'float32', want_params=False)
    z, _, _, inv, xh = gbn_ref(x, 1.0, 0.0, P, EPS)
    check(got['y'], z, 'float32', 'y')
    check(got['dx'], gbn_bwd_ref(dy, xh, inv, 1.0, P)[0], 'float32', 'dx')
    assert 'dgamma' not in got


def test_gbn_through_the_layer_api():
    import myconvnet_amd as M
    import gbn_case
    gbn_case.run_case(M, check)
