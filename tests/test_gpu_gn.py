"""Group normalisation on the MI355X (myconvnet_amd/csrc/gn.hip: mcn_gn_fwd / mcn_gn_bwd, reference convnet.py:1928-2013) through the C-ABI against a
float64 NumPy restatement of the formulas in include/mcn.h, on both launch paths, and through ConvNet.group_norm (tests/gn_case.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_ops import check  # noqa: E402

EPS = 1e-3
# (N, H, W, C, G): each the smallest shape that reaches one way of going wrong
CASES = [(2, 5, 7, 16, 8),        # 2 channels per group: a chunk spans 2 (fp32) / 4 (2-byte) groups; HW = 35 is odd against every row-lane count / unroll
         (3, 4, 4, 32, 32),       # 1 channel per group
         (2, 6, 6, 32, 4),        # a group = one 2-byte chunk / two fp32 chunks
         (2, 3, 3, 2048, 32),     # a group spans 8-16 chunks; more columns than one workgroup holds
         (2, 40, 40, 64, 32),     # several row slices per image (two-pass); too large a slab for LDS (resident: refused)
         (4, 1, 1, 64, 32)]       # the 2-D [B, C] case


def gn_ref(x, gamma, beta, G, eps):
    n, hw, c = x.shape
    xg = x.reshape(n, hw, G, c // G)
    mean, var = xg.mean(axis=(1, 3), keepdims=True), xg.var(axis=(1, 3), keepdims=True)
    inv = 1.0 / np.sqrt(var + eps)
    xh = ((xg - mean) * inv).reshape(n, hw, c)
    return xh * gamma + beta, mean.reshape(n, G), inv.reshape(n, G), xh


def gn_bwd_ref(dz, xh, inv, gamma, G):
    n, hw, c = dz.shape
    t, xg = (dz * gamma).reshape(n, hw, G, c // G), xh.reshape(n, hw, G, c // G)
    dx = inv.reshape(n, 1, G, 1) * (t - t.mean(axis=(1, 3), keepdims=True) - xg * (t * xg).mean(axis=(1, 3), keepdims=True))
    return dx.reshape(n, hw, c), (dz * xh).sum(axis=(0, 1)), dz.sum(axis=(0, 1))


def gn_device(x, gamma, beta, skip, dy, G, act, dtype, path, want_params=True):
    """mcn_gn_fwd then mcn_gn_bwd (mask from the stored y) on the device; every output as a host array"""
    import torch
    from abi_util import DEV, MDT, TDT, dev, host, stream, workspace
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    n, hw, c = x.shape
    p = lambda t: t.data_ptr() if t is not None else 0
    xd, dyd = dev(x, dtype), dev(dy, dtype)
    sd = dev(skip, dtype) if skip is not None else None
    gd, bd = (dev(gamma), dev(beta)) if gamma is not None else (None, None)
    nan = lambda shape, dt: torch.full(shape, float('nan'), dtype=dt, device=DEV)
    y, dx = nan(x.shape, TDT[dtype]), nan(x.shape, TDT[dtype])
    dsk = nan(x.shape, TDT[dtype]) if skip is not None else None
    sm, si = nan((n, G), torch.float32), nan((n, G), torch.float32)
    dg, db = (nan((c,), torch.float32), nan((c,), torch.float32)) if want_params else (None, None)
    ws = workspace(lib.mcn_gn_workspace_bytes(n, hw, c, G))
    _ffi.check(lib.mcn_gn_fwd(xd.data_ptr(), p(gd), p(bd), p(sd), y.data_ptr(), sm.data_ptr(), si.data_ptr(), n, hw, c, G, EPS, act, MDT[dtype], path,
                              ws.data_ptr(), ws.numel() * 4, stream()))
    _ffi.check(lib.mcn_gn_bwd(dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), p(gd), sm.data_ptr(), si.data_ptr(), dx.data_ptr(), p(dsk), p(dg), p(db), 1.0,
                              n, hw, c, G, act, MDT[dtype], path, ws.data_ptr(), ws.numel() * 4, stream()))
    return {k: host(t) for k, t in dict(y=y, mean=sm, invstd=si, dx=dx, dskip=dsk, dgamma=dg, dbeta=db).items() if t is not None}


def _inputs(case, dtype, seed=0):
    from abi_util import lp_round
    n, h, w, c, G = case
    rng = np.random.default_rng(seed + c + h)
    r = lambda *s: lp_round(rng.standard_normal(s), dtype)
    x = lp_round(rng.standard_normal((n, h * w, c)) * 2.0 + 3.0, dtype)        # non-zero mean: exercises the shifted sums
    gamma, beta = (0.5 + rng.random(c)).astype(np.float32).astype(np.float64), rng.standard_normal(c).astype(np.float32).astype(np.float64)
    return x, gamma, beta, r(n, h * w, c), r(n, h * w, c)


@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'add_relu'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('path', [1, 2], ids=['two_pass', 'resident'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'float16'])
def test_gn_fwd_bwd(dtype, path, case, fused):
    from abi_util import MDT
    from myconvnet_amd import _ffi
    n, h, w, c, G = case
    x, gamma, beta, skip, dy = _inputs(case, dtype)
    act = _ffi.ACT_RELU if fused else _ffi.ACT_NONE
    if path == _ffi.GN_RESIDENT and not (_ffi.lib.mcn_gn_resident_ok(0, n, h * w, c, G, MDT[dtype]) and _ffi.lib.mcn_gn_resident_ok(1, n, h * w, c, G, MDT[dtype])):
        assert case == (2, 40, 40, 64, 32)                     # 1600 pixels x 128 bytes: above the LDS budget in either direction
        with pytest.raises(_ffi.McnError) as e:
            gn_device(x, gamma, beta, None, dy, G, act, dtype, path)
        assert e.value.code == _ffi.E_UNSUPPORTED
        return
    got = gn_device(x, gamma, beta, skip if fused else None, dy, G, act, dtype, path)
    z, mean, inv, xh = gn_ref(x, gamma, beta, G, EPS)
    y_ref = np.maximum(z + skip, 0.0) if fused else z
    check(got['y'], y_ref, dtype, 'y')
    check(got['mean'], mean, 'float32', 'save_mean', rel=1e-5)
    check(got['invstd'], inv, 'float32', 'save_invstd', rel=1e-5)
    dz = dy * (got['y'] > 0) if fused else dy                  # the mask the device stored: near-ties cannot turn into gradient errors
    dx_ref, dgamma_ref, dbeta_ref = gn_bwd_ref(dz, xh, inv, gamma, G)
    check(got['dx'], dx_ref, dtype, 'dx')
    if fused:
        check(got['dskip'], dz, dtype, 'dskip')
    check(got['dgamma'], dgamma_ref, 'float32', 'dgamma', rel=1e-4)
    check(got['dbeta'], dbeta_ref, 'float32', 'dbeta', rel=1e-4)
    again = gn_device(x, gamma, beta, skip if fused else None, dy, G, act, dtype, path)
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k + ': a repeated call differs')


@pytest.mark.parametrize('path', [1, 2], ids=['two_pass', 'resident'])
def test_gn_without_parameters(path):
    """gamma = beta = NULL (scale=False / shift=False) and dgamma = dbeta = NULL (frozen block: only dx is wanted)"""
    x, _, _, _, dy = _inputs(CASES[0], 'float32')
    G = CASES[0][4]
    got = gn_device(x, None, None, None, dy, G, 0, 'float32', path, want_params=False)
    z, _, inv, xh = gn_ref(x, 1.0, 0.0, G, EPS)
    check(got['y'], z, 'float32', 'y')
    check(got['dx'], gn_bwd_ref(dy, xh, inv, 1.0, G)[0], 'float32', 'dx')
    assert 'dgamma' not in got


def test_gn_through_the_layer_api():
    import myconvnet_amd as M
    import gn_case
    gn_case.run_case(M, check)
