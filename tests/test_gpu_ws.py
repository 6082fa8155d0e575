"""Weight standardisation on the MI355X (myconvnet_amd/csrc/ws.hip: mcn_ws_table_build / mcn_ws_fwd_run / mcn_ws_bwd, reference convnet.py:1410-1419) through the
C-ABI against a float64 NumPy restatement of the formulas in include/mcn.h, and through conv_layer(ws=True) (tests/ws_case.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_ops import check  # noqa: E402

EPS, GUARD = 1e-5, 64
# (K, C): each the smallest shape that reaches one way of going wrong
CASES = [(9, 4),          # fewer rows than row lanes, one chunk of columns
         (147, 64),       # the 7x7x3 stem: K odd against every lane count / unroll
         (64, 256),       # plain 1x1, several full strips
         (4608, 40),      # the longest ResNet-50 column (row slices, slice fold) + a tail strip
         (300, 6),        # C % 4 != 0: rows not 16-byte aligned, scalar-column path
         (333, 1)]        # a single column (the depthwise shape of the follow-up)


def _inputs(case):
    K, C = case
    rng = np.random.default_rng(K + C)
    w = (0.3 * rng.standard_normal((K, C)) + 0.5).astype(np.float32).astype(np.float64)      # non-zero mean: exercises the shifted sums
    return w, rng.standard_normal((K, C)).astype(np.float32).astype(np.float64)


def ws_ref(w, g):
    m = w.mean(axis=0)
    s = np.sqrt(((w - m) ** 2).mean(axis=0))
    assert s.min() >= 0.05, 'ill-conditioned column in the test input'
    wh = (w - m) / (s + EPS)
    return wh, m, s, (g - g.mean(axis=0)) / (s + EPS) - wh * (g * wh).mean(axis=0) / s


def ws_device(cases):
    """all of `cases` through ONE table, then mcn_ws_bwd per tensor out of place and in place; NaN-filled outputs with NaN guards behind each"""
    import torch
    from abi_util import DEV, dev, host, stream, workspace
    from myconvnet_amd import _ffi
    nan = lambda n: torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    t = [dict(K=K, C=C, w=dev(_inputs((K, C))[0]), g=dev(_inputs((K, C))[1]), w_hat=nan(K * C), stats=nan(2 * C), dw=nan(K * C)) for K, C in cases]
    jobs = [_ffi.WsJob(d['w'].data_ptr(), d['w_hat'].data_ptr(), d['stats'].data_ptr(), d['K'], d['C']) for d in t]
    table, ndesc, nbytes = _ffi.ws_table(jobs)
    table, ws = torch.frombuffer(table, dtype=torch.uint8).to(DEV), workspace(nbytes)
    _ffi.check(_ffi.lib.mcn_ws_fwd_run(table.data_ptr(), ndesc, EPS, ws.data_ptr(), ws.numel() * 4, stream()))
    out = []
    for d in t:
        K, C = d['K'], d['C']
        wb = workspace(_ffi.lib.mcn_ws_bwd_workspace_bytes(K, C))
        bwd = lambda dst: _ffi.check(_ffi.lib.mcn_ws_bwd(d['g'].data_ptr(), d['w_hat'].data_ptr(), d['stats'].data_ptr(), dst.data_ptr(), K, C, EPS, wb.data_ptr(), wb.numel() * 4, stream()))
        bwd(d['dw'])
        bwd(d['g'])                                            # in place: dw == dw_hat
        r = dict({k: host(d[k]) for k in ('w_hat', 'stats', 'dw')}, dw_inplace=host(d['g']).ravel())
        for k, n in (('w_hat', K * C), ('stats', 2 * C), ('dw', K * C)):
            assert np.isnan(r[k][n:]).all(), k + ': wrote behind its buffer'
            r[k] = r[k][:n]
        out.append(r)
    return out


@pytest.fixture(scope='module')
def single():
    return {case: ws_device([case])[0] for case in CASES}


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_ws_fwd_bwd(case, single):
    (K, C), got = case, single[case]
    wh, m, s, dw = ws_ref(*_inputs(case))
    check(got['w_hat'].reshape(K, C), wh, 'float32', 'w_hat')
    check(got['stats'][:C], m, 'float32', 'm', rel=1e-5)
    check(got['stats'][C:], s, 'float32', 's', rel=1e-5)
    check(got['dw'].reshape(K, C), dw, 'float32', 'dw')
    np.testing.assert_array_equal(got['dw_inplace'], got['dw'], err_msg='in place (dw == dw_hat) differs from out of place')
    for k, v in ws_device([case])[0].items():
        np.testing.assert_array_equal(v, got[k], err_msg=k + ': a repeated call differs')


def test_ws_one_table_for_all_tensors(single):
    for case, got in zip(CASES, ws_device(CASES)):
        for k in ('w_hat', 'stats', 'dw'):
            np.testing.assert_array_equal(got[k], single[case][k], err_msg='{} of {} in the shared table'.format(k, case))


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_ws_through_the_layer_api(dtype):
    import myconvnet_amd as M
    import ws_case
    ws_case.run_case(M, check, dtype=dtype)
