"""mcn_deconv2d_fwd / _dgrad / _wgrad on the GPU against the float64 gather formula (tests/deconv_case.py), and the layer case."""
import ctypes

import numpy as np
import pytest
import torch

from deconv_case import deconv_ref_grads, run_case, same_pads_before
from test_gpu_ops import check

pytestmark = pytest.mark.gpu

# (N, h, w, Cs, Cb, KH, KW, SH, SW, OH, OW): each the smallest shape that reaches one way of going wrong
CASES = [
    (2, 3, 4, 16, 24, 5, 5, 2, 2, 6, 8),        # four phases of 4/6/6/9 taps; halo leaves the image on all sides; tile larger than the image
    (1, 9, 19, 32, 3, 5, 5, 2, 2, 18, 37),      # narrow output (Cb = 3); odd sizes; several tiles in both directions (also at the fp32 tile width of 16: 20 base columns)
    (2, 5, 4, 8, 16, 3, 3, 2, 2, 9, 7),         # explicit odd output_shape: the last phase row and column are short
    (2, 4, 4, 40, 72, 2, 2, 2, 2, 8, 8),        # k == s: one tap per phase; Cs not a whole K-step; Cb not a whole N block
    (1, 6, 5, 16, 16, 4, 4, 2, 2, 12, 10),      # even kernel
    (2, 4, 5, 16, 8, 3, 3, 1, 1, 4, 5),         # stride 1: a single phase
    (1, 3, 4, 16, 8, 5, 3, 2, 1, 6, 4),         # mixed strides, non-square filter
    (1, 2, 2, 520, 64, 3, 3, 2, 2, 4, 4),       # many K-steps with a remainder; both buffers wrap
    (1, 3, 2, 6, 5, 3, 3, 3, 3, 7, 6),          # gather kernel: stride 3, channels not chunk multiples
]


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'float16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_deconv_entry_points(case, dtype):
    import abi_util as U
    from myconvnet_amd import _ffi
    lib, dt = _ffi.lib, U.MDT[dtype]
    N, h, w, Cs, Cb, KH, KW, SH, SW, OH, OW = case
    rng = np.random.default_rng(sum(case))
    x, wt = U.lp_round(rng.standard_normal((N, h, w, Cs)), dtype), U.lp_round(rng.standard_normal((KH, KW, Cs, Cb)) * 0.2, dtype)
    bias, dy = rng.standard_normal(Cb).astype(np.float32).astype(np.float64), U.lp_round(rng.standard_normal((N, OH, OW, Cb)), dtype)
    pads = [same_pads_before(OH, KH, SH), 0, same_pads_before(OW, KW, SW), 0]
    pads[1] = max((h - 1) * SH + KH - OH, 0) - pads[0]
    pads[3] = max((w - 1) * SW + KW - OW, 0) - pads[2]
    g = _ffi.conv_geom(N, OH, OW, Cb, Cs, KH, KW, SH, SW, 1, 1, tuple(pads))
    y_ref, dx_ref, dw_ref, db_ref = deconv_ref_grads(x, wt, bias, dy, (SH, SW), (OH, OW), (pads[0], pads[2]))
    xd, wd, bd, dyd = U.dev(x, dtype), U.dev(wt), U.dev(bias), U.dev(dy, dtype)
    nan = lambda shape, t: torch.full(shape, float('nan'), dtype=t, device=U.DEV)
    gt = _ffi.conv_geom(N, OH, OW, Cb, Cs, KH, KW, SH, SW, 1, 1, tuple(pads), 0, 1)
    ws = U.workspace(max(lib.mcn_deconv2d_workspace_bytes(op, ctypes.byref(gg), dt) for op in (0, 1, 2) for gg in (g, gt)))
    wsa = (ws.data_ptr(), ws.numel() * 4, U.stream())
    g.tile = 0 if Cb <= 16 else 1                          # (the fused kernel, forced where the dispatcher may route to the conv kernels: its own choice below)
    nb = int(lib.mcn_deconv2d_packed_bytes(ctypes.byref(g), dt))
    assert (nb == 0) == (SH == 3)
    pk = torch.zeros(max(nb, 1), dtype=torch.uint8, device=U.DEV)
    if nb:
        _ffi.check(lib.mcn_deconv2d_pack(wd.data_ptr(), pk.data_ptr(), ctypes.byref(g), dt, U.stream()))
    outs = []
    for b, packed in ((bd.data_ptr(), pk.data_ptr() if nb else 0), (0, 0), (bd.data_ptr(), pk.data_ptr() if nb else 0)):
        y = nan((N, OH, OW, Cb), U.TDT[dtype])
        _ffi.check(lib.mcn_deconv2d_fwd(xd.data_ptr(), wd.data_ptr(), packed, b, y.data_ptr(), ctypes.byref(g), dt, _ffi.NHWC, *wsa))
        outs.append(U.host(y))
    check(outs[0], y_ref, dtype, 'deconv fwd, bias, pre-packed')
    check(outs[1], y_ref - bias, dtype, 'deconv fwd, no bias, packed per call')
    assert np.array_equal(outs[0], outs[2]), 'a repeated call is not bit-identical'
    g.tile = 0
    for b, ref in ((bd.data_ptr(), y_ref), (0, y_ref - bias)):      # the dispatcher's own choice (it depends on the bias: csrc/deconv.hip dc_routed)
        y = nan((N, OH, OW, Cb), U.TDT[dtype])
        _ffi.check(lib.mcn_deconv2d_fwd(xd.data_ptr(), wd.data_ptr(), 0, b, y.data_ptr(), ctypes.byref(g), dt, _ffi.NHWC, *wsa))
        check(U.host(y), ref, dtype, 'deconv fwd, default dispatch, bias {}'.format(bool(b)))
    dx = nan((N, h, w, Cs), U.TDT[dtype])
    _ffi.check(lib.mcn_deconv2d_dgrad(dyd.data_ptr(), wd.data_ptr(), 0, 0, dx.data_ptr(), ctypes.byref(g), dt, _ffi.NHWC, *wsa))
    check(U.host(dx), dx_ref, dtype, 'deconv dgrad')
    grads = []
    for _ in range(2):
        dw, db = nan((KH, KW, Cs, Cb), torch.float32), nan((Cb,), torch.float32)
        _ffi.check(lib.mcn_deconv2d_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), ctypes.byref(g), 0.5, dt, _ffi.NHWC, *wsa))
        grads.append((U.host(dw), U.host(db)))
    check(grads[0][0], 0.5 * dw_ref, dtype, 'deconv wgrad', rel=2e-5 if dtype == 'float32' else 2e-3)
    check(grads[0][1], 0.5 * db_ref, dtype, 'deconv dbias', rel=2e-5 if dtype == 'float32' else 2e-3)
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1]), 'a repeated wgrad is not bit-identical'


def test_deconv_layer_case_on_gpu():
    import myconvnet_amd as M
    run_case(M, check)
