#!/usr/bin/env python3
"""The phase-fused transposed convolution (myconvnet_amd/csrc/deconv.hip) against the route the library offered before it for the same result —
mcn_conv2d_dgrad on the filter with its channel axes swapped, one GEMM launch per stride-parity class — on the four 5x5/2 layers of the
DCGAN generator (models/dcgan.py:86) and one 3x3/2 64 -> 64 layer, BIASED (a third argument `nobias`: unbiased).  Three columns: `fused` = mcn_deconv2d_fwd with tile = 1 (pre-packed operand,
bias in the epilogue); `routed` = the other route of mcn_deconv2d_fwd (tile = 2), all of it: the per-call filter swap, mcn_conv2d_dgrad with its
per-call pack, and the bias pass over the output; `dgrad` = the bare mcn_conv2d_dgrad on a pre-swapped filter, no bias (the floor of that route).  Device events around CALLS back-to-back calls, ROUNDS
rounds with the routes alternated inside every round; median, minimum and maximum of the round means (the spread), warmed up.  Fractions:
2 * N*h*w*taps*Cs*Cb flop against the dense MFMA peak of the type (fp32 157.3, bf16 / fp16 2500 TFLOP/s); TB/s of one read of x + one write of y.
usage: python3 profiles/deconv_bandwidth.py [batch=256] [out.txt]   ->  the table (committed as profiles/deconv_kernel_bandwidth.txt)"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myconvnet_amd import _ffi  # noqa: E402

lib = _ffi.lib
NOBIAS = len(sys.argv) > 3 and sys.argv[3] == 'nobias'
LAYERS = [(4, 512, 256, 5), (8, 256, 128, 5), (16, 128, 64, 5), (32, 64, 3, 5), (32, 64, 64, 3)]      # (h = w, Cs, Cb, k), stride 2, SAME
ROUNDS, CALLS = 5, 4
TDT = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float16': torch.float16}
MDT = {'float32': _ffi.F32, 'bfloat16': _ffi.BF16, 'float16': _ffi.F16}
PEAK = {'float32': 157.3, 'bfloat16': 2500.0, 'float16': 2500.0}


def timed(variants):
    sp = torch.cuda.current_stream().cuda_stream
    for f in variants.values():
        for _ in range(2):
            _ffi.check(f(sp))
    torch.cuda.synchronize()
    means = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                _ffi.check(f(sp))
            e1.record()
            e1.synchronize()
            means[k].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in means.items()}


def layer_row(N, h, Cs, Cb, k, dtype):
    dev, dt, OH = 'cuda:0', MDT[dtype], 2 * h
    total = max((h - 1) * 2 + k - OH, 0)
    pads = (total // 2, total - total // 2) * 2
    g = _ffi.conv_geom(N, OH, OH, Cb, Cs, k, k, 2, 2, 1, 1, pads)
    gf = _ffi.conv_geom(N, OH, OH, Cb, Cs, k, k, 2, 2, 1, 1, pads, 0, 1)         # tile = 1: the fused kernel whatever the dispatcher's default
    bias = torch.randn(Cb, device=dev)
    bp = 0 if NOBIAS else bias.data_ptr()
    gr = _ffi.conv_geom(N, OH, OH, Cb, Cs, k, k, 2, 2, 1, 1, pads, 0, 2)         # tile = 2: the conv-kernel route whatever the dispatcher's default
    x = torch.randn((N, h, h, Cs), device=dev).to(TDT[dtype])
    y = torch.empty((N, OH, OH, Cb), dtype=TDT[dtype], device=dev)
    w = torch.randn((k, k, Cs, Cb), device=dev) * 0.05
    wsw = torch.empty((k, k, Cb, Cs), device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    _ffi.check(lib.mcn_filter_swap_io(w.data_ptr(), wsw.data_ptr(), k * k, Cs, Cb, 1.0, sp))
    pk = torch.zeros(max(int(lib.mcn_deconv2d_packed_bytes(ctypes.byref(gf), dt)), 1), dtype=torch.uint8, device=dev)
    _ffi.check(lib.mcn_deconv2d_pack(w.data_ptr(), pk.data_ptr(), ctypes.byref(gf), dt, sp))
    nb = max(int(lib.mcn_conv2d_workspace_bytes(_ffi.CONV_DGRAD, ctypes.byref(g), dt)), int(lib.mcn_deconv2d_workspace_bytes(_ffi.CONV_FWD, ctypes.byref(gf), dt)),
             int(lib.mcn_deconv2d_workspace_bytes(_ffi.CONV_FWD, ctypes.byref(g), dt)), 256)
    ws = torch.zeros(nb // 4 + 64, dtype=torch.float32, device=dev)
    name = ctypes.create_string_buffer(128)
    launches = lib.mcn_conv2d_kernel_name(_ffi.CONV_DGRAD, ctypes.byref(g), dt, name, 128)
    variants = {
        'fused': lambda s: lib.mcn_deconv2d_fwd(x.data_ptr(), w.data_ptr(), pk.data_ptr(), bp, y.data_ptr(), ctypes.byref(gf), dt, _ffi.NHWC, ws.data_ptr(), ws.numel() * 4, s),
        'routed': lambda s: lib.mcn_deconv2d_fwd(x.data_ptr(), w.data_ptr(), 0, bp, y.data_ptr(), ctypes.byref(gr), dt, _ffi.NHWC, ws.data_ptr(), ws.numel() * 4, s),
        'dgrad': lambda s: lib.mcn_conv2d_dgrad(x.data_ptr(), wsw.data_ptr(), 0, y.data_ptr(), ctypes.byref(g), 0, dt, _ffi.NHWC, ws.data_ptr(), ws.numel() * 4, s)}
    if Cb <= 16:                                             # (that route is naive_conv_dgrad there: the `dgrad` column)
        del variants['routed']
    res = timed(variants)
    flop, byt = 2.0 * N * h * h * k * k * Cs * Cb, (x.numel() + y.numel()) * x.element_size()
    cols = ['{:>8} {:>2}^2x{:<3}->{:>2}^2x{:<3} {}x{}/2'.format(dtype, h, Cs, OH, Cb, k, k)]
    for key in res:
        med, lo, hi = res[key]
        cols.append('{} {:8.1f} us ({:.1f}-{:.1f}) {:5.1f} % MFMA {:5.2f} TB/s'.format(key, med, lo, hi, 100 * flop / (med * 1e-6) / 1e12 / PEAK[dtype], byt / (med * 1e-6) / 1e12))
    cols.append('[{} x {}]'.format(launches, name.value.decode()[:40]))
    return '  '.join(cols)


if __name__ == '__main__':
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    lines = ['transposed convolution forward at N = {}: fused kernel, the dispatched wide route and bare mcn_conv2d_dgrad, {} layers (median us, min-max of {} rounds x {} calls)'.format(N, 'unbiased' if NOBIAS else 'biased', ROUNDS, CALLS)]
    for dtype in TDT:
        for lay in LAYERS:
            lines.append(layer_row(N, *lay, dtype))
            print(lines[-1], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            f.write('\n'.join(lines) + '\n')
