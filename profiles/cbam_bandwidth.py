#!/usr/bin/env python3
"""The CBAM attention-tail kernels (myconvnet_amd/csrc/cbam.hip) on the four block-output shapes of a ResNet-50: us per call and bytes over time of
every new entry point, beside the existing BN forward (mcn_bn_fwd_train: statistics pass + apply pass) on the same tensor in the same session.
Device events around CALLS back-to-back calls, ROUNDS rounds with the kernels of a shape alternated inside every round (ROUNDS * CALLS >= 20 calls per
figure, median of the round means, warmed up).  Bytes are the full-size tensors each call must move (M = N*H*W, e = element size, in units of
M*C*e): pools 1 (1R), chpool 1 (1R), apply 2 (1R + 1W), cbam_bwd 5 (reduce 2R, dx pass 2R + 1W), pool_bwd 3 (in place: 2R + 1W), bn_fwd 3 (2R + 1W);
the per-pixel and per-(image, channel) side tensors are not counted.
usage: python3 profiles/cbam_bandwidth.py [batch=256] [out.txt]   ->  the table (committed as profiles/cbam_kernel_bandwidth.txt)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myconvnet_amd import _ffi  # noqa: E402

lib = _ffi.lib
SHAPES = [(56, 256), (28, 512), (14, 1024), (7, 2048)]
K, ROUNDS, CALLS = 7, 5, 4
TDT = {'float32': torch.float32, 'bfloat16': torch.bfloat16}
MDT = {'float32': _ffi.F32, 'bfloat16': _ffi.BF16}
UNITS = [('pools', 1), ('chpool', 1), ('apply', 2), ('cbam_bwd', 5), ('pool_bwd', 3), ('bn_fwd', 3)]


def timed(variants):
    """{name: call} -> {name: median us per call} with the variants alternated inside every round"""
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
    return {k: sorted(v)[len(v) // 2] for k, v in means.items()}


def shape_row(N, hw, C, dtype):
    HW, M, dt, e = hw * hw, N * hw * hw, MDT[dtype], 4 if dtype == 'float32' else 2
    dev = 'cuda:0'
    x = torch.randn(N, hw, hw, C, device=dev).to(TDT[dtype])
    dy = torch.randn(N, hw, hw, C, device=dev).to(TDT[dtype])
    y, dx = torch.empty_like(x), torch.empty_like(x)
    lp = lambda *s: torch.rand(*s, device=dev).to(TDT[dtype])
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    cm, pools, dpool, dcm, s, sm = lp(N, C), lp(2, N, C), lp(2, N, C), lp(N, C), lp(N, hw, hw, 2), lp(N, hw, hw)
    w, b, dw, db, ties = f32(K, K, 2, 1) + 0.01, f32(1), f32(K, K, 2, 1), f32(1), f32(N, C)
    gamma, beta, bsm, bsi = f32(C) + 1.5, f32(C) + 0.25, f32(C), f32(C)
    nws = max(int(lib.mcn_cbam_workspace_bytes(N, hw, hw, C, K)), int(lib.mcn_global_avgmax_pool_workspace_bytes(N, HW, C)), int(lib.mcn_bn_workspace_bytes(M, C)))
    ws = torch.zeros(nws // 4 + 64, dtype=torch.float32, device=dev)
    wp, wb = ws.data_ptr(), ws.numel() * 4
    p = lambda t: t.data_ptr()
    variants = {
        'pools': lambda st: lib.mcn_global_avgmax_pool_fwd(p(x), p(pools), N, HW, C, dt, wp, wb, st),
        'chpool': lambda st: lib.mcn_cbam_chpool_fwd(p(x), p(cm), p(s), N, HW, C, dt, st),
        'apply': lambda st: lib.mcn_cbam_apply_fwd(p(x), p(cm), p(s), p(w), p(b), p(sm), p(y), N, hw, hw, C, K, dt, st),
        'cbam_bwd': lambda st: lib.mcn_cbam_bwd(p(dy), p(x), p(cm), p(s), p(sm), p(w), p(pools), p(dx), p(dcm), p(dw), p(db), p(ties), 1.0, N, hw, hw, C, K, dt, wp, wb, st),
        'pool_bwd': lambda st: lib.mcn_global_avgmax_pool_bwd(p(dpool), p(x), p(pools), p(ties), p(dx), 1, N, HW, C, dt, st),
        'bn_fwd': lambda st: lib.mcn_bn_fwd_train(p(x), p(gamma), p(beta), 0, p(y), 0, p(bsm), p(bsi), 0, 0, 0, 0, 0.99, M, C, 1e-3, 0, dt, wp, wb, st),
    }
    # real forward products first: the backward reads the s / sm / pools / ties the forward kernels left
    sp = torch.cuda.current_stream().cuda_stream
    for k in ('pools', 'chpool', 'apply', 'cbam_bwd'):
        _ffi.check(variants[k](sp))
    t = timed(variants)
    return '  %-8s %3dx%-3d %-5d' % (dtype, hw, hw, C) + ''.join('  %8.1f %5.2f' % (t[k], u * M * C * e / t[k] / 1e6) for k, u in UNITS)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    out = ['# CBAM attention tail (K = %d) against the BN forward, N = %d, build %s; us per call (median of %d rounds x %d calls, kernels alternated), TB/s of the full-size bytes'
           % (K, N, lib.mcn_build_id().decode()[:12], ROUNDS, CALLS),
           '# %-8s %-7s %-5s' % ('dtype', 'HxW', 'C') + ''.join('  %8s %5s' % (k, 'TB/s') for k, _ in UNITS)]
    for dtype in ('float32', 'bfloat16'):
        for hw, C in SHAPES:
            out.append(shape_row(N, hw, C, dtype))
            print(out[-1], flush=True)
    text = '\n'.join(out) + '\n'
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as fh:
            fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
