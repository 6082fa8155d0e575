#!/usr/bin/env python3
"""Grouped batch norm (P channels per group) against batch norm on the same buffers: us per call of mcn_gbn_fwd_train + mcn_gbn_bwd beside
mcn_bn_fwd_train + mcn_bn_bwd (the unfused entry points), no activation, no residual.  Both move 3*M*C*e bytes forward (2R + 1W) and 5*M*C*e
backward.  Device events around CALLS back-to-back calls, ROUNDS rounds with the two forms alternated inside every round, median of the round
means (min .. max), warmed up.
usage: python3 profiles/gbn_bandwidth.py [batch=256] [P=8] [out.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myconvnet_amd import _ffi  # noqa: E402

lib = _ffi.lib
SHAPES = [(56, 256), (14, 1024)]
EPS, ROUNDS, CALLS = 1e-3, 7, 20


def timed(variants):
    sp = torch.cuda.current_stream().cuda_stream
    for f in variants.values():
        for _ in range(3):
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


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    out = ['# grouped batch norm (P = %d) against batch norm, bf16, N = %d, build %s; us per call: median (min .. max) of %d rounds x %d calls, TB/s of 3 / 5 x M*C*2 bytes'
           % (P, N, lib.mcn_build_id().decode()[:12], ROUNDS, CALLS)]
    dev, dt = 'cuda:0', _ffi.BF16
    for hw, C in SHAPES:
        M = N * hw * hw
        x = (torch.randn(M, C, device=dev) * 2 + 3).to(torch.bfloat16)
        dy = torch.randn(M, C, device=dev).to(torch.bfloat16)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        gamma, beta, dgm, dbt, sm, si, bm, bv, gsm, gsi = f32(C) + 1.5, f32(C) + 0.25, f32(C), f32(C), f32(C), f32(C), f32(C), f32(C), f32(C // P), f32(C // P)
        ws = torch.zeros(max(int(lib.mcn_gbn_workspace_bytes(M, C, P)), int(lib.mcn_bn_workspace_bytes(M, C))) // 4 + 64, dtype=torch.float32, device=dev)
        wp, wb = ws.data_ptr(), ws.numel() * 4
        p = lambda t: t.data_ptr()
        fwd = {'gbn': lambda s: lib.mcn_gbn_fwd_train(p(x), p(gamma), p(beta), 0, p(y), p(gsm), p(gsi), p(bm), p(bv), 0, 0, 0.99, M, C, P, EPS, 0, dt, wp, wb, s),
               'bn': lambda s: lib.mcn_bn_fwd_train(p(x), p(gamma), p(beta), 0, p(y), 0, p(sm), p(si), p(bm), p(bv), 0, 0, 0.99, M, C, EPS, 0, dt, wp, wb, s)}
        bwd = {'gbn': lambda s: lib.mcn_gbn_bwd(p(dy), p(x), 0, p(gamma), p(beta), p(gsm), p(gsi), p(dx), 0, p(dgm), p(dbt), 1.0, M, C, P, 0, dt, wp, wb, s),
               'bn': lambda s: lib.mcn_bn_bwd(p(dy), p(x), 0, 0, p(gamma), p(beta), p(sm), p(si), p(dx), 0, p(dgm), p(dbt), 1.0, M, C, 0, dt, wp, wb, s)}
        for name, variants, units in (('fwd', fwd, 3), ('bwd', bwd, 5)):
            t = timed(variants)
            out.append('  %3dx%-3d %-5d %s  ' % (hw, hw, C, name) + '   '.join('%s %7.1f (%7.1f .. %7.1f) %5.2f TB/s' % ((k,) + t[k] + (units * M * C * 2 / t[k][0] / 1e6,))
                                                                             for k in ('gbn', 'bn')))
            print(out[-1], flush=True)
    text = '\n'.join(out) + '\n'
    if len(sys.argv) > 3:
        with open(sys.argv[3], 'w') as fh:
            fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
