#!/usr/bin/env python3
"""Group norm kernels against the batch norm passes on the normalisation shapes of a ResNet-50 (G = 32): us per call and bytes over time of
mcn_gn_fwd / mcn_gn_bwd on both launch paths and with the library's own choice (path 0), beside mcn_bn_fwd_train / mcn_bn_bwd on the same tensors.
Device events around CALLS back-to-back calls, ROUNDS rounds with the variants of a shape alternated inside every round (ROUNDS * CALLS >= 20 calls per
figure, median of the round means, warmed up).  No activation, no residual.  Bytes are the ones each form must move (M = N*HW, e = element size):
forward two-pass and BN 3*M*C*e (2R + 1W), resident 2*M*C*e (1R + 1W); backward two-pass and BN 5*M*C*e (reduce 2R, apply 2R + 1W), resident 3*M*C*e.
usage: python3 profiles/gn_bandwidth.py [batch=256] [out.txt]   ->  the table (committed as profiles/gn_kernel_bandwidth.txt)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myconvnet_amd import _ffi  # noqa: E402

lib = _ffi.lib
SHAPES = [(112, 64), (56, 64), (56, 256), (28, 128), (28, 512), (14, 256), (14, 1024), (7, 512), (7, 2048)]
G, EPS, ROUNDS, CALLS = 32, 1e-3, 5, 4
TDT = {'float32': torch.float32, 'bfloat16': torch.bfloat16}
MDT = {'float32': _ffi.F32, 'bfloat16': _ffi.BF16}


def timed(variants):
    """{name: call} -> {name: (median us per call, min, max)} with the variants alternated inside every round"""
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


def shape_rows(N, hw, C, dtype):
    HW, M, dt, e = hw * hw, N * hw * hw, MDT[dtype], 4 if dtype == 'float32' else 2
    dev = 'cuda:0'
    x = (torch.randn(N, HW, C, device=dev) * 2 + 3).to(TDT[dtype])
    dy = torch.randn(N, HW, C, device=dev).to(TDT[dtype])
    y, dx = torch.empty_like(x), torch.empty_like(x)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    gamma, beta, dgm, dbt = f32(C) + 1.5, f32(C) + 0.25, f32(C), f32(C)
    sm, si, bsm, bsi = f32(N, G), f32(N, G), f32(C), f32(C)
    nws = max(int(lib.mcn_gn_workspace_bytes(N, HW, C, G)), int(lib.mcn_bn_workspace_bytes(M, C)))
    ws = torch.zeros(nws // 4 + 64, dtype=torch.float32, device=dev)
    wp, wb = ws.data_ptr(), ws.numel() * 4
    p = lambda t: t.data_ptr()
    gn_f = lambda path: (lambda s: lib.mcn_gn_fwd(p(x), p(gamma), p(beta), 0, p(y), p(sm), p(si), N, HW, C, G, EPS, 0, dt, path, wp, wb, s))
    gn_b = lambda path: (lambda s: lib.mcn_gn_bwd(p(dy), p(x), 0, p(gamma), p(sm), p(si), p(dx), 0, p(dgm), p(dbt), 1.0, N, HW, C, G, 0, dt, path, wp, wb, s))
    bn_f = lambda s: lib.mcn_bn_fwd_train(p(x), p(gamma), p(beta), 0, p(y), 0, p(bsm), p(bsi), 0, 0, 0, 0, 0.99, M, C, EPS, 0, dt, wp, wb, s)
    bn_b = lambda s: lib.mcn_bn_bwd(p(dy), p(x), 0, 0, p(gamma), p(beta), p(bsm), p(bsi), p(dx), 0, p(dgm), p(dbt), 1.0, M, C, 0, dt, wp, wb, s)
    rows = []
    for direction, gn, bn, units in (('fwd', gn_f, bn_f, (3, 2)), ('bwd', gn_b, bn_b, (5, 3))):
        variants = {'two-pass': gn(_ffi.GN_TWO_PASS), 'bn': bn, 'auto': gn(0)}
        if lib.mcn_gn_resident_ok(1 if direction == 'bwd' else 0, N, HW, C, G, dt):
            variants['resident'] = gn(_ffi.GN_RESIDENT)
        t = timed(variants)
        tb = lambda k, u: u * M * C * e / t[k][0] / 1e6 if k in t else float('nan')
        us = lambda k: t[k][0] if k in t else float('nan')
        best = min((k for k in ('two-pass', 'resident') if k in t), key=lambda k: t[k][0])
        auto = min((k for k in ('two-pass', 'resident') if k in t), key=lambda k: abs(t[k][0] - t['auto'][0]))
        rows.append('  %-8s %4dx%-4d %-5d %s  %8.1f %6.2f  %8.1f %6.2f  %8.1f %6.2f  %8.1f  %-9s %s' % (
            dtype, hw, hw, C, direction, us('two-pass'), tb('two-pass', units[0]), us('resident'), tb('resident', units[1]), us('bn'), tb('bn', units[0]),
            us('auto'), best, auto))
    return rows


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    out = ['# group norm (G = %d) against batch norm, N = %d, build %s; us per call (median of %d rounds x %d calls, variants alternated), TB/s of the bytes the form must move'
           % (G, N, lib.mcn_build_id().decode()[:12], ROUNDS, CALLS),
           '# %-8s %-9s %-5s %s  %8s %6s  %8s %6s  %8s %6s  %8s  %-9s %s' % ('dtype', 'HxW', 'C', 'dir', 'two-pass', 'TB/s', 'resident', 'TB/s', 'bn', 'TB/s', 'path 0', 'fastest', 'path 0 ran')]
    for dtype in ('float32', 'bfloat16'):
        for hw, C in SHAPES:
            out += shape_rows(N, hw, C, dtype)
            print('\n'.join(out[-2:]), flush=True)
    text = '\n'.join(out) + '\n'
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as fh:
            fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
