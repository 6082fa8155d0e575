#!/usr/bin/env python3
"""Weight standardisation kernels (csrc/ws.hip) on the filter shapes of a ResNet-50: the batched forward over all 53 filters as ONE table
(mcn_ws_fwd_run: us per run, bytes over time against 2*4*sum(K*C), 1R + 1W) and mcn_ws_bwd per distinct filter shape (us per call, bytes over time
against 3*4*K*C, 2R + 1W; out of place).  Device events around CALLS back-to-back calls, ROUNDS rounds, median of the round means, warmed up; the
backward shapes are alternated inside every round.
usage: python3 profiles/ws_bandwidth.py [out.txt]   ->  the table (committed as profiles/ws_kernel_bandwidth.txt)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myconvnet_amd import _ffi  # noqa: E402

lib = _ffi.lib
EPS, ROUNDS, CALLS = 1e-5, 7, 20


def resnet50_filters():
    """(K, C) of the 53 convolutions of ResNet-50 v1.5, in model order"""
    out, cin = [(7 * 7 * 3, 64)], 64
    for units, width in ((3, 256), (4, 512), (6, 1024), (3, 2048)):
        for j in range(units):
            mid = width // 4
            if cin != width:
                out.append((cin, width))                        # projection shortcut
            out += [(cin, mid), (9 * mid, mid), (mid, width)]
            cin = width
    return out


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


def main():
    dev = 'cuda:0'
    filters = resnet50_filters()
    assert len(filters) == 53
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    w = [torch.randn(K * C, device=dev) * 0.05 + 0.01 for K, C in filters]
    hat, stats = [f32(K * C) for K, C in filters], [f32(2 * C) for K, C in filters]
    table, ndesc, nbytes = _ffi.ws_table([_ffi.WsJob(a.data_ptr(), b.data_ptr(), c.data_ptr(), K, C) for a, b, c, (K, C) in zip(w, hat, stats, filters)])
    table = torch.frombuffer(table, dtype=torch.uint8).to(dev)
    ws = f32(nbytes // 4 + 64)
    total = sum(K * C for K, C in filters)
    t = timed({'fwd': lambda s: lib.mcn_ws_fwd_run(table.data_ptr(), ndesc, EPS, ws.data_ptr(), ws.numel() * 4, s)})['fwd']
    out = ['# weight standardisation, ResNet-50 filters, build %s; us (median of %d rounds x %d calls; min, max of the round means), TB/s of the bytes the form must move'
           % (lib.mcn_build_id().decode()[:12], ROUNDS, CALLS),
           '# batched forward: %d filters, %d descriptors, %.1f MB of fp32 weights, 2 launches, bytes = 2*4*sum(K*C)' % (len(filters), ndesc, total * 4 / 1e6),
           '  fwd  all-53        %9.1f us  (%.1f .. %.1f)  %6.2f TB/s' % (t[0], t[1], t[2], 2 * 4 * total / t[0] / 1e6),
           '# mcn_ws_bwd per distinct filter shape (count in the model), bytes = 3*4*K*C',
           '# %-4s %-12s %5s %10s %19s %7s' % ('dir', 'K x C', 'count', 'us', '(min .. max)', 'TB/s')]
    shapes = sorted(set(filters), key=lambda kc: (kc[0] * kc[1], kc))
    variants, keep = {}, []
    for K, C in shapes:
        i = filters.index((K, C))
        g, dw = torch.randn(K * C, device=dev), f32(K * C)
        wb = f32(int(lib.mcn_ws_bwd_workspace_bytes(K, C)) // 4 + 64)
        keep.append((g, dw, wb))
        variants[(K, C)] = (lambda s, g=g, dw=dw, wb=wb, i=i, K=K, C=C:
                            lib.mcn_ws_bwd(g.data_ptr(), hat[i].data_ptr(), stats[i].data_ptr(), dw.data_ptr(), K, C, EPS, wb.data_ptr(), wb.numel() * 4, s))
    tb = timed(variants)
    step = 0.0
    for K, C in shapes:
        us, lo, hi = tb[(K, C)]
        step += us * filters.count((K, C))
        out.append('  bwd  %-12s %5d %10.1f %19s %7.2f' % ('%dx%d' % (K, C), filters.count((K, C)), us, '(%.1f .. %.1f)' % (lo, hi), 3 * 4 * K * C / us / 1e6))
    out.append('# all 53 backward calls of a step, back to back: %.1f us (sum of the medians above)' % step)
    text = '\n'.join(out) + '\n'
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as fh:
            fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
