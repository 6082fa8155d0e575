"""Weight standardisation without a GPU: argument validation of mcn_ws_* (no launch), the host code of conv_layer(ws=True) (shared w_hat / stats
stores, prepack and backward launch lists, EMA inference) on libmcn_cpu.so in a fresh process (tests/ws_case.py), and the ResNet-WSGN model file's graph."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_argument_validation_without_gpu():
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    jobs = lambda *kc: (_ffi.WsJob * len(kc))(*[_ffi.WsJob(16, 16, 16, k, c) for k, c in kc])
    buf, nd = ctypes.create_string_buffer(1 << 20), ctypes.c_int32(-1)
    build = lambda j, n, b=ctypes.cast(buf, ctypes.c_void_p), nb=1 << 20: lib.mcn_ws_table_build(j, n, b, nb, ctypes.byref(nd))
    assert build(jobs((1, 64)), 1) == _ffi.E_BADARG and 'K = 1' in _ffi.last_error()
    assert build((_ffi.WsJob * 1)(_ffi.WsJob(16, 0, 16, 9, 4)), 1) == _ffi.E_BADARG and build(jobs((9, 4)), 1, b=None) == _ffi.E_BADARG
    big = jobs((9, 4), (4608, 40), (300, 6), (333, 1))
    assert build(big, 4, nb=lib.mcn_ws_table_bytes(big, 4) - 1) == _ffi.E_WORKSPACE
    for j, n in ((big, 4), (jobs((64, 256)), 1)):           # table_bytes is an upper bound of what table_build writes: a canary right behind it survives
        nb = int(lib.mcn_ws_table_bytes(j, n))
        assert 0 < nb < (1 << 20) - 8
        buf[nb:nb + 8] = b'\xa5' * 8
        assert build(j, n, nb=nb) == _ffi.OK and nd.value >= n and buf[nb:nb + 8] == b'\xa5' * 8
    need = int(lib.mcn_ws_fwd_workspace_bytes(big, 4))
    assert build(big, 4) == _ffi.OK and lib.mcn_ws_fwd_run(0, nd.value, 1e-5, 16, need, 0) == _ffi.E_BADARG
    assert lib.mcn_ws_fwd_run(16, nd.value, 1e-5, 0, need, 0) == _ffi.E_WORKSPACE and lib.mcn_ws_fwd_run(16, nd.value, 1e-5, 16, need - 1, 0) == _ffi.E_WORKSPACE
    bwd = lambda dwh=16, wh=16, st=16, dw=16, K=64, C=64, ws=16, nb=1 << 30: lib.mcn_ws_bwd(dwh, wh, st, dw, K, C, 1e-5, ws, nb, 0)
    assert bwd(K=1) == _ffi.E_BADARG and 'K = 1' in _ffi.last_error()
    assert bwd(dwh=0) == bwd(wh=0) == bwd(st=0) == bwd(dw=0) == _ffi.E_BADARG
    assert bwd(ws=0) == _ffi.E_WORKSPACE and bwd(K=4608, C=512, nb=lib.mcn_ws_bwd_workspace_bytes(4608, 512) - 1) == _ffi.E_WORKSPACE


def test_ws_host_code_on_the_cpu_library():
    from myconvnet_amd import _ffi
    env = dict(os.environ, MCN_LIB_PATH=_ffi._build_module().build_cpu(), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'ws_case.py')], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    assert r.stdout.splitlines()[-1] == 'weight standardisation layer case ok', r.stdout


def test_resnet50_wsgn_graph():
    import myconvnet_amd as M
    kw = dict(batch_size=2, auto_compile=False, num_gpus=1)
    net, bn_net = M.resnet_v1_5_wsgn.ResNet50([32, 32, 3], 10, **kw), M.ResNet50([32, 32, 3], 10, **kw)
    convs = [n for n in net.graph.nodes if n.op == 'conv']
    assert len(convs) == 53 and all(n.attrs['ws'] and n.attrs['b'] is None for n in convs)
    ops = [n.op for n in net.graph.nodes]
    assert ops.count('gn') == 53 and 'bn' not in ops and all(n.attrs['groups'] == 32 for n in net.graph.nodes if n.op == 'gn')
    assert {'block_0/conv_0/weights', 'block_1/res_0/conv_1/weights', 'block_1/res_0/conv_1/bn/gamma', 'block_1/res_0/conv_skip/bn/beta', 'block_4/res_2/conv_2/bn/gamma',
            'block_None/logits/weights'} <= set(net.variables)
    assert float(net.variables['block_4/res_2/conv_2/bn/gamma'].init((4,), None).sum()) == 0.0          # zero_scale_init on conv_2's norm
    weights = lambda m: {k: v.shape for k, v in m.variables.items() if k.endswith('/weights')}
    assert weights(net) == weights(bn_net)


def test_depthwise_and_fc_ws_still_raise():
    import myconvnet_amd as M
    net = M.ResNet18([32, 32, 3], 10, batch_size=2, auto_compile=False, num_gpus=1)          # (any built model: the block methods are then callable)
    with pytest.raises(NotImplementedError, match='depthwise'):
        net.conv_layer(net.X, 3, 1, depthwise=True, ws=True)
    with pytest.raises(NotImplementedError, match='fc_layer'):
        net.fc_layer(net.global_avg_pool(net.X), 10, ws=True)
