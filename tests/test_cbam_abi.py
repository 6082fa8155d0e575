"""The CBAM attention tail without a GPU: argument validation of mcn_cbam_* / mcn_global_avgmax_pool_* (no launch), the host code of
ConvNet.cbam_attention (graph nodes, lowering, backward routing, EMA inference) on libmcn_cpu.so in a fresh process (tests/cbam_case.py), and the
variable names and shapes of ResNetCBAM50 against the reference's (models/resnet_v2_d_cbam.py)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40


def test_cbam_argument_validation_without_gpu():
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    pool = lambda x=1, o=1, C=64, ws=1, wb=BIG: lib.mcn_global_avgmax_pool_fwd(x, o, 2, 16, C, 0, ws, wb, 0)
    chpool = lambda x=1, C=64, dt=0: lib.mcn_cbam_chpool_fwd(x, 1, 1, 2, 16, C, dt, 0)
    apply_ = lambda x=1, w=1, C=64, K=7: lib.mcn_cbam_apply_fwd(x, 1, 1, w, 1, 1, 1, 2, 4, 4, C, K, 0, 0)
    bwd = lambda dy=1, C=64, K=7, ws=1, wb=BIG, pools=0, ties=0: lib.mcn_cbam_bwd(dy, 1, 1, 1, 1, 1, pools, 1, 1, 0, 0, ties, 1.0, 2, 4, 4, C, K, 0, ws, wb, 0)
    for call in (pool, chpool, apply_):
        assert call(x=0) == _ffi.E_BADARG                                                     # NULL tensor
        assert call(C=6) == _ffi.E_UNSUPPORTED and 'chunk' in _ffi.last_error()
    assert bwd(dy=0) == _ffi.E_BADARG and apply_(w=0) == _ffi.E_BADARG and bwd(pools=1) == _ffi.E_BADARG      # (pools without ties)
    assert bwd(C=6) == _ffi.E_UNSUPPORTED and chpool(dt=7) == _ffi.E_UNSUPPORTED
    for call in (apply_, bwd):
        assert call(K=4) == _ffi.E_BADARG and call(K=9) == _ffi.E_BADARG and call(K=0) == _ffi.E_BADARG
    assert pool(wb=16) == _ffi.E_WORKSPACE and pool(ws=0) == _ffi.E_WORKSPACE and bwd(wb=16) == _ffi.E_WORKSPACE and bwd(ws=0) == _ffi.E_WORKSPACE
    assert lib.mcn_global_avgmax_pool_bwd(1, 1, 1, 0, 1, 0, 2, 16, 64, 0, 0) == _ffi.E_BADARG                 # no tie counts
    assert lib.mcn_cbam_workspace_bytes(2, 4, 4, 64, 7) >= 2 * 16 * 4 * 4 and lib.mcn_cbam_workspace_bytes(2, 4, 4, 64, 9) == 0


def test_cbam_host_code_on_the_cpu_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_mcn_build_cbam', os.path.join(ROOT, 'myconvnet_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    env = dict(os.environ, MCN_LIB_PATH=mod.build_cpu(), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'cbam_case.py')], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    assert r.stdout.splitlines()[-1] == 'cbam layer case ok', r.stdout


def test_resnet_cbam50_variables():
    import myconvnet_amd as M
    m = M.ResNetCBAM50([224, 224, 3], 1000, auto_compile=False)
    shapes = {k: v.shape for k, v in m.variables.items()}
    want = {'block_0/conv_0/weights': (3, 3, 3, 32), 'block_0/conv_2/weights': (3, 3, 32, 64), 'block_0/conv_2/bn/gamma': (64,),
            'block_None/logits/bn/gamma': (2048,), 'block_None/logits/weights': (2048, 1000), 'block_None/logits/biases': (1000,)}
    # one unit of each block: (in, out) widths; res_0 of every block projects its shortcut with a biased 1x1
    for blk, cin, c in ((1, 64, 256), (2, 256, 512), (3, 512, 1024), (4, 1024, 2048)):
        u = 'block_{}/res_0/'.format(blk)
        want.update({u + 'conv_skip/weights': (1, 1, cin, c), u + 'conv_skip/biases': (c,), u + 'conv_0/bn/gamma': (cin,), u + 'conv_0/weights': (1, 1, cin, c // 4),
                     u + 'conv_1/bn/mu': (c // 4,), u + 'conv_1/weights': (3, 3, c // 4, c // 4), u + 'conv_2/bn/beta': (c // 4,), u + 'conv_2/weights': (1, 1, c // 4, c),
                     u + 'conv_2/biases': (c,), u + 'channel_mask/fc1/weights': (c, c // 8), u + 'channel_mask/fc1/biases': (c // 8,),
                     u + 'channel_mask/fc2/weights': (c // 8, c), u + 'channel_mask/fc2/biases': (c,), u + 'spatial_mask/conv/weights': (7, 7, 2, 1),
                     u + 'spatial_mask/conv/biases': (1,)})
    assert {k: shapes.get(k) for k in want} == want
    assert 'block_1/res_1/conv_skip/weights' not in shapes and 'block_1/res_0/conv_0/biases' not in shapes
    assert sum(k.endswith('spatial_mask/conv/weights') for k in shapes) == 16 and m.d['block_4'].shape == (16, 7, 7, 2048)
    assert m.d['block_1/res_0/spatial_mask'].shape == (16, 56, 56, 1) and m.d['block_1/res_0/channel_mask'].shape == (16, 256)
