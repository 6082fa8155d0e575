"""Grouped batch normalisation without a GPU: argument validation of mcn_gbn_* (no launch), and the host code of norm_type='grouped_batch'
(dispatch, graph node, fusion, lowering, running statistics, moving-statistics inference) on libmcn_cpu.so in a fresh process
(tests/gbn_case.py)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fwd(lib, x=1, M=32, C=64, P=8, act=0, dtype=0, residual=0, ws=1, ws_bytes=1 << 40):
    return lib.mcn_gbn_fwd_train(x, 0, 0, residual, 1, 1, 1, 0, 0, 0, 0, 0.99, M, C, P, 1e-3, act, dtype, ws, ws_bytes, 0)


def _bwd(lib, x=1, M=32, C=64, P=8, act=0, dtype=0, residual=0, ws=1, ws_bytes=1 << 40):
    return lib.mcn_gbn_bwd(1, x, 1, 0, 0, 1, 1, 1, residual, 0, 0, 1.0, M, C, P, act, dtype, ws, ws_bytes, 0)


def test_gbn_argument_validation_without_gpu():
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    for call in (_fwd, _bwd):
        assert call(lib, C=60, P=8) == _ffi.E_BADARG                                    # C % P != 0
        assert call(lib, C=24, P=3) == _ffi.E_UNSUPPORTED and 'chunk' in _ffi.last_error()
        assert call(lib, dtype=7) == _ffi.E_UNSUPPORTED
        assert call(lib, act=_ffi.ACT_SIGMOID) == _ffi.E_UNSUPPORTED
        assert call(lib, act=_ffi.ACT_SWISH, residual=1) == _ffi.E_UNSUPPORTED
        assert call(lib, ws_bytes=16) == _ffi.E_WORKSPACE and call(lib, ws=0) == _ffi.E_WORKSPACE
        assert call(lib, x=0) == _ffi.E_BADARG                                          # NULL x
    assert lib.mcn_gbn_workspace_bytes(256 * 49, 2048, 8) >= 2 * 2048 * 4 and lib.mcn_gbn_workspace_bytes(0, 64, 8) == 0


def test_grouped_batch_norm_host_code_on_the_cpu_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_mcn_build_gbn', os.path.join(ROOT, 'myconvnet_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    env = dict(os.environ, MCN_LIB_PATH=mod.build_cpu(), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gbn_case.py')], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    assert r.stdout.splitlines()[-1] == 'grouped batch norm layer case ok', r.stdout
