"""Group normalisation without a GPU: argument validation and the path query of mcn_gn_* (no launch), and the host code of ConvNet.group_norm
(graph node, fusion, lowering, saved statistics, EMA inference) on libmcn_cpu.so in a fresh process (tests/gn_case.py)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fwd(lib, x=1, N=2, HW=16, C=64, G=32, act=0, dtype=0, path=0, ws=1, ws_bytes=1 << 40):
    return lib.mcn_gn_fwd(x, 0, 0, 0, 1, 0, 0, N, HW, C, G, 1e-3, act, dtype, path, ws, ws_bytes, 0)


def _bwd(lib, N=2, HW=16, C=64, G=32, act=0, dtype=0, path=0, ws=1, ws_bytes=1 << 40):
    return lib.mcn_gn_bwd(1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1.0, N, HW, C, G, act, dtype, path, ws, ws_bytes, 0)


def test_gn_argument_validation_without_gpu():
    from myconvnet_amd import _ffi
    lib = _ffi.lib
    big = dict(N=1, HW=112 * 112, C=64, G=32)               # 12544 pixels x 128 bytes = 1.6 MB at the narrowest legal block: above any LDS
    assert lib.mcn_gn_resident_ok(0, 1, 112 * 112, 64, 32, _ffi.F32) == 0 and lib.mcn_gn_resident_ok(1, 1, 112 * 112, 64, 32, _ffi.F32) == 0
    assert lib.mcn_gn_resident_ok(0, 256, 28 * 28, 128, 32, _ffi.F32) == 1 and lib.mcn_gn_resident_ok(1, 256, 28 * 28, 128, 32, _ffi.F32) == 0      # two slabs: half the budget
    for call in (_fwd, _bwd):
        assert call(lib, path=_ffi.GN_RESIDENT, **big) == _ffi.E_UNSUPPORTED and 'LDS' in _ffi.last_error()
        assert call(lib, C=48, G=32) == _ffi.E_BADARG                                   # C % G != 0
        assert call(lib, C=6, G=3) == _ffi.E_UNSUPPORTED and 'chunk' in _ffi.last_error()
        assert call(lib, act=_ffi.ACT_SWISH) == _ffi.E_UNSUPPORTED
        assert call(lib, dtype=7) == _ffi.E_UNSUPPORTED
        assert call(lib, ws_bytes=16) == _ffi.E_WORKSPACE and call(lib, ws=0) == _ffi.E_WORKSPACE
    assert _fwd(lib, x=0) == _ffi.E_BADARG                                               # NULL x
    assert lib.mcn_gn_bwd(1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 1.0, 2, 16, 64, 32, _ffi.ACT_RELU, 0, 0, 1, 1 << 40, 0) == _ffi.E_BADARG      # ReLU without the stored y
    assert lib.mcn_gn_workspace_bytes(256, 49, 2048, 32) >= 2 * 256 * 2048 * 4


def test_group_norm_host_code_on_the_cpu_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_mcn_build_gn', os.path.join(ROOT, 'myconvnet_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    env = dict(os.environ, MCN_LIB_PATH=mod.build_cpu(), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gn_case.py')], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    assert r.stdout.splitlines()[-1] == 'group norm layer case ok', r.stdout
