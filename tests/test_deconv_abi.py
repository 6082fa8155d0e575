"""Transposed convolution without a GPU: argument validation of mcn_deconv2d_* (no launch), the host code of ConvNet.transposed_conv_layer
(graph node, lowering, derived filter copies, EMA inference) on libmcn_cpu.so in a fresh process (tests/deconv_case.py), and the layer's
variables and errors."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40


def test_deconv_argument_validation_without_gpu():
    from myconvnet_amd import _ffi
    lib = _ffi.lib

    def geom(OH=8, pads=(1, 2, 1, 2), d=1, s=2, tile=0, cs=128):
        return ctypes.byref(_ffi.conv_geom(2, OH, 8, 24, cs, 5, 5, s, s, d, d, pads, 0, tile))
    fwd = lambda x=1, g=None, dt=0: lib.mcn_deconv2d_fwd(x, 1, 0, 0, 1, g or geom(), dt, 0, 0, 0, 0)
    dgrad = lambda dy=1, g=None, ws=1, wb=BIG: lib.mcn_deconv2d_dgrad(dy, 1, 0, 0, 1, g or geom(), 0, 0, ws, wb, 0)
    wgrad = lambda x=1, g=None, ws=1, wb=BIG: lib.mcn_deconv2d_wgrad(x, 1, 1, 0, g or geom(), 1.0, 0, 0, ws, wb, 0)
    for call in (fwd, dgrad, wgrad):
        assert call(0) == _ffi.E_BADARG                                                       # NULL tensor
        assert call(g=geom(OH=11)) == _ffi.E_BADARG and 'height' in _ffi.last_error()         # SAME pads of 8 do not map 11 rows back to 4
        assert call(g=geom(d=2)) == _ffi.E_UNSUPPORTED
    assert fwd(dt=7) == _ffi.E_UNSUPPORTED
    assert dgrad(wb=16) == _ffi.E_WORKSPACE and wgrad(wb=16) == _ffi.E_WORKSPACE and wgrad(ws=0) == _ffi.E_WORKSPACE
    if not _ffi.IS_CPU_LIB:                                                                   # (the CPU library packs nothing)
        assert lib.mcn_deconv2d_packed_bytes(geom(tile=1), _ffi.BF16) == 24 * 25 * 256 and lib.mcn_deconv2d_packed_bytes(geom(), _ffi.BF16) == 0
        assert lib.mcn_deconv2d_packed_bytes(geom(cs=16), _ffi.BF16) == 24 * 25 * 128 and lib.mcn_deconv2d_packed_bytes(geom(cs=16, tile=2), _ffi.BF16) == 0      # (light: 100 MACs per output)
        assert lib.mcn_deconv2d_packed_bytes(geom(OH=7, pads=(1, 1, 1, 1), s=3), 0) == 0
        assert fwd() == _ffi.E_WORKSPACE and fwd(g=geom(tile=1)) == _ffi.E_WORKSPACE               # per-call swap / packing without room
    assert lib.mcn_deconv2d_workspace_bytes(_ffi.CONV_WGRAD, geom(), 0) >= 25 * 24 * 128 * 4 and lib.mcn_deconv2d_workspace_bytes(_ffi.CONV_WGRAD, geom(OH=11), 0) == 0
    assert lib.mcn_filter_swap_io(1, 1, 9, 4, 4, 1.0, 0) == _ffi.E_BADARG                     # in place


def test_deconv_host_code_on_the_cpu_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_mcn_build_deconv', os.path.join(ROOT, 'myconvnet_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    env = dict(os.environ, MCN_LIB_PATH=mod.build_cpu(), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'deconv_case.py')], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    assert r.stdout.splitlines()[-1] == 'deconv layer case ok', r.stdout


def test_transposed_conv_layer_variables_and_errors():
    import myconvnet_amd as M
    made = {}

    class Net(M.ConvNet):
        def _init_params(self, **kwargs):
            pass

        def _build_model(self):
            self._curr_block = 0
            x = self.conv_layer(self.X, 3, 2, 8, scope='c')                                   # 8 x 8 -> 4 x 4
            made['same'] = self.transposed_conv_layer(x, 5, 2, 6, scope='a')
            made['odd'] = self.transposed_conv_layer(x, [3, 3], [2], 6, biased=False, output_shape=[None, 7, 8, 6], scope='b')
            made['valid'] = self.transposed_conv_layer(x, 2, 2, 6, padding='VALID', output_shape=(8, 8), scope='v')
            for kw in (dict(output_shape=(9, 8)), dict(padding='VALID'), dict(padding='VALID', output_shape=(8, 8))):
                with pytest.raises(ValueError):
                    self.transposed_conv_layer(x, 3, 2, 6, scope='bad', **kw)
            for kw in (dict(dilation=2), dict(ws=True)):
                with pytest.raises(NotImplementedError):
                    self.transposed_conv_layer(x, 3, 2, 6, scope='bad', **kw)
            made['valid3'] = self.transposed_conv_layer(x, 3, 2, 6, padding='VALID', output_shape=(9, 10), scope='v3')
            return {'block_0': made['same']}
    m = Net([8, 8, 3], 10, batch_size=2, backbone_only=True, num_gpus=1, auto_compile=False)
    assert {k: v.shape for k, v in made.items()} == {'same': (2, 8, 8, 6), 'odd': (2, 7, 8, 6), 'valid': (2, 8, 8, 6), 'valid3': (2, 9, 10, 6)}
    shapes = {k: v.shape for k, v in m.variables.items()}
    assert shapes['a/weights'] == (5, 5, 8, 6) and shapes['a/biases'] == (6,) and shapes['b/weights'] == (3, 3, 8, 6) and 'b/biases' not in shapes
    info = [i for i in m._layer_info if i['name'] == 'a'][0]
    assert info['flops'] == 8 * 8 * 25 * 8 * 6 + 8 * 8 * 6 and info['params'] == 25 * 8 * 6 + 6 and info['nodes'] == 8 * 8 * 6
