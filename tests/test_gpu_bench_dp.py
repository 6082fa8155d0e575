"""The N>1 path of bench.py executed once per round on the one-GPU box: `bench.py --gpus 2` launched exactly as the driver
launches it (`python -m torch.distributed.run --nproc-per-node 2 ...`, fresh child processes, rendezvous on 127.0.0.1),
both ranks on GPU 0 (MCN_BENCH_DEVICE=0) with the gloo backend standing in for RCCL (two ranks cannot share one device
under RCCL).  Asserts the contract: ONE JSON line from rank 0 with n_gpus 2, whole-job images/sec, weak scaling."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('ranks,batch', [(2, 64), (4, 16)])
def test_bench_n_ranks_prints_one_json_line(ranks, batch):
    """(4 ranks: the driver's N = 4 command line on the one GPU; six GPU processes are the box's limit, so N = 8 is rehearsed on the CPU
    only — tests/test_dist_gloo.py)"""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MCN_BENCH_DEVICE='0', MCN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', str(ranks), '--steps', '3', '--warmup', '1', '--dtype', 'bf16',
           '--batch', str(batch)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out['n_gpus'] == ranks and out['steps'] == 3 and out['warmup'] == 1 and out['scaling'] == 'weak'
    assert out['config']['global_batch'] == ranks * batch and out['config']['parallelism'] == 'dp{}'.format(ranks)
    assert out['value'] > 0 and abs(out['value'] - ranks * batch * 3 / (out['ms_per_step'] * 3e-3)) <= 0.01 * out['value']
    assert 'roofline' not in out and 'cpu_baseline' not in out            # N=1-only objects


def test_bench_without_a_launcher_spawns_its_own_ranks():
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment (it used to die on an assertion): the parent
    starts two fresh rank processes before touching the GPU itself, rank 0 prints the one JSON line, the exit code is the ranks'."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MCN_BENCH_DEVICE='0', MCN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--dtype', 'bf16', '--batch', '32']
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['config']['global_batch'] == 64 and out['config']['parallelism'] == 'dp2' and out['value'] > 0
    # a failing rank fails the parent (bad flag -> argparse exits 2 in every rank)
    r = subprocess.run(cmd + ['--no-such-flag'], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0


@pytest.mark.parametrize('dtype', ['fp32', 'fp16'])
def test_bench_single_gpu_line_carries_the_roofline_object(dtype):
    """The N=1 contract: one JSON line with metric / value / ms_per_step and a `roofline` object whose bound follows the dominant
    kernel's arithmetic intensity (short run at B=32 with --full, which is what measures the object; `cpu_baseline` and the secondary
    workloads are switched off here — `python bench.py --full` adds them)."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--full', '--steps', '5', '--warmup', '1', '--batch', '32', '--dtype', dtype, '--no-secondary', '--no-cpu-baseline']
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out['n_gpus'] == 1 and out['steps'] == 5 and out['unit'] == 'images/sec' and out['higher_is_better'] is True
    assert out['dtype'] == {'fp32': 'f32', 'fp16': 'f16'}[dtype] and out['vs_baseline'] is None and out['data'] == 'synthetic'
    assert abs(out['value'] - 32 * 5 / (out['ms_per_step'] * 5e-3)) <= 0.01 * out['value']
    rf = out['roofline']
    assert rf['bound'] in ('mfma', 'hbm') and rf['unit'] == ('TFLOP/s' if rf['bound'] == 'mfma' else 'GB/s')
    assert rf['kernel'].startswith('conv_gemm_') and rf['launches_per_step'] > 0 and rf['avg_launch_us'] > 0
    assert 0.0 < rf['frac'] <= 1.0 and abs(rf['frac'] - rf['achieved'] / rf['peak']) <= 2e-3
    assert rf['kernel'] in out['roofline_by_kernel'] and out['kernel_ms_total'] > 0
    # utilisation from EXECUTED flop (Winograd layers in fp32) beside the direct-convolution equivalent; the reference's per-step fetch
    assert 0.0 < out['e2e_mfma_frac'] <= out['direct_equivalent_frac'] and out['executed_flop_per_image'] <= out['train_flop_per_image']
    assert (out['executed_flop_per_image'] < out['train_flop_per_image']) == (dtype == 'fp32')
    assert out['config']['fetch'] is False and out['fetch_true']['value'] > 0.0


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline figure only (no instrumented pass, no secondaries, no CPU baseline), and
    --dump-outputs DIR leaves what the last timed step returned (loss, y_true, y_pred) as float32 .npy files."""
    import numpy as np
    out_dir = str(tmp_path / 'dump')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '8', '--dump-outputs', out_dir]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out['steps'] == 2 and out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert abs(out['value'] - 8 / (out['ms_per_step'] * 1e-3)) <= 0.01 * out['value']
    for key in ('roofline', 'roofline_by_kernel', 'kernel_ms_per_step', 'fetch_true', 'bf16', 'fp16', 'efficientnet_b0_bf16', 'deeplabv3plus_bf16', 'cpu_baseline'):
        assert key not in out, key
    got = {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    assert sorted(got) == ['loss.npy', 'y_pred.npy', 'y_true.npy']
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got['y_pred.npy'].shape == (8, 1000) and got['y_true.npy'].shape == (8, 1000)
    np.testing.assert_allclose(got['y_pred.npy'].sum(-1), 1.0, rtol=1e-4)                # softmax rows
    np.testing.assert_array_equal(got['y_true.npy'].sum(-1), 1.0)                        # one-hot rows
    assert got['loss.npy'].size >= 1 and got['loss.npy'].reshape(-1)[0] > 0.0
    # --layers / --all-kernels read the instrumented pass: refused without --full, before any GPU work
    r = subprocess.run(cmd + ['--layers'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 2 and '--full' in r.stderr
