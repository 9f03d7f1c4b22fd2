"""CPU-only tests of the per-step record ring (train.py --tb_every_iter / --tb_health): the descriptor's layout, the numpy model of the
kernel on hand-derived rows, the loss_dict refactor, the ring bookkeeping, the rank mean over gloo and the flags.  The kernel itself is
tested on the GPU (test_gpu_step_log.py)."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_module():
    spec = importlib.util.spec_from_file_location('rd_train_step_log', os.path.join(ROOT, 'ram-dsir_amd', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_struct_size_and_symbols(tmp_path):
    from ramdsir import _lib as L
    c = tmp_path / 's.c'
    c.write_text('#include <stdio.h>\n#include "ramdsir.h"\nint main(){printf("%zu %d %d %d\\n", sizeof(rd_step_log_t), RD_LOG_ROW, '
                 'RD_LOG_MAX_REC, RD_LOG_CHUNK);return 0;}')
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [ctypes.sizeof(L.RdStepLog), L.LOG_ROW, L.LOG_MAX_REC, L.LOG_CHUNK]
    assert L.LOG_ROW == 32 and ctypes.sizeof(L.RdStepLog) == 4 * 8 + 4 * 8 + 8 + 4 * 4 + 8
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ('rd_step_log', 'rd_step_log_workspace'):
        assert hasattr(raw, name) and name in L.exported_symbols()
    lib = L.lib()
    # host-only: bytes of the partials of n elements in three groups (16 bytes per chunk, at most n / chunk + 3 chunks)
    assert lib.rd_step_log_workspace(0) == 48 and lib.rd_step_log_workspace(3800021) == (3800021 // 4096 + 3) * 16
    assert lib.rd_step_log_workspace(-5) == 48


def test_model_row_on_hand_derived_rows():
    from ramdsir import step_log as SL
    losses = [0.5, 0.25, 1.5, 2.0, 0.125, 4.0, 0.0, 0.0]
    hyper = [0.002, 0.1, 0.001, 7.0]
    rec = [0.75, 0.5, 0.25]
    # group 0 = (3, 4) -> 5; group 1 = (1, 2, 2) -> 3; group 2 = (6, 8, 0) -> 10
    g = np.array([3, 4, 1, 2, 2, 6, 8, 0], np.float32)
    row = SL.model_row(losses, rec, hyper, g, [0, 2, 5, 8])
    assert row.dtype == np.float32 and row.shape == (32,)
    want = np.zeros(32, np.float32)
    want[0:8], want[8:12], want[12:15] = losses, np.float32(hyper), rec
    want[28:32] = [5.0, 3.0, 10.0, 0.0]
    assert np.array_equal(row, want)
    # without gradients the health words are zero and the rest is the same
    plain = SL.model_row(losses, rec, hyper)
    assert np.array_equal(plain[:28], want[:28]) and not plain[28:].any()
    # a NaN and an Inf at the first and the last element of a range: counted, left out of the sum
    g2 = np.array([np.nan, 3, 4, -np.inf, 1, 2, 2, 6, 8, np.inf], np.float32)
    row2 = SL.model_row(losses, rec, hyper, g2, [0, 4, 7, 10])
    assert row2[28:32].tolist() == [5.0, 3.0, 10.0, 3.0]
    # the ranges need not start at 0 nor cover the array; an empty group has norm 0
    row3 = SL.model_row(losses, rec, hyper, g, [1, 1, 2, 5])
    assert row3[28:32].tolist() == [0.0, 4.0, 3.0, 0.0]


@pytest.mark.parametrize('dataset,seg', [('fundus', 'bce'), ('prostate', 'ce')])
def test_loss_dict_is_the_pure_function_of_its_two_lists(dataset, seg):
    from ramdsir import step as S
    from ramdsir import step_log as SL

    class Fake:
        pass
    f = Fake()
    f.dataset, f.lambda_rec = dataset, 0.1
    f.losses = torch.tensor([0.7, 0.3, 0.6, 0.2, 0.05, 1.85, 0.0, 0.0])
    f.rec_mse = torch.tensor([0.11, 0.22, 0.33] if dataset == 'fundus' else [0.1, 0.2, 0.3, 0.4, 0.5])
    got = S.TrainStep.loss_dict(f)
    l, r = f.losses.tolist(), f.rec_mse.tolist()
    assert got == S.loss_dict_of(dataset, 0.1, l, r)
    assert list(got) == ['loss_%s_1' % seg, 'loss_dice_1', 'loss_%s_2' % seg, 'loss_dice_2', 'loss_consistency', 'rec', 'loss']
    assert got['rec'] == r and got['loss'] == l[5] + 0.1 * sum(r) and got['loss_dice_2'] == l[3]
    # a drained row goes through the same function on the same floats: the record's dict is EQUAL
    row = SL.model_row(l, r, [2e-3, 0.1, 0.001, 12.0])
    rec = SL.records_of(row[None], dataset, 0.1, len(r))[0]
    assert rec['losses'] == got and rec['iteration'] == 12 and rec['lr'] == float(np.float32(2e-3))
    assert rec['norms'] == (0.0, 0.0, 0.0) and rec['nonfinite'] == 0


def _stub_log(rows):
    """A StepLog on CPU tensors whose launch is replaced by the numpy model: each append stamps the next iteration number."""
    from ramdsir import step_log as SL

    class Stub(SL.StepLog):
        def _launch(self, row, stream):
            it = self.appended
            self.ring[row] = torch.from_numpy(SL.model_row([it + 0.5] * 8, [it * 0.25] * 3, [1e-3, 0, 0, it]))
            self.launched.append(row)
    log = Stub(torch.zeros(8), torch.zeros(3), torch.zeros(4), rows=rows)
    log.launched = []
    return log


def test_ring_bookkeeping():
    log = _stub_log(4)
    seen = []
    for i in range(11):
        log.append(None)
        if log.full():
            seen += log.drain('fundus', 0.1)
    assert log.pending == 3
    seen += log.drain('fundus', 0.1)
    assert [r['iteration'] for r in seen] == list(range(11)) and log.pending == 0 and log.drain('fundus', 0.1) == []
    assert log.launched == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2]
    assert [r['losses']['loss_bce_1'] for r in seen] == [i + 0.5 for i in range(11)]
    assert seen[10]['losses']['rec'] == [2.5] * 3
    # wrap-around: the pending rows are two spans, the older one (the end of the ring) first
    log = _stub_log(4)
    for _ in range(3):
        log.append(None)
    assert log.spans() == [(0, 3)]
    log.drain('fundus', 0.1)
    for _ in range(3):
        log.append(None)
    assert log.spans() == [(3, 4), (0, 2)]
    assert [r['iteration'] for r in log.drain('fundus', 0.1)] == [3, 4, 5]
    assert log.spans() == []
    # overflow: the fifth undrained row would overwrite the oldest; a counter that got past the capacity is refused at the drain, too
    for _ in range(4):
        log.append(None)
    with pytest.raises(RuntimeError, match='pending'):
        log.append(None)
    log.appended += 1
    with pytest.raises(RuntimeError, match='overwritten'):
        log.drain('fundus', 0.1)
    with pytest.raises(ValueError):
        _stub_log(0)


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path[:0] = [%r, %r]
from ramdsir import step_log as SL
rank, world = int(sys.argv[1]), int(sys.argv[3])
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=sys.argv[2], RANK=str(rank), WORLD_SIZE=str(world))
dist.init_process_group('gloo', rank=rank, world_size=world)
g = torch.Generator().manual_seed(5)
a, b = torch.rand(5, 32, generator=g), torch.rand(5, 32, generator=g)
mine = (a, b)[rank].clone()
out = SL.rank_mean(mine.clone())
mean = (a + b) / 2
assert torch.equal(out[:, 0:8], mean[:, 0:8]) and torch.equal(out[:, 12:28], mean[:, 12:28])
assert torch.equal(out[:, 8:12], mine[:, 8:12]) and torch.equal(out[:, 28:32], mine[:, 28:32])      # hyper, health: untouched
# through StepLog.drain: the records carry the rank mean, and what FusedTrainer.losses() would form for one row
class Stub(SL.StepLog):
    def _launch(self, row, stream):
        self.ring[row] = mine[self.appended]
log = Stub(torch.zeros(8), torch.zeros(3), torch.zeros(4), rows=8)
for _ in range(5):
    log.append(None)
recs = log.drain('fundus', 0.1, world=world)
buf = torch.cat([a[2, 0:8], a[2, 12:15]]) + torch.cat([b[2, 0:8], b[2, 12:15]])
buf /= world
assert recs[2]['losses']['loss_dice_1'] == float(buf[1]) and recs[2]['losses']['rec'] == buf[8:].tolist()
assert recs[2]['lr'] == float(mine[2, 8]) and recs[2]['iteration'] == int(mine[2, 11])
dist.destroy_process_group()
print('ok')
'''


def test_rank_mean_over_gloo(tmp_path):
    script = tmp_path / 'w.py'
    script.write_text(_WORKER % (ROOT, os.path.join(ROOT, 'ram-dsir_amd')))
    port = str(31500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), port, '2'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and 'ok' in o, o


def test_flags():
    m = _train_module()
    base = ['--save_path', 'x', '--ram', '--rec']
    a = m.parse_args(base)
    assert a.tb_every_iter is False and a.tb_health is False and not m.uses_step_log(a)
    assert m.uses_step_log(m.parse_args(base + ['--tb_health'])) and m.uses_step_log(m.parse_args(base + ['--tb_every_iter']))
    for flag in ('--tb_every_iter', '--tb_health'):
        with pytest.raises(ValueError, match='--log_every 1'):
            m.main(m.parse_args(base + ['--norm', 'gn', flag]))
    # what a drained record contributes to the event file
    rec = {'iteration': 7, 'lr': 0.5, 'losses': {'loss_bce_1': 1.0, 'loss_dice_1': 2.0, 'loss_bce_2': 3.0, 'loss_dice_2': 4.0,
                                                   'loss_consistency': 5.0, 'rec': [1.0, 2.0, 5.0], 'loss': 9.0},
           'norms': (1.5, 2.5, 3.5), 'nonfinite': 2}
    seven = [('lr', 0.5), ('loss/loss_bce_1', 1.0), ('loss/loss_dice_1', 2.0), ('loss/loss_bce_2', 3.0), ('loss/loss_dice_2', 4.0),
             ('loss/loss_consistency', 5.0), ('loss/loss_rec', 2.0)]
    health = [('health/grad_norm_encoder', 1.5), ('health/grad_norm_seg_decoder', 2.5), ('health/grad_norm_rec_decoder', 3.5),
              ('health/nonfinite_grads', 2.0)]
    assert m.step_log_pairs(rec, True, False, 20) == seven == m.scalar_pairs(0.5, rec['losses'])
    assert m.step_log_pairs(rec, True, True, 20) == seven + health
    assert m.step_log_pairs(rec, False, True, 20) == health and m.step_log_pairs(rec, False, True, 7) == seven + health
    assert not m.record_is_finite(rec) and m.record_is_finite(dict(rec, nonfinite=0))
    assert not m.record_is_finite(dict(rec, nonfinite=0, losses=dict(rec['losses'], loss_dice_1=float('nan'))))
