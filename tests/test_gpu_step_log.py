"""-m gpu: train.py --tb_every_iter / --tb_health -- rd_step_log (csrc/step_log.hip) against its numpy model (ramdsir/step_log.py
model_row), the fused trainer appending a row behind every step without changing the training, and the CLI end to end.

Equality rules.  On gradients that are dyadic rationals (k / 8, |k| <= 16: the squares are multiples of 1 / 64 and every partial sum is an
integer multiple of 1 / 64 far below 2^53) the fp64 sums are exact in any order, so a row equals the model in every word.  On random
gradients the model restates the kernel's summation order (ramdsir/sumsq.py, given the arena's alignment), so the row equals it there
as well; the ulp figure is printed.  Only the comparison with torch's norm, which sums in another order, is held to one ulp: the fp64
accumulation of n <= 4e6 terms is off by at most n * 2^-53 ~ 4e-10 relative, far below the fp32 half-ulp of 6e-8, so the stored
float32 can differ from float32(sqrt(float64 sum)) only next to a rounding boundary, and then by one ulp."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth_data as SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, step_log as SL       # noqa: E402

LOSSES = [0.5, 0.25, 1.5, 2.0, 0.125, 4.375, -1.0, 3.0]
HYPER = [2e-3, 0.1, 1e-3, 41.0]
REC = [0.75, 0.5, 0.25]


def _row(grads, ranges, rec=REC, rows=3, row=1):
    """One rd_step_log call through StepLog's descriptor at ring row `row` -> (the row, the whole ring) as numpy."""
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)       # noqa: E731
    log = SL.StepLog(dev(LOSSES), dev(rec), dev(HYPER), grads, ranges, rows=rows)
    log.ring.fill_(-7.0)
    log._launch(row, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ring = log.ring.cpu().numpy()
    return ring[row], ring


def _dyadic(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-16, 17, (n,), generator=g).float() / 8).to(DEV)


def _ranges(base, lens):
    return [base, base + lens[0], base + lens[0] + lens[1], base + sum(lens)]


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


# (elements skipped in front of the view, range[0], the three group lengths)
LAYOUTS = [(0, 0, (1, 1, 1)), (0, 0, (5, 0, 3)), (0, 2, (1031, 4099, 7)), (0, 0, (70001, 3, 65537)), (1, 0, (1031, 4099, 7)),
           (3, 5, (4096, 8192, 4097)), (2, 1, (100003, 150001, 50007))]


@pytest.mark.parametrize('skip,base,lens', LAYOUTS)
def test_kernel_equals_the_model_bit_for_bit_on_exact_data(skip, base, lens):
    n = base + sum(lens) + 9
    whole = _dyadic(skip + n, sum(lens))
    grads = whole[skip:]                                     # skip != 0: the arena does not start on a 16-byte boundary
    assert grads.data_ptr() % 16 == (4 * skip) % 16
    ranges = _ranges(base, lens)
    row, ring = _row(grads, ranges)
    want = SL.model_row(LOSSES, REC, HYPER, grads.cpu().numpy(), ranges)
    assert np.array_equal(_bits(row), _bits(want)), (row, want)
    assert row[31] == 0 and (row[28:31] > 0).sum() == sum(1 for v in lens if v)
    assert (ring[0] == -7.0).all() and (ring[2] == -7.0).all()          # only row 1 of the ring is written
    assert (row[15:28] == 0).all()                           # the restoration slots beyond n_rec


def test_random_gradients_within_one_ulp_and_reproducible():
    lens = (400003, 350001, 250007)
    g = torch.Generator().manual_seed(9)
    grads = (torch.randn(sum(lens) + 3, generator=g) * torch.logspace(-6, 1, sum(lens) + 3)).to(DEV)
    ranges = _ranges(3, lens)
    row, _ = _row(grads, ranges)
    again, _ = _row(grads, ranges)
    assert np.array_equal(_bits(row), _bits(again))
    want = SL.model_row(LOSSES, REC, HYPER, grads.cpu().numpy(), ranges, align_words=(grads.data_ptr() >> 2) & 3)
    d = np.abs(_bits(row[28:31]).astype(np.int64) - _bits(want[28:31]).astype(np.int64))
    print('norms', row[28:31], 'model', want[28:31], 'ulp', d)
    assert d.max() == 0 and row[31] == 0                     # the model is order-exact (ramdsir/sumsq.py): not one ulp, equal
    assert np.array_equal(_bits(row[:28]), _bits(want[:28]))


def test_non_finite_elements_are_counted_and_left_out():
    lens = (10000, 9000, 5000)
    ranges = _ranges(3, lens)
    grads = _dyadic(ranges[3] + 5, 4)
    grads[:3] = float('nan')                                 # outside every range: neither counted nor summed
    grads[ranges[3]:] = float('inf')
    bad = []
    for k in range(3):
        bad += [ranges[k], ranges[k + 1] - 1]                # the first and the last element of each range
        bad += [ranges[k] + L.LOG_CHUNK - 1, ranges[k] + L.LOG_CHUNK]       # both sides of a chunk boundary
    vals = [float('nan'), float('inf'), float('-inf')]
    clean = grads.clone()
    for i, idx in enumerate(bad):
        grads[idx] = vals[i % 3]
        clean[idx] = 0.0
    row, _ = _row(grads, ranges)
    ref, _ = _row(clean, ranges)
    assert row[31] == len(bad) == 12 and ref[31] == 0
    assert np.array_equal(_bits(row[28:31]), _bits(ref[28:31])) and np.isfinite(row[28:31]).all()
    assert np.array_equal(_bits(row), _bits(SL.model_row(LOSSES, REC, HYPER, grads.cpu().numpy(), ranges)))


def test_without_gradients_and_argument_validation():
    rec16 = [0.5 + i for i in range(16)]
    row, ring = _row(None, None, rec=rec16, rows=2, row=1)
    assert np.array_equal(_bits(row), _bits(SL.model_row(LOSSES, rec16, HYPER)))
    assert not row[28:].any() and (ring[0] == -7.0).all()
    # the documented codes, before anything is launched: the ring keeps its contents
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)       # noqa: E731
    grads = _dyadic(100, 1)
    log = SL.StepLog(dev(LOSSES), dev(REC), dev(HYPER), grads, [0, 10, 20, 100], rows=4)
    log.ring.fill_(-7.0)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream

    def code(**kw):
        d = L.RdStepLog.from_buffer_copy(log.desc)
        for k, v in kw.items():
            if k == 'range':
                for i, x in enumerate(v):
                    d.range[i] = x
            else:
                setattr(d, k, v)
        return lib.rd_step_log(C.byref(d), st)
    assert lib.rd_step_log(None, st) == -1
    for field in ('losses', 'rec_mse', 'hyper', 'ring', 'partial'):
        assert code(**{field: None}) == -1, field
    assert code(row=4) == -2 and code(row=-1) == -2 and code(rows=0) == -2
    assert code(n_rec=17) == -3 and code(n_rec=-1) == -3
    assert code(range=[0, 20, 10, 100]) == -4 and code(range=[-1, 10, 20, 100]) == -4 and code(range=[0, 10, 20, (1 << 24) + 1]) == -4
    torch.cuda.synchronize()
    assert (log.ring == -7.0).all()
    assert code(row=3) == 0
    torch.cuda.synchronize()
    assert (log.ring[:3] == -7.0).all() and log.ring[3, 11] == 41.0


# ------------------------------------------------------------------------------------------------------------- the trainer
def _trainer(dataset, bs, S):
    from networks.unet import Encoder, Decoder, Rec_Decoder
    from ramdsir.trainer import FusedTrainer
    torch.manual_seed(17)
    enc, dec = Encoder().to(DEV), Decoder(num_classes=2).to(DEV)
    rec = Rec_Decoder(num_classes=3, norm='dsbn', num_domains=len(bs)).to(DEV)
    return FusedTrainer(enc, dec, rec, bs, S, S, dataset=dataset, consistency='kd', lr=1e-3, total_iters=40, dtype=torch.bfloat16)


def _batches(dataset, B, S, n):
    gen = torch.Generator(device=DEV).manual_seed(5)
    out = []
    for i in range(n):
        if dataset == 'fundus':
            src = (torch.rand(B, S, S, 3, device=DEV, generator=gen) * 255).to(torch.uint8)
            trg = (torch.rand(B, S, S, 3, device=DEV, generator=gen) * 255).to(torch.uint8)
            tgt = (torch.rand(B, 2, S, S, device=DEV, generator=gen) > 0.5).float()
        else:
            src = torch.rand(B, S, S, 3, device=DEV, generator=gen) * 2 - 1
            trg = torch.rand(B, S, S, 3, device=DEV, generator=gen) * 2 - 1
            tgt = (torch.rand(B, S, S, device=DEV, generator=gen) > 0.7).long()
        lam = torch.tensor([0.1 * (1 + (i + j) % 9) for j in range(B)], device=DEV)
        out.append((src, trg, lam, tgt))
    return out


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_twin_trainers_records_equal_the_reads_and_training_is_unchanged(dataset):
    """Twin A reads losses() and lr() after every step; twin B logs every step into a 4-row ring (health on) and drains it when full and
    at the end.  11 pipelined steps: every record equals A's reads exactly, and the two trainers end bit-identical.  Fundus: one of B's
    steps also has the image grids armed, so both users of the one after-step hook fire in the same step."""
    bs, S, n = [2, 3, 3], 32, 11
    batches = _batches(dataset, sum(bs), S, n)
    A, Bt = _trainer(dataset, bs, S), _trainer(dataset, bs, S)
    assert torch.equal(A.bank.params, Bt.bank.params)
    log = Bt.enable_step_log(health=True, rows=4)
    reads, records, images = [], [], None
    for i in range(n):
        nxt = batches[i + 1] if i + 1 < n else None
        A.step(*batches[i], next_batch=nxt)
        reads.append((A.losses(), A.lr()))
        if dataset == 'fundus' and i == 5:
            Bt.arm_tb_images()
        Bt.step(*batches[i], next_batch=nxt)
        if dataset == 'fundus' and i == 5:
            images = Bt.take_tb_images().images()
        if Bt.step_log_full():
            assert log.pending == 4
            records += Bt.drain_step_log()
    assert log.pending == 3
    records += Bt.drain_step_log()
    assert [r['iteration'] for r in records] == list(range(n))
    for (l, lr), r in zip(reads, records):
        assert r['losses'] == l and r['lr'] == lr, (r, l, lr)
        assert r['nonfinite'] == 0 and all(np.isfinite(v) and v > 0 for v in r['norms'])
    assert len({r['lr'] for r in records}) > 1              # the poly schedule moves: the rows are not copies of one row
    if dataset == 'fundus':
        assert len(images) == 7 and all(g.any() for _, g in images[:2])
    torch.cuda.synchronize()
    a, b = A.bank, Bt.bank
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.grads, b.grads) and list(a.buffers) == list(b.buffers)
    for k in a.buffers:
        assert torch.equal(a.buffers[k], b.buffers[k]), k
    # health against torch: the gradient arena is untouched until the next step zeroes it
    r = Bt.bank.module_range
    for k, m in enumerate(('enc', 'dec', 'rec')):
        want = np.float32(torch.linalg.vector_norm(b.grads[r[m][0]:r[m][1]].double()).item())
        got = np.float32(records[-1]['norms'][k])
        print(m, got, want)
        assert abs(int(_bits(got)) - int(_bits(want))) <= 1, (m, got, want)


def test_step_log_refuses_a_captured_graph():
    tr = _trainer('fundus', [1, 1, 1], 32)
    tr._graphs = True                                       # (what use_graph=True leaves; nothing is captured here)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_step_log()
    with pytest.raises(RuntimeError, match='enable_step_log'):
        tr.drain_step_log()


# ------------------------------------------------------------------------------------------------------------- the CLI
def _train(data, out, extra):
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', 'fundus', '--domain_idxs', '1,2,3',
           '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd', '--save_path', out,
           '--epochs', '20', '--max_iters', '45', '--num_workers', '0', '--deterministic']
    return subprocess.run(cmd + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)


def test_train_cli_every_iteration_equals_log_every_1(tmp_path):
    """(a) --log_every 1 without the flags against (b) --log_every 20 --tb_every_iter --tb_health, 45 iterations: the scalar records
    of (b) outside health/ are the records of (a) -- tags, steps, order, float32 values; (b) adds 45 x 4 finite health records with no
    non-finite gradient; the trained models are byte-identical; (b) prints the console line at the --log_every iterations only."""
    sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))
    from utils import tfevents
    data = str(tmp_path / 'data')
    SD.make_fundus_tree(data, n_train=21, n_test=1, hw=(72, 80), vary=False)
    runs = {}
    for name, extra in (('a', ['--log_every', '1']), ('b', ['--log_every', '20', '--tb_every_iter', '--tb_health'])):
        out = str(tmp_path / name)
        r = _train(data, out, extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        logs = os.listdir(os.path.join(out, 'log'))
        assert len(logs) == 1
        ev = tfevents.read_events(os.path.join(out, 'log', logs[0]))
        assert all(len(e['scalars']) == 1 and not e['images'] for e in ev[1:])
        runs[name] = ([(e['step'],) + tuple(e['scalars'][0]) for e in ev[1:]], open(os.path.join(out, 'final_model.pth'), 'rb').read(),
                      r.stdout.decode())
    (ev_a, ck_a, out_a), (ev_b, ck_b, out_b) = runs['a'], runs['b']
    tags = ['lr', 'loss/loss_bce_1', 'loss/loss_dice_1', 'loss/loss_bce_2', 'loss/loss_dice_2', 'loss/loss_consistency', 'loss/loss_rec']
    assert [(s, t) for s, t, _ in ev_a] == [(it, t) for it in range(45) for t in tags]
    plain_b = [e for e in ev_b if not e[1].startswith('health/')]
    assert plain_b == ev_a
    health = [e for e in ev_b if e[1].startswith('health/')]
    assert [(s, t) for s, t, _ in health] == [(it, t) for it in range(45) for t in SL.HEALTH_TAGS]
    assert all(np.isfinite(v) for _, _, v in health)
    assert all(v == 0 for _, t, v in health if t == 'health/nonfinite_grads') and all(v > 0 for _, t, v in health if 'grad_norm' in t)
    # within an iteration the health tags follow the seven scalars
    assert [t for s, t, _ in ev_b if s == 44] == tags + list(SL.HEALTH_TAGS)
    assert ck_a == ck_b
    assert sum(line.startswith('iter ') for line in out_a.splitlines()) == 45
    assert [line.split()[1] for line in out_b.splitlines() if line.startswith('iter ')] == ['0', '20', '40']
    assert 'tb_health:' not in out_b
