"""-m gpu: resumable training (train.py --ckpt_every / --resume / --stop_after_epochs) -- rd_snapshot (csrc/snapshot.hip) against the
numpy model of its checksums (ramdsir/ckpt.py checksums) bit for bit in both directions, a restore that refuses a corrupted staging
buffer, twin trainers (uninterrupted against snapshot -> fresh trainer -> restore), and the CLI: a run cut in two equals the
uninterrupted run byte for byte.

Everything here is an equality: the kernel moves words and adds integers mod 2^64 (no rounding, no order dependence), and the training
step is bitwise reproducible, so there is no tolerance anywhere in this file."""
import glob
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

from ramdsir import _lib as L, ckpt as CK       # noqa: E402

CH = L.SNAP_CHUNK
GUARD = 4096
SIZES = [4, 8, 12, 16, 20, 60, 64, 68, CH - 4, CH, CH + 4, 3 * CH + 12]
SHIFTS = [0, 4, 8, 12]


def _hash_words(n):
    """arange plus a hash: every word differs from its neighbours and from its index, high bits set in many (the sums wrap)."""
    x = np.arange(n, dtype=np.uint64)
    return ((x * np.uint64(2654435761) ^ (x >> np.uint64(7)) ^ np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)).astype('<u4')


def _dev_bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def _up16(v):
    return (v + 15) // 16 * 16


# a layout: [(bytes, shift of the device start from a 16-byte boundary, shift of the staging offset from one)]
LAYOUTS = {
    'sizes_x_alignments': [(b, s, t) for b in SIZES for s in SHIFTS for t in SHIFTS],
    'zero_length_between': [(68, 4, 0), (0, 0, 8), (CH + 4, 0, 0), (0, 8, 8), (0, 0, 0), (12, 12, 12), (0, 4, 0)],
    'single': [(3 * CH + 12, 8, 8)],
    'single_word': [(4, 12, 4)],
    'many_small': [(8, 4 * (i % 4), 4 * ((i // 4) % 4)) for i in range(200)],
}


def _place(layout, gap):
    """Device-side and staging-side byte positions of every range: starts shifted as asked, `gap` bytes between device ranges."""
    dpos, spos, out = gap, 0, []
    for nbytes, dshift, sshift in layout:
        d, s = _up16(dpos) + dshift, _up16(spos) + sshift
        out.append((d, s, nbytes))
        dpos, spos = d + nbytes + gap, s + nbytes
    return out, _up16(dpos) + 16, _up16(spos) + 16


def _call(ranges_buf, staging, body, placed, direction, sums):
    arr, chunks = CK.build_table([(ranges_buf.data_ptr() + d, n, s) for d, s, n in placed])
    table_dev = CK.upload_table(arr, len(placed), DEV)
    code = CK.run(arr, table_dev, len(placed), chunks, staging.data_ptr() + GUARD, body, sums.data_ptr(), direction)
    torch.cuda.synchronize()
    return code, chunks


def _sums(sums, n):
    return CK.read_sums(sums, n)


def _sum_buffer(n, fill=-1):
    """n lines of sums and one more behind them that no call may touch."""
    return torch.full(((n + 1) * L.SNAP_SUM_STRIDE,), fill, dtype=torch.int64, device=DEV)


def _only_the_sums_are_written(sums, n):
    a = sums.cpu().numpy().reshape(n + 1, L.SNAP_SUM_STRIDE)
    return bool((a[:n, 2:] == -1).all() and (a[n] == -1).all())


@pytest.mark.parametrize('name', list(LAYOUTS))
def test_gather_equals_the_model_bit_for_bit(name):
    layout = LAYOUTS[name]
    placed, dbytes, body = _place(layout, 0)
    src_np = _hash_words(dbytes // 4).view(np.uint8)
    src = _dev_bytes(src_np)
    assert src.data_ptr() % 16 == 0
    staging = torch.full((GUARD + body + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    sums = _sum_buffer(len(layout))
    code, chunks = _call(src, staging, body, placed, 0, sums)
    assert code == 0 and chunks == sum((n + CH - 1) // CH for n, _, _ in layout)
    want = np.full(GUARD + body + GUARD, 0xA5, np.uint8)
    for d, s, n in placed:
        want[GUARD + s:GUARD + s + n] = src_np[d:d + n]
    got = staging.cpu().numpy()
    assert np.array_equal(got, want)                                        # the ranges, the gaps between them and both sentinels
    assert np.array_equal(src.cpu().numpy(), src_np)                        # a gather only reads its sources
    model = [CK.checksums(src_np[d:d + n]) for d, s, n in placed]
    assert _sums(sums, len(layout)) == model
    assert _only_the_sums_are_written(sums, len(layout))                    # two words per line, nothing behind the n lines
    if name == 'sizes_x_alignments':
        assert any(a >= 1 << 40 for a, _ in model) and len(set(model)) > len(SIZES)
    # again: the sums are cleared, not accumulated
    code, _ = _call(src, staging, body, placed, 0, sums)
    assert code == 0 and _sums(sums, len(layout)) == model and np.array_equal(staging.cpu().numpy(), want)


@pytest.mark.parametrize('name', list(LAYOUTS))
def test_scatter_equals_the_model_bit_for_bit(name):
    layout = LAYOUTS[name]
    placed, dbytes, body = _place(layout, GUARD)                            # 4 KiB of sentinel around every destination range
    stage_np = np.full(GUARD + body + GUARD, 0xA5, np.uint8)
    stage_np[GUARD:GUARD + body] = _hash_words(body // 4).view(np.uint8)
    staging = _dev_bytes(stage_np)
    dst = torch.full((dbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    assert dst.data_ptr() % 16 == 0 and staging.data_ptr() % 16 == 0
    sums = _sum_buffer(len(layout))
    code, _ = _call(dst, staging, body, placed, 1, sums)
    assert code == 0
    want = np.full(dbytes, 0x5A, np.uint8)
    for d, s, n in placed:
        want[d:d + n] = stage_np[GUARD + s:GUARD + s + n]
    assert np.array_equal(dst.cpu().numpy(), want)                          # every range, and every sentinel around every range
    assert np.array_equal(staging.cpu().numpy(), stage_np)
    model = [CK.checksums(stage_np[GUARD + s:GUARD + s + n]) for d, s, n in placed]
    assert _sums(sums, len(layout)) == model and _only_the_sums_are_written(sums, len(layout))
    code, _ = _call(dst, staging, body, placed, 1, sums)
    assert code == 0 and _sums(sums, len(layout)) == model and np.array_equal(dst.cpu().numpy(), want)


def test_gather_then_scatter_round_trips_through_other_alignments():
    """Gather from one set of device alignments, scatter to another: the sums of both directions agree range by range."""
    layout = LAYOUTS['sizes_x_alignments']
    placed, dbytes, body = _place(layout, 0)
    src_np = _hash_words(dbytes // 4).view(np.uint8)
    src = _dev_bytes(src_np)
    staging = torch.zeros(GUARD + body + GUARD, dtype=torch.uint8, device=DEV)
    sums = _sum_buffer(len(layout))
    assert _call(src, staging, body, placed, 0, sums)[0] == 0
    first = _sums(sums, len(layout))
    back_layout = [(n, (ds + 8) % 16, ss) for n, ds, ss in layout]
    placed2, dbytes2, body2 = _place(back_layout, GUARD)
    assert body2 == body and [p[1:] for p in placed2] == [p[1:] for p in placed]
    dst = torch.zeros(dbytes2, dtype=torch.uint8, device=DEV)
    assert _call(dst, staging, body, placed2, 1, sums)[0] == 0
    assert _sums(sums, len(layout)) == first
    out = dst.cpu().numpy()
    for (d, s, n), (d2, _, _) in zip(placed, placed2):
        assert np.array_equal(out[d2:d2 + n], src_np[d:d + n])


def test_validation_codes_and_the_empty_call():
    buf = torch.full((8 * CH,), 0x11, dtype=torch.uint8, device=DEV)
    staging = torch.full((4 * CH,), 0x22, dtype=torch.uint8, device=DEV)
    sums = _sum_buffer(3)
    base, st, sp = buf.data_ptr(), staging.data_ptr(), sums.data_ptr()
    good = [(base, 64, 0), (base + 4096, CH + 8, 64), (base + 3 * CH, 16, 2 * CH)]
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream

    def code(entries=good, n=None, total=None, staging_bytes=4 * CH, direction=0, chunk0=None, stage=st, sums_ptr=sp, dev=True):
        arr, chunks = CK.build_table(entries)
        for i, v in (chunk0 or {}).items():
            arr[i].chunk0 = v
        table_dev = CK.upload_table(arr, len(entries), DEV)
        n = len(entries) if n is None else n
        return lib.rd_snapshot(arr, table_dev.data_ptr() if dev else None, n, chunks if total is None else total, stage, staging_bytes,
                               sums_ptr, direction, stream)
    assert code(n=-1) == -1 and code(stage=None) == -1 and code(sums_ptr=None) == -1 and code(dev=False) == -1
    assert code([(base, 6, 0)]) == -2 and code([(base, -4, 0)]) == -2
    assert code([(base + 2, 8, 0)]) == -3 and code([(base, 8, 2)]) == -3 and code(stage=st + 2) == -3 and code([(None, 8, 0)]) == -3
    assert code([(base, 64, 0), (base + 4096, 64, 60)]) == -4                 # overlap
    assert code([(base, 64, 64), (base + 4096, 64, 0)]) == -4                 # descending
    assert code(staging_bytes=2 * CH + 12) == -4 and code([(base, 64, 4 * CH - 60)]) == -4 and code([(base, 8 * CH, 0)]) == -4
    assert code(total=3) == -5 and code(total=5) == -5 and code(chunk0={1: 0}) == -5 and code(chunk0={2: 2}) == -5
    assert code(direction=2) == -6 and code(direction=-1) == -6
    # n == 0 succeeds without a table, a staging buffer or sums
    assert lib.rd_snapshot(None, None, 0, 0, None, 0, None, 0, stream) == 0 and lib.rd_snapshot(None, None, 0, 0, None, 0, None, 1, stream) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0x11).all()) and bool((staging == 0x22).all()) and bool((sums == -1).all())       # nothing was launched
    assert code() == 0 and code(staging_bytes=2 * CH + 16) == 0
    torch.cuda.synchronize()
    assert bool((staging[:64] == 0x11).all()) and bool((staging[2 * CH + 16:] == 0x22).all()) and _only_the_sums_are_written(sums, 3)
    # only empty ranges: the clear alone
    assert code([(base, 0, 0), (None, 0, 0)]) == 0
    torch.cuda.synchronize()
    assert _sums(sums, 2) == [(0, 0), (0, 0)] and _sums(sums, 3)[2][0] == 4 * 0x11111111 and _only_the_sums_are_written(sums, 3)


# ------------------------------------------------------------------------------------------------------------- the trainer
def _trainer(dataset, bs, S, seed=17):
    from networks.unet import Encoder, Decoder, Rec_Decoder
    from ramdsir.trainer import FusedTrainer
    torch.manual_seed(seed)
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


def _epoch(tr, batches):
    """One 'epoch' as train.py runs it: pipelined steps, the last one without a successor."""
    for i, b in enumerate(batches):
        tr.step(*b, next_batch=batches[i + 1] if i + 1 < len(batches) else None)


def _assert_same_trainer(a, b, what):
    torch.cuda.synchronize()
    for name in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(a.bank, name), getattr(b.bank, name)), (what, name)
    assert list(a.bank.buffers) == list(b.bank.buffers)
    for k in a.bank.buffers:
        assert torch.equal(a.bank.buffers[k], b.bank.buffers[k]), (what, k)
    for name in ('iter', 'hyper', 'losses', 'rec_mse'):
        assert torch.equal(getattr(a.ts, name), getattr(b.ts, name)), (what, name)
    assert torch.equal(a.ts.wpack.packed, b.ts.wpack.packed), (what, 'packed weights')


@pytest.mark.parametrize('dataset,bs', [('fundus', [3, 6, 7]), ('prostate', [2, 2, 2, 2, 2])])
def test_twin_trainers_restore_continues_bit_for_bit(tmp_path, dataset, bs):
    """A: 2 k steps.  B: k steps, snapshot (the writer's host checksums verified), k more.  C: freshly initialised modules with other
    weights, restore, k steps on the same batches.  k = 4: three pipelined steps leave A and B on input slot 1 at the boundary while C
    starts on slot 0.  A == B == C in every arena, buffer, counter, loss word and packed weight."""
    S, k = 32, 4
    batches = _batches(dataset, sum(bs), S, 2 * k)
    A, B = _trainer(dataset, bs, S), _trainer(dataset, bs, S)
    _epoch(A, batches[:k])
    _epoch(A, batches[k:])
    _epoch(B, batches[:k])
    sb = CK.TrainState(B, dict(total_iters=40))
    assert [e['name'] for e in sb.table][:3] == ['params', 'exp_avg', 'exp_avg_sq'] and sb.table[-2]['name'] == 'iter'
    path = str(tmp_path / 'last_state.pth')
    sb.snapshot(path, dict(epoch=0, iter_num=k))
    _epoch(B, batches[k:])                                  # training goes on while the writer works
    sb.close()
    assert os.listdir(tmp_path) == ['last_state.pth'] and sb.seconds['calls'] == 1 and sb.seconds['gather'] > 0
    print(sb.report())
    _assert_same_trainer(A, B, 'a snapshot does not change the trainer')
    state = CK.load_file(path)                              # verifies every range on the host once more
    assert state['meta'] == dict(epoch=0, iter_num=k) and int(CK.range_tensor(state, 'iter')) == k
    Cm = _trainer(dataset, bs, S, seed=99)
    assert not torch.equal(Cm.bank.params, B.bank.params)
    sc = CK.TrainState(Cm, dict(total_iters=40))
    sc.restore(state)
    assert sc.device_sums() == [(e['s1'], e['s2']) for e in state['table']]
    for m, mod in Cm.modules.items():                       # the module parameters are the arena's views
        for key, p in mod.named_parameters():
            assert p.data_ptr() == Cm.bank.p(m, key).data_ptr()
    _epoch(Cm, batches[k:])
    _assert_same_trainer(A, Cm, 'restored and continued')
    with pytest.raises(ValueError, match='total_iters = 40, this run has 50'):
        CK.TrainState(Cm, dict(total_iters=50)).restore(state)
    sc.close()


def test_restore_refuses_a_corrupted_staging_buffer(tmp_path):
    """One word of the staging buffer flipped between the upload and the scatter: the device checksum of the words written differs
    from the file's, and restore names the range."""
    bs, S = [1, 1, 1], 32
    B = _trainer('fundus', bs, S)
    _epoch(B, _batches('fundus', 3, S, 2))
    sb = CK.TrainState(B)
    path = str(tmp_path / 's.pth')
    sb.snapshot(path, {})
    sb.close()
    state = CK.load_file(path)
    Cm = _trainer('fundus', bs, S, seed=99)
    sc = CK.TrainState(Cm)
    e = next(e for e in state['table'] if e['name'] == 'exp_avg')
    sc.upload(state)
    word = sc.dev[e['offset'] + 4 * 1000:e['offset'] + 4 * 1000 + 4]
    word ^= 0x40
    with pytest.raises(ValueError, match='range exp_avg arrived corrupt'):
        sc.scatter(state)
    sc.upload(state)                                        # the intact blob again: accepted
    sc.scatter(state)
    assert torch.equal(Cm.bank.exp_avg, B.bank.exp_avg)
    sc.close()


# ------------------------------------------------------------------------------------------------------------- the CLI
def _truncate(path, n):
    lines = open(path).read().split('\n')[:n]
    open(path, 'w').write('\n'.join(lines) + '\n')


def _tree(tmp_path, dataset):
    """Domain lists of DIFFERENT lengths: the longest loader is the middle one, the cycled loader in front of it wraps within an epoch
    and loses an item at every epoch end (zip), the ones behind it wrap without losing one."""
    data = str(tmp_path / 'data')
    if dataset == 'fundus':                                  # batch sizes 3, 6, 7 -> 3, 5 and 2 batches per pass
        base = SD.make_fundus_tree(data, n_train=30, n_test=2, hw=(72, 80), vary=False)
        for d, n in ((2, 9), (3, 30), (4, 14)):
            _truncate(os.path.join(base, 'Domain%d_train.list' % d), n)
    else:                                                   # batch size 2 everywhere -> 3, 5, 2, 4 and 1 batches per pass
        base = SD.make_prostate_tree(data, n=10, S=64)
        for d, n in ((2, 6), (3, 10), (4, 4), (5, 8), (6, 2)):
            for i in range(n, 10):
                for sub in ('image', 'mask'):
                    os.remove(os.path.join(base, 'Domain%d' % d, sub, 'd%d_s%02d.npy' % (d, i)))
    return data


def _train(data, dataset, out, extra, epochs=4, source=('--gpu_data',)):
    domains = '1,2,3' if dataset == 'fundus' else '1,2,3,4,5'
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', dataset, '--domain_idxs',
           domains, '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd',
           '--save_path', out, '--epochs', str(epochs), '--num_workers', '0', '--log_every', '3', '--deterministic']
    cmd += list(source) + (['--gpu_val'] if dataset == 'fundus' else []) + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    log = r.stdout.decode()
    # a process that died of a signal (a GPU fault, an abort) ends the test here: nothing more is started on the device
    assert r.returncode >= 0 and r.returncode not in (134, 139), log[-3000:]
    return r.returncode, log


def _scalars(out):
    sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))
    from utils import tfevents
    recs, files = [], sorted(os.listdir(os.path.join(out, 'log')))
    for f in files:
        ev = tfevents.read_events(os.path.join(out, 'log', f))
        assert all(len(e['scalars']) == 1 and not e['images'] for e in ev[1:])
        recs += [(e['step'],) + tuple(e['scalars'][0]) for e in ev[1:]]
    return recs, len(files)


def _outputs(out, dataset):
    ck = torch.load(os.path.join(out, 'final_model.pth'), map_location='cpu')
    csv = os.path.join(out, '0_val_log.csv')
    return dict(ck=ck, csv=open(csv).read() if os.path.exists(csv) else None,
                models=sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, 'model_*.pth'))), scalars=_scalars(out)[0])


def _assert_same_run(a, b, what):
    assert list(a['ck']) == list(b['ck']), what
    for part in a['ck']:
        assert list(a['ck'][part]) == list(b['ck'][part]), (what, part)
        for k in a['ck'][part]:
            assert torch.equal(a['ck'][part][k], b['ck'][part][k]), (what, part, k)
    assert a['csv'] == b['csv'] and a['models'] == b['models'], what
    assert a['scalars'] == b['scalars'], what


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_a_run_cut_in_two_equals_the_uninterrupted_run(tmp_path, dataset):
    """(a) 4 epochs without the flags; (b) --ckpt_every 1; (c) --ckpt_every 1 --stop_after_epochs 2, then --resume in the same
    --save_path.  final_model.pth tensor for tensor and key for key, the validation CSV, the model_*.pth names and the scalar records
    of (b) and of (c)'s two event files together are those of (a); a further --resume under another --epochs names total_iters."""
    data = _tree(tmp_path, dataset)
    dirs = {n: str(tmp_path / n) for n in 'abc'}
    code, log_a = _train(data, dataset, dirs['a'], [])
    assert code == 0, log_a[-3000:]
    assert 'ckpt:' not in log_a and not os.path.exists(os.path.join(dirs['a'], 'last_state.pth'))
    code, log_b = _train(data, dataset, dirs['b'], ['--ckpt_every', '1'])
    assert code == 0, log_b[-3000:]
    assert 'ckpt: 4 snapshots' in log_b and os.listdir(dirs['b']).count('last_state.pth') == 1
    assert not any(f.endswith('.tmp') for f in os.listdir(dirs['b']))
    code, log_c1 = _train(data, dataset, dirs['c'], ['--ckpt_every', '1', '--stop_after_epochs', '2'])
    assert code == 0, log_c1[-3000:]
    assert 'ckpt: 2 snapshots' in log_c1 and 'Stopped after 2 epochs' in log_c1
    assert not os.path.exists(os.path.join(dirs['c'], 'final_model.pth'))
    state = os.path.join(dirs['c'], 'last_state.pth')
    mid = CK.load_file(state)
    assert mid['meta']['epoch'] == 1 and mid['meta']['iter_num'] == 10 and int(CK.range_tensor(mid, 'iter')) == 10
    cycles = mid['meta']['cycles']
    assert cycles[1] is None and all(c is not None for i, c in enumerate(cycles) if i != 1)
    assert cycles[0][1] == (2 * 6) % 3 and cycles[2][1] == (2 * 5) % 2 and len(cycles[0][0]) == 3      # the lost item: 6 pulls per epoch
    if dataset == 'fundus':
        # lines of an epoch that ran after the snapshot: a resumed run drops them
        with open(os.path.join(dirs['c'], '0_val_log.csv'), 'a') as f:
            f.write('a line of an epoch that was lost with its process\n')
    code, log_c2 = _train(data, dataset, dirs['c'], ['--resume', state, '--ckpt_every', '1'])
    assert code == 0, log_c2[-3000:]
    assert 'continuing at epoch 2 (iteration 10' in log_c2 and ('truncated from' in log_c2) == (dataset == 'fundus')
    a, b, c = (_outputs(dirs[n], dataset) for n in 'abc')
    assert (a['csv'] is not None and len(a['models']) == 1) == (dataset == 'fundus')
    assert [s for s, t, _ in a['scalars'] if t == 'lr'] == [0, 3, 6, 9, 12, 15, 18]
    assert _scalars(dirs['c'])[1] == 2
    _assert_same_run(a, b, 'snapshots every epoch')
    _assert_same_run(a, c, 'stopped after two epochs and resumed')
    # the snapshot of a finished epoch turns into the reference's checkpoint without a GPU
    sds = CK.state_dicts(CK.load_file(os.path.join(dirs['b'], 'last_state.pth')))
    for part in a['ck']:
        assert list(sds[part]) == list(a['ck'][part])
        assert all(torch.equal(sds[part][k], a['ck'][part][k]) for k in sds[part]), part
    code, log_d = _train(data, dataset, dirs['c'], ['--resume', state, '--ckpt_every', '1'], epochs=5)
    assert code != 0 and 'total_iters' in log_d, log_d[-3000:]


def test_train_cli_resume_on_the_host_data_path(tmp_path):
    """(c) with --num_workers 0 instead of --gpu_data: the replay lists of the host path (batches of tensors) pickle and restore, and
    the resumed run ends where the uninterrupted host-path run ends."""
    data = _tree(tmp_path, 'fundus')
    a, c = str(tmp_path / 'a'), str(tmp_path / 'c')
    code, log = _train(data, 'fundus', a, [], source=())
    assert code == 0, log[-3000:]
    code, log = _train(data, 'fundus', c, ['--ckpt_every', '1', '--stop_after_epochs', '2'], source=())
    assert code == 0 and not os.path.exists(os.path.join(c, 'final_model.pth')), log[-3000:]
    code, log = _train(data, 'fundus', c, ['--resume', os.path.join(c, 'last_state.pth'), '--ckpt_every', '1'], source=())
    assert code == 0 and 'freshly seeded workers' not in log, log[-3000:]
    _assert_same_run(_outputs(a, 'fundus'), _outputs(c, 'fundus'), 'host data path, stopped and resumed')
