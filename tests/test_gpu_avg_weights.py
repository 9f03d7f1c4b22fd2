"""-m gpu: train.py --avg_weights -- rd_avg_step (csrc/avg.hip) against its numpy model (ramdsir/avg.py model) bit for bit, the fused
trainer maintaining the averaged bank behind every step without changing the training, the fused forward over the averaged bank, and
the CLI end to end (the flag leaves every existing output alone; the averaged outputs of a resumed run equal the uninterrupted run's).

Every comparison is an equality.  The kernel's arithmetic is three correctly rounded fp32 operations (and one correctly rounded
division for the uniform weight) on finite data, denormals kept: numpy float32 forms the same bits."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, avg as AV, ckpt as CK       # noqa: E402

CH = L.AVG_CHUNK
GAP = 4096                                                  # bytes of sentinel around every destination range
SENT = 0xA5
F32 = np.float32


def _st():
    return torch.cuda.current_stream().cuda_stream


def _floats(rng, n):
    """Random float32 words of many magnitudes with denormals, both zeros and exact repeats among them; all finite."""
    x = (rng.randn(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(F32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0], F32)
    idx = rng.randint(0, n, max(n // 7, 1))
    x[idx] = special[rng.randint(0, special.size, idx.size)]
    return x


class Arena:
    """Ranges placed by hand in one source and one destination buffer: range i starts `so` / `do` bytes behind a 16-byte boundary,
    GAP bytes of sentinel lie in front of and behind every destination range.  specs: [(bytes, src offset, dst offset, kind)]."""

    def __init__(self, specs, seed):
        self.specs, self.rng = specs, np.random.RandomState(seed)
        self.pos, cur = [], GAP
        for nbytes, so, do, kind in specs:
            self.pos.append(cur)
            cur = (cur + 16 + nbytes + GAP + 15) // 16 * 16
        self.size = cur + GAP
        self.src_host = np.zeros(self.size, np.uint8)
        self.dst_host = np.full(self.size, SENT, np.uint8)
        for i in range(len(specs)):
            self.fill(i, self.src_host, specs[i][1])
            self.fill(i, self.dst_host, specs[i][2])
        self.src, self.dst = torch.from_numpy(self.src_host).to(DEV), torch.from_numpy(self.dst_host).to(DEV)
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        self.iter = torch.zeros((), dtype=torch.int32, device=DEV)
        entries = [(self.src.data_ptr() + p + so, self.dst.data_ptr() + p + do, nbytes, kind)
                   for p, (nbytes, so, do, kind) in zip(self.pos, specs)]
        self.arr, self.chunks = AV.build_table(entries)
        self.n = len(specs)
        self.table = AV.upload_table(self.arr, self.n, DEV)

    def fill(self, i, buf, off):
        nbytes, kind = self.specs[i][0], self.specs[i][3]
        if nbytes == 0:
            return
        words = _floats(self.rng, nbytes // 4).view(np.uint32) if kind == L.AVG_F32 else self.rng.randint(0, 1 << 32, nbytes // 4, dtype=np.uint64).astype(np.uint32)
        buf[self.pos[i] + off:self.pos[i] + off + nbytes] = words.view(np.uint8)

    def words(self, buf, i, which):
        off = self.specs[i][which]
        return buf[self.pos[i] + off:self.pos[i] + off + self.specs[i][0]].view(np.uint32)

    def new_sources(self):
        """The next iterate: fresh live words, uploaded."""
        for i in range(self.n):
            self.fill(i, self.src_host, self.specs[i][1])
        self.src.copy_(torch.from_numpy(self.src_host))

    def launch(self, s, mode, w, start):
        self.iter.fill_(s)                                  # the counter is written from the host: the kernel reads it
        return AV.run(self.arr, self.table, self.n, self.chunks, self.iter.data_ptr(), mode, w, start)

    def expect(self, s, mode, decay, start):
        """The destination buffer the model predicts from the host copies; the host copy moves on to it."""
        for i, (nbytes, so, do, kind) in enumerate(self.specs):
            p, a = self.words(self.src_host, i, 1), self.words(self.dst_host, i, 2)
            if kind == L.AVG_F32:
                a[:] = AV.model(a.view(F32), p.view(F32), s, mode, decay, start).view(np.uint32)
            else:
                a[:] = p
        return self.dst_host

    def check(self, what):
        torch.cuda.synchronize()
        got = self.dst.cpu().numpy()
        bad = np.nonzero(got != self.dst_host)[0]
        assert bad.size == 0, (what, 'first differing byte', int(bad[0]), 'of', bad.size)
        assert np.array_equal(self.src.cpu().numpy(), self.src_host), (what, 'the sources were written')


SIZES = [4, CH - 4, CH, CH + 4, 3 * CH + 20]
OFFS = [0, 4, 8, 12]
S_SEQ = lambda start: [start - 1, start, start + 1, start + 2, start + 3, 10 ** 6]       # noqa: E731


@pytest.mark.parametrize('mode,decay', [('ema', 0.999), ('ema', 0.5), ('uniform', None)])
def test_kernel_equals_the_model_bit_for_bit(mode, decay):
    """Five sizes x the 16 pairings of source and destination offsets (the 16-byte path with its heads and tails where the two sides
    agree mod 16, the 4-byte path elsewhere), an empty range between two full ones and two int64 (kind 1) ranges, in ONE table; the counter walks start - 1 ... start + 3 and then 10^6 with fresh sources at every step, the average carried along.
    The sentinels around every destination and the sources stay intact."""
    specs = [(nb, so, do, L.AVG_F32) for nb in SIZES for so in OFFS for do in OFFS]
    specs[7:7] = [(0, 0, 0, L.AVG_F32)]                     # empty, between two full ranges
    specs += [(8 * 1031, 8, 8, L.AVG_COPY), (CH + 8, 0, 8, L.AVG_COPY)]
    ar = Arena(specs, seed=len(mode) + int(1000 * (decay or 0)))
    assert ar.n == 83 and ar.chunks == sum(-(-s[0] // CH) for s in specs)
    start, w = 5, AV.one_minus_decay(decay) if mode == 'ema' else 0.0
    for s in S_SEQ(start):
        assert ar.launch(s, AV.MODES[mode], w, start) == 0
        before = ar.dst_host.copy()
        ar.expect(s, mode, decay, start)
        ar.check((mode, s))
        k = s - 1 - start
        moved = not np.array_equal(before, ar.dst_host)
        assert moved, s                                     # (fresh sources every time: a copy moves the destination too)
        if k > 0:                                           # an average, not a copy: the fp32 ranges differ from their sources
            assert not np.array_equal(ar.words(ar.dst_host, 70, 2), ar.words(ar.src_host, 70, 1))
        i64 = len(specs) - 2                                # kind 1: the source's bits at every s
        assert np.array_equal(ar.words(ar.dst_host, i64, 2), ar.words(ar.src_host, i64, 1))
        ar.new_sources()


def test_200_ranges_and_a_null_empty_range():
    rng = np.random.RandomState(200)
    specs = [(int(4 * rng.randint(0, CH // 2)) if i % 9 else 0, int(rng.choice(OFFS)), int(rng.choice(OFFS)), int(i % 5 == 4)) for i in range(200)]
    ar = Arena(specs, seed=201)
    ar.arr[9].src = ar.arr[9].dst = None                    # bytes == 0: null pointers are allowed
    ar.table = AV.upload_table(ar.arr, ar.n, DEV)
    assert ar.n == 200 and sum(1 for s in specs if s[0] == 0) >= 20
    for s, start in ((1, 0), (2, 0), (3, 0), (40, 7)):
        assert ar.launch(s, L.AVG_UNIFORM, 0.0, start) == 0
        ar.expect(s, 'uniform', None, start)
        ar.check(('200 ranges', s))
        ar.new_sources()


def test_validation_codes_and_the_empty_call():
    """Every documented code comes back before anything is launched: the destination keeps its bytes."""
    specs = [(CH + 4, 0, 0, L.AVG_F32), (0, 0, 0, L.AVG_F32), (64, 4, 8, L.AVG_COPY)]
    ar = Arena(specs, seed=5)
    lib, it, w = L.lib(), ar.iter.data_ptr(), float(AV.one_minus_decay(0.9))
    ar.iter.fill_(9)

    def code(table=True, dev=True, n=3, chunks=None, iter_ptr=it, mode=0, w=w, start=0, **edit):
        arr = (L.RdAvgRange * 3).from_buffer_copy(ar.arr)
        for k, (i, v) in edit.items():
            setattr(arr[i], k, v)
        return lib.rd_avg_step(arr if table else None, ar.table.data_ptr() if dev else None, n, ar.chunks if chunks is None else chunks,
                               iter_ptr, mode, w, start, _st())
    assert code(table=False) == -1 and code(dev=False) == -1 and code(iter_ptr=None) == -1 and code(n=-1) == -1
    assert code(n=0, iter_ptr=None) == -1
    assert code(bytes=(0, -4)) == -2 and code(bytes=(0, CH + 6)) == -2 and code(bytes=(2, 63)) == -2
    assert code(src=(0, ar.src.data_ptr() + GAP + 2)) == -3 and code(dst=(2, ar.dst.data_ptr() + 1)) == -3
    assert code(src=(0, None)) == -3 and code(dst=(2, None)) == -3 and code(iter_ptr=it + 2) == -3
    assert code(kind=(0, 2)) == -4 and code(kind=(2, -1)) == -4
    assert code(chunk0=(1, 1)) == -5 and code(chunk0=(0, 1)) == -5 and code(chunks=ar.chunks + 1) == -5 and code(chunks=0) == -5
    assert code(bytes=(0, CH)) == -5                        # one chunk fewer than the column says
    assert code(mode=2) == -6 and code(mode=-1) == -6
    assert code(w=0.0) == -7 and code(w=1.0) == -7 and code(w=-0.25) == -7 and code(w=1.5) == -7 and code(w=float('nan')) == -7
    assert code(start=-1) == -8
    ar.check('after the refused calls')                     # the host copy was never advanced: the destination still equals it
    # the empty calls succeed and launch nothing
    assert code(n=0) == 0 and code(n=0, table=False, dev=False, chunks=0) == 0
    assert code(n=1, chunks=0, bytes=(0, 0)) == 0           # every range empty
    ar.check('after the empty calls')
    # the same descriptor, valid: mode 1 does not read the weight
    assert code(mode=1, w=0.0) == 0
    ar.expect(9, 'uniform', None, 0)
    ar.check('the valid call')


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


BS, S, STEPS = [2, 3, 3], 32, 11
_PLAIN = {}


def _plain(dataset):
    """The twin without averaging, once per dataset: its state behind 11 pipelined steps."""
    if dataset not in _PLAIN:
        tr, batches = _trainer(dataset, BS, S), _batches(dataset, sum(BS), S, STEPS)
        for i in range(STEPS):
            tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        torch.cuda.synchronize()
        b = tr.bank
        _PLAIN[dataset] = dict(params=b.params.cpu(), exp_avg=b.exp_avg.cpu(), exp_avg_sq=b.exp_avg_sq.cpu(), iter=int(tr.ts.iter),
                               buffers={k: v.cpu() for k, v in b.buffers.items()})
    return _PLAIN[dataset]


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(-1)


@pytest.mark.parametrize('dataset,mode,decay,start,compose', [('fundus', 'ema', 0.5, 0, True), ('fundus', 'ema', 0.999, 0, False),
                                                              ('fundus', 'uniform', None, 0, False), ('fundus', 'uniform', None, 4, False),
                                                              ('prostate', 'ema', 0.5, 0, True)])
def test_twin_trainers_average_equals_the_replayed_model_and_training_is_unchanged(dataset, mode, decay, start, compose):
    """Twin A trains alone; twin B averages behind every one of 11 pipelined steps.  The averaged bank equals model() replayed over B's
    per-step read-backs of the parameters and buffers, bit for bit; A and B end bit-identical in parameters, Adam moments and BatchNorm
    buffers.  compose: B also logs every step into the ring and (fundus) composes the image grids in one of the steps -- all three
    users of the one after-step hook fire in that step."""
    batches = _batches(dataset, sum(BS), S, STEPS)
    want = _plain(dataset)
    Bt = _trainer(dataset, BS, S)
    wa = Bt.enable_avg_weights(mode, 0.999 if decay is None else decay, start)
    assert Bt._avg is wa and torch.equal(wa.bank.params, Bt.bank.params)
    log = Bt.enable_step_log(health=True, rows=16) if compose else None
    live = Bt.bank
    avg_p = live.params.cpu().numpy().copy()
    avg_b = {k: v.cpu().numpy().copy() for k, v in live.buffers.items()}
    images = None
    for i in range(STEPS):
        if compose and dataset == 'fundus' and i == 5:
            Bt.arm_tb_images()
        Bt.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        if compose and dataset == 'fundus' and i == 5:
            images = Bt.take_tb_images().images()
        torch.cuda.synchronize()
        s = i + 1
        assert int(Bt.ts.iter) == s
        avg_p = wa.model(avg_p, live.params.cpu().numpy(), s)
        for k, v in live.buffers.items():
            avg_b[k] = wa.model(avg_b[k], v.cpu().numpy(), s) if v.dtype == torch.float32 else v.cpu().numpy().copy()
        got = wa.bank.params.cpu().numpy()
        assert np.array_equal(got.view(np.int32), avg_p.view(np.int32)), ('params', s, int((got.view(np.int32) != avg_p.view(np.int32)).sum()))
    for k, v in wa.bank.buffers.items():
        got = v.cpu().numpy()
        assert got.dtype == avg_b[k].dtype and got.shape == avg_b[k].shape and got.tobytes() == avg_b[k].tobytes(), k
    # an average, not a copy (past the start), and num_batches_tracked is the live counter
    assert not torch.equal(wa.bank.params, live.params)
    nbt = [k for k in live.buffers if k[1].endswith('num_batches_tracked')]
    assert nbt and all(torch.equal(wa.bank.buffers[k], live.buffers[k]) and int(live.buffers[k]) > 0 for k in nbt)
    rm = [k for k in live.buffers if k[1].endswith('running_mean')]
    assert any(not torch.equal(wa.bank.buffers[k], live.buffers[k]) for k in rm)
    # the training itself: bit-identical to the twin without the pass
    assert int(Bt.ts.iter) == want['iter'] == STEPS
    for name in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(_bits(getattr(live, name).cpu()), _bits(want[name])), name
    assert list(live.buffers) == list(want['buffers'])
    for k in live.buffers:
        assert torch.equal(_bits(live.buffers[k].cpu()), _bits(want['buffers'][k])), k
    if compose:
        assert [r['iteration'] for r in Bt.drain_step_log()] == list(range(STEPS)) and log.pending == 0
        if dataset == 'fundus':
            assert len(images) == 7 and all(g.any() for _, g in images[:2])


def test_avg_weights_refuses_a_captured_graph_and_arms_nothing_without_users():
    tr = _trainer('fundus', [1, 1, 1], 32)
    tr._arm_after_step()
    assert tr.ts._after_step is None                        # no user: nothing armed
    tr._graphs = True                                       # (what use_graph=True leaves; nothing is captured here)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_avg_weights('ema', 0.9, 0)
    assert tr._avg is None
    tr._graphs = False
    tr.enable_avg_weights('uniform')
    tr._arm_after_step()
    assert tr.ts._after_step is not None


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_averaged_forward_equals_the_live_forward_while_the_average_is_a_copy(dtype):
    """start beyond the steps taken: the averaged bank is a copy of the live one after every step, and the fused forward over it (its
    own weight pack, its own coefficients) gives the logits of EvalForward.from_trainer bit for bit."""
    from ramdsir.infer import EvalForward
    bs, n = [1, 2, 1], 3
    tr = _trainer('fundus', bs, S, seed=31)
    wa = tr.enable_avg_weights('ema', 0.9, 1000)
    batches = _batches('fundus', sum(bs), S, n)
    for i in range(n):
        tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < n else None)
    torch.cuda.synchronize()
    assert torch.equal(_bits(wa.bank.params), _bits(tr.bank.params)) and wa.bank.params.data_ptr() != tr.bank.params.data_ptr()
    for k, v in tr.bank.buffers.items():
        assert torch.equal(_bits(wa.bank.buffers[k]), _bits(v)), k
    live, mine = EvalForward.from_trainer(tr, dtype), wa.eval_forward(dtype)
    assert mine.owns_pack and mine.bank is wa.bank and mine.wpack is not tr.ts.wpack and wa.eval_forward(dtype) is mine
    g = torch.Generator().manual_seed(32)
    N = 3
    x = torch.empty(live.input(N, S, S).shape).uniform_(-1, 1, generator=g)
    outs = []
    with torch.no_grad():
        for fwd in (live, mine):
            fwd.refresh()
            fwd.input(N, S, S).copy_(x.to(DEV))
            outs.append(fwd.run(N, S, S).float().clone())
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # state_dicts(): the live model's, tensor for tensor, under the reference's keys
    sds = wa.state_dicts()
    for (m, key), mod in zip(CK.MODULE_KEYS, (tr.modules['enc'], tr.modules['dec'], tr.modules['rec'])):
        ref = mod.state_dict()
        assert list(sds[key]) == list(ref)
        assert all(sds[key][k].dtype == ref[k].dtype and sds[key][k].shape == ref[k].shape and torch.equal(sds[key][k], ref[k]) for k in ref), m


# ------------------------------------------------------------------------------------------------------------- the CLI
def _tree(tmp_path, dataset):
    import synth_data as SD
    from test_gpu_ckpt import _truncate
    data = str(tmp_path / 'data')
    if dataset == 'fundus':                                  # batch sizes 3, 6, 7 -> 3, 5 and 2 batches per pass; 5 iterations per epoch
        base = SD.make_fundus_tree(data, n_train=30, n_test=3, hw=(72, 80), vary=False)
        for d, n in ((2, 9), (3, 30), (4, 14)):
            _truncate(os.path.join(base, 'Domain%d_train.list' % d), n)
    else:
        from test_gpu_gpu_val_volumes import _write_volumes
        SD.make_prostate_tree(data, n=6, S=64)               # 3 iterations per epoch
        _write_volumes(os.path.join(data, 'prostate', 'ISBI'), [('Case00', 6, np.float32, (2,)), ('Case01', 5, np.int16, ())])
    return data


def _train(data, dataset, out, extra, epochs=4):
    domains = '1,2,3' if dataset == 'fundus' else '1,2,3,4,5'
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', dataset, '--domain_idxs',
           domains, '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd',
           '--save_path', out, '--epochs', str(epochs), '--num_workers', '0', '--log_every', '3', '--deterministic', '--gpu_data']
    cmd += (['--gpu_val'] if dataset == 'fundus' else ['--gpu_val_volumes', '--test_batch_size', '4']) + ['--fused_val'] + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    log = r.stdout.decode()
    # a process that died of a signal (a GPU fault, an abort) ends the test here: nothing more is started on the device
    assert r.returncode >= 0 and r.returncode not in (134, 139), log[-3000:]
    return r.returncode, log


def _read(out, name):
    p = os.path.join(out, name)
    return open(p, 'rb').read() if os.path.exists(p) else None


def _models(out, prefix):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, prefix + '*.pth')) if prefix != 'model_' or '_avg_' not in p)


def _same_checkpoint(a, b, what):
    assert list(a) == list(b) == [k for _, k in CK.MODULE_KEYS], what
    for part in a:
        assert list(a[part]) == list(b[part]), (what, part)
        for k in a[part]:
            assert a[part][k].dtype == b[part][k].dtype and torch.equal(a[part][k], b[part][k]), (what, part, k)


AVG = ['--avg_weights', 'ema', '--avg_decay', '0.5']


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_the_flag_leaves_every_existing_output_alone(tmp_path, dataset):
    """(a) with --avg_weights ema --avg_decay 0.5 against without: final_model.pth, the validation CSV and the keep-best names are the
    same bytes; final_model_avg.pth has the reference's keys and differs from final_model.pth; the averaged model has its own CSV and
    its own keep-best file.  (b) --avg_start beyond the run: the averaged CSV, final model and keep-best percentage are the live ones."""
    data = _tree(tmp_path, dataset)
    plain, on, late = (str(tmp_path / n) for n in ('plain', 'on', 'late'))
    code, log0 = _train(data, dataset, plain, [], epochs=2)
    assert code == 0, log0[-3000:]
    assert 'avg' not in ' '.join(os.listdir(plain)) and 'averaged' not in log0
    code, log1 = _train(data, dataset, on, AVG, epochs=2)
    assert code == 0, log1[-3000:]
    assert _read(on, 'final_model.pth') == _read(plain, 'final_model.pth') is not None
    assert _read(on, '0_val_log.csv') == _read(plain, '0_val_log.csv') is not None
    assert _models(on, 'model_') == _models(plain, 'model_') and len(_models(plain, 'model_')) == 1
    assert log1.count('Test the averaged model on target domain 0') == 2 and 'not validated per epoch' not in log1
    final, final_avg = (torch.load(os.path.join(on, n), map_location='cpu') for n in ('final_model.pth', 'final_model_avg.pth'))
    assert list(final_avg) == list(final) and all(list(final_avg[p]) == list(final[p]) for p in final)
    assert all(final_avg[p][k].dtype == final[p][k].dtype and final_avg[p][k].shape == final[p][k].shape for p in final for k in final[p])
    assert any(not torch.equal(final_avg[p][k], final[p][k]) for p in final for k in final[p])
    nbt = [(p, k) for p in final for k in final[p] if k.endswith('num_batches_tracked')]
    assert nbt and all(torch.equal(final_avg[p][k], final[p][k]) for p, k in nbt)
    assert len(_read(on, '0_val_log_avg.csv').decode().splitlines()) == 2 and len(_models(on, 'model_avg_')) == 1
    # (b)
    code, log2 = _train(data, dataset, late, ['--avg_weights', 'uniform', '--avg_start', '1000000'], epochs=2)
    assert code == 0, log2[-3000:]
    assert _read(late, 'final_model.pth') == _read(plain, 'final_model.pth')
    assert _read(late, '0_val_log_avg.csv') == _read(late, '0_val_log.csv') == _read(plain, '0_val_log.csv')
    _same_checkpoint(torch.load(os.path.join(late, 'final_model_avg.pth'), map_location='cpu'),
                     torch.load(os.path.join(late, 'final_model.pth'), map_location='cpu'), 'the average is a copy')
    assert [m.replace('model_avg_', 'model_') for m in _models(late, 'model_avg_')] == _models(late, 'model_') and len(_models(late, 'model_')) == 1


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_a_resumed_run_ends_in_the_same_average(tmp_path, dataset):
    """(c) 4 epochs with --ckpt_every 1 against the same run stopped after 2 epochs and resumed: final_model_avg.pth tensor for tensor,
    <target>_val_log_avg.csv and the model_avg_* names are equal (and so are the live outputs).  Fundus: a resume without the flag is
    refused, naming avg_weights."""
    data = _tree(tmp_path, dataset)
    whole, cut = str(tmp_path / 'whole'), str(tmp_path / 'cut')
    code, log = _train(data, dataset, whole, AVG + ['--ckpt_every', '1'])
    assert code == 0 and 'ckpt: 4 snapshots' in log, log[-3000:]
    code, log = _train(data, dataset, cut, AVG + ['--ckpt_every', '1', '--stop_after_epochs', '2'])
    assert code == 0 and 'Stopped after 2 epochs' in log, log[-3000:]
    assert not os.path.exists(os.path.join(cut, 'final_model.pth')) and not os.path.exists(os.path.join(cut, 'final_model_avg.pth'))
    state = os.path.join(cut, 'last_state.pth')
    mid = CK.load_file(state)
    names = [e['name'] for e in mid['table']]
    assert names.index('avg/params') == names.index('hyper') + 1 and names[-1].startswith('avg/buffer/rec/')
    saved = mid['meta']['avg_weights']
    assert (saved['mode'], saved['decay'], saved['start']) == ('ema', 0.5, 0)
    assert saved['val_log_bytes'] == len(_read(cut, '0_val_log_avg.csv')) > 0 and saved['previous_best_avg'] >= 0
    with open(os.path.join(cut, '0_val_log_avg.csv'), 'a') as f:
        f.write('a line of an epoch that was lost with its process\n')
    if dataset == 'fundus':
        code, log = _train(data, dataset, cut, ['--resume', state, '--ckpt_every', '1'])
        assert code != 0 and 'avg_weights' in log and 'holds an averaged model' in log, log[-3000:]
        code, log = _train(data, dataset, cut, ['--avg_weights', 'ema', '--avg_decay', '0.75', '--resume', state, '--ckpt_every', '1'])
        assert code != 0 and 'avg_weights decay' in log, log[-3000:]
    code, log = _train(data, dataset, cut, AVG + ['--resume', state, '--ckpt_every', '1'])
    assert code == 0 and 'continuing at epoch 2' in log and '0_val_log_avg.csv truncated from' in log, log[-3000:]
    for name in ('0_val_log_avg.csv', '0_val_log.csv'):
        assert _read(cut, name) == _read(whole, name) is not None, name
    assert len(_read(whole, '0_val_log_avg.csv').decode().splitlines()) == 4
    assert _models(cut, 'model_avg_') == _models(whole, 'model_avg_') and len(_models(whole, 'model_avg_')) == 1
    assert _models(cut, 'model_') == _models(whole, 'model_')
    for name in ('final_model_avg.pth', 'final_model.pth'):
        _same_checkpoint(torch.load(os.path.join(cut, name), map_location='cpu'), torch.load(os.path.join(whole, name), map_location='cpu'), name)
