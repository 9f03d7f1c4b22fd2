"""GPU tests of the BatchNorm re-estimation of the averaged model (train.py --avg_bn_recal, ramdsir/avg_bn.py): rd_bn_recal equals the
numpy model bit for bit between sentinels, the pass equals the model replayed over the statistic slots it read and an independent
CPU forward, the capture leaves the training and the averaged bank bit-identical and holds the step's clean input, and train.py
writes the re-estimated statistics where -- and only where -- the issue of the flag says."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, avg as AV, avg_bn as AB, ckpt as CK, engine as E       # noqa: E402

F32 = np.float32
SLOTS = L.STAT_SLOTS
GAP = 4096                                                  # bytes of sentinel around every destination
SENT = 0xA5


# ------------------------------------------------------------------------------------------------------------- the kernel alone
class Sites:
    """n sites laid out by hand: one fp64 slot buffer per site, the three destinations of every site in ONE byte arena with GAP
    bytes of sentinel in front of and behind each.  Site i: C = Cs[i], nslots, count and conv_bias (or NULL) cycle."""

    def __init__(self, Cs, seed):
        self.rng = np.random.RandomState(seed)
        self.Cs, self.n = list(Cs), len(Cs)
        self.nslots = [(8, 64)[i % 2] for i in range(self.n)]
        self.count = [(1.0, 2.0, 16384.0)[(i // 2) % 3] for i in range(self.n)]
        self.bias_host = [None if i % 3 == 2 else self.rng.normal(0, 1, c).astype(F32) for i, c in enumerate(self.Cs)]
        self.bias = [None if b is None else torch.from_numpy(b).to(DEV) for b in self.bias_host]
        self.slots_host = [None] * self.n
        self.slots = [torch.zeros(SLOTS, c, 2, dtype=torch.float64, device=DEV) for c in self.Cs]
        self.off, cur = [], GAP
        for c in self.Cs:
            o = []
            for nbytes in (4 * c, 4 * c, 8):
                o.append(cur)
                cur = (cur + nbytes + GAP + 15) // 16 * 16
            self.off.append(o)
        self.size = cur + GAP
        self.dst_host = np.full(self.size, SENT, np.uint8)
        for i, c in enumerate(self.Cs):                     # old contents: NaN (k = 0 must not read them), then whatever the model leaves
            self.vec(self.dst_host, i, 0)[:] = np.nan
            self.vec(self.dst_host, i, 1)[:] = np.nan
            self.nbt(self.dst_host, i)[:] = -7
        self.dst = torch.from_numpy(self.dst_host).to(DEV)
        assert self.dst.data_ptr() % 16 == 0
        self.arr = (L.RdBnRecalSite * self.n)()
        for i, r in enumerate(self.arr):
            r.stats = self.slots[i].data_ptr()
            r.conv_bias = None if self.bias[i] is None else self.bias[i].data_ptr()
            r.running_mean, r.running_var, r.num_batches_tracked = (self.dst.data_ptr() + o for o in self.off[i])
            r.count, r.C, r.nslots = self.count[i], self.Cs[i], self.nslots[i]
        self.table = AB.upload_table(self.arr, self.n, DEV)
        self.max_c = max(self.Cs)

    def vec(self, buf, i, which):
        o = self.off[i][which]
        return buf[o:o + 4 * self.Cs[i]].view(F32)

    def nbt(self, buf, i):
        o = self.off[i][2]
        return buf[o:o + 8].view(np.int64)

    def new_slots(self):
        """Chosen doubles straight into the slot buffers: sums of many magnitudes, second moments that leave the variance positive,
        zero and (clamped) negative; copies behind a site's nslots hold junk that must not be read."""
        for i, c in enumerate(self.Cs):
            s = np.empty((SLOTS, c, 2), np.float64)
            s[:, :, 0] = self.rng.normal(0, 3, (SLOTS, c)) * 10.0 ** self.rng.uniform(-3, 2, (1, c))
            s[:, :, 1] = self.rng.uniform(0, 50, (SLOTS, c)) * 10.0 ** self.rng.uniform(-2, 3, (1, c))
            s[self.nslots[i]:] = 1e300
            self.slots_host[i] = s
            self.slots[i].copy_(torch.from_numpy(s))

    def launch(self, k, **kw):
        return AB.run(kw.get('arr', self.arr), kw.get('table', self.table), kw.get('n', self.n), kw.get('max_c', self.max_c), k)

    def expect(self, k):
        for i in range(self.n):
            rm, rv, nbt = AB.model(self.vec(self.dst_host, i, 0), self.vec(self.dst_host, i, 1), self.slots_host[i], self.count[i],
                                   self.bias_host[i], k, self.nslots[i])
            self.vec(self.dst_host, i, 0)[:] = rm
            self.vec(self.dst_host, i, 1)[:] = rv
            self.nbt(self.dst_host, i)[:] = nbt

    def check(self, what):
        torch.cuda.synchronize()
        got = self.dst.cpu().numpy()
        bad = np.nonzero(got != self.dst_host)[0]
        assert bad.size == 0, (what, 'first differing byte', int(bad[0]), 'of', bad.size)
        for i in range(self.n):
            assert np.array_equal(self.slots[i].cpu().numpy().view(np.int64), self.slots_host[i].view(np.int64)), (what, 'slots written', i)


C_SET = [1, 16, 17, 256]


@pytest.mark.parametrize('n_sites,rot', [(n, r) for n in (1, 7, 27, 60) for r in range(4)] + [(7, 4)])
def test_kernel_equals_the_model_bit_for_bit(n_sites, rot):
    """Sites of C in {1, 16, 17, 256} (rot 4: 700 among them, more than one workgroup per site) in ONE table -- a ragged or idle
    workgroup per narrower site --, nslots in {8, 64}, count in {1, 2, 16384}, conv_bias given or NULL; k walks 0, 1, 2, 10^6 with
    fresh slots every time and the running values carried along.  Every byte of the destination arena -- the vectors, the int64
    counters, the 4 KiB sentinels -- equals the model's; the slots are only read."""
    cs = (C_SET + [700]) if rot == 4 else C_SET
    st = Sites([cs[(i + rot) % len(cs)] for i in range(n_sites)], seed=100 * n_sites + rot)
    for k in (0, 1, 2, 10 ** 6):
        st.new_slots()
        assert st.launch(k) == 0
        st.expect(k)
        st.check((n_sites, rot, k))
        assert all(int(st.nbt(st.dst_host, i)[0]) == k + 1 for i in range(st.n))
        assert all(np.isfinite(st.vec(st.dst_host, i, w)).all() for i in range(st.n) for w in (0, 1))


def test_a_refused_call_touches_nothing():
    st = Sites([16, 17, 256, 1], seed=9)
    st.new_slots()
    assert st.launch(0) == 0
    st.expect(0)
    st.check('valid')

    def edited(i, **kw):
        arr = (L.RdBnRecalSite * st.n).from_buffer_copy(st.arr)
        for k, v in kw.items():
            setattr(arr[i], k, v)
        return arr
    assert st.launch(-1) == -2
    assert st.launch(1, arr=None) == -1 and st.launch(1, table=None) == -1 and st.launch(1, n=0) == -1 and st.launch(1, n=4097) == -1
    assert st.launch(1, max_c=255) == -4 and st.launch(1, arr=edited(1, C=0)) == -4
    assert st.launch(1, arr=edited(2, running_var=None)) == -3 and st.launch(1, arr=edited(0, num_batches_tracked=None)) == -3
    assert st.launch(1, arr=edited(3, stats=None)) == -3
    assert st.launch(1, arr=edited(0, count=0.0)) == -5
    assert st.launch(1, arr=edited(1, nslots=12)) == -6 and st.launch(1, arr=edited(1, nslots=0)) == -6
    st.check('after the refused calls')                     # the host copy was never advanced
    assert st.launch(1) == 0
    st.expect(1)
    st.check('the valid call behind them')


# ------------------------------------------------------------------------------------------------------------- the pass
def _oracle_states():
    from oracle import unet as OU
    return OU, OU.encoder_state(seed=1), OU.decoder_state(seed=2), OU.rec_decoder_state(num_classes=3, num_domains=3, seed=3)


def _banks():
    """A live bank with the oracle's states (non-trivial running statistics), its averaged copy and the third set of buffers."""
    from ramdsir import step as S
    OU, enc, dec, rec = _oracle_states()
    bank, mods = S.make_bank(DEV, 3, 16, 2, 3)
    g = torch.Generator().manual_seed(4)
    for m, sd in (('enc', enc), ('dec', dec), ('rec', rec)):
        for k in sd:
            if k.endswith('running_mean'):
                sd[k] = torch.randn(sd[k].shape, generator=g)
            elif k.endswith('running_var'):
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
            elif k.endswith('num_batches_tracked'):
                sd[k] = torch.tensor(11)
        S.load_state(bank, m, sd)
    avg = AV.AveragedBank(bank)
    return bank, mods, avg, AB.RecalBank(avg), (enc, dec)


def _forward(view, mods, dtype, N):
    wpack = E.WeightPack(view, mods[:2], dtype)
    fwd = AB.RecalForward(view, wpack, dtype, N, 32, 32)
    wpack.refresh(L._stream())
    return fwd


def _inputs(N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(N, 32, 32, 3, generator=g) * 2 - 1).to(dtype) for _ in range(K)]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(-1).view(torch.int32) if t.dtype == torch.float32 else t.view(-1)


def _snapshot(bank):
    return {k: v.detach().cpu().clone() for k, v in bank.buffers.items()}, bank.params.detach().cpu().clone()


def _same(bank, snap, what):
    for k, v in bank.buffers.items():
        assert torch.equal(_bits(v), _bits(snap[0][k])), (what, k)
    assert torch.equal(_bits(bank.params), _bits(snap[1])), what


def _site_keys(fwd):
    """(module, running_mean key) of every site, in the table's order."""
    out = []
    for s in fwd.sites:
        o = s[8]
        out.append((o.norm.mname, o.norm.key(0, 'running_mean')))
    return out


def _replay(fwd, xs, state=None):
    """Runs the batches; returns (the model replayed over the slots read back after each batch, the slots)."""
    state = [None] * fwd.n_sites if state is None else state
    seen = []
    for k, x in enumerate(xs):
        fwd.input().copy_(x.to(DEV))
        fwd.run(k)
        torch.cuda.synchronize()
        slots = [fwd.slots(i).cpu().numpy().copy() for i in range(fwd.n_sites)]
        seen.append(slots)
        for i, s in enumerate(fwd.sites):
            cb = None if s[1] is None else _conv_bias(fwd, i)
            old = state[i] if state[i] is not None else (np.full(s[6], np.nan, F32), np.full(s[6], np.nan, F32))
            state[i] = AB.model(old[0], old[1], slots[i], s[5], cb, k, s[7])[:2]
    return state, seen


def _conv_bias(fwd, i):
    """The conv bias of site i from the bank (the site record holds its pointer)."""
    o = fwd.sites[i][8]
    m, name = o.name.split('.', 1)
    t = fwd.bank.p(m, name + '.bias')
    assert t.data_ptr() == fwd.sites[i][1]
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('N', [4, 5])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_the_pass_equals_the_model_replayed_over_its_slots(dtype, N):
    """Fundus 32^2 with batch sizes summing to 4, Prostate 32^2 with 5 x 1 (16 resp. 20 values per channel at the bottom level).
    (a) K = 1: running_mean has the bits of the mean vector the plan's finalize saved, running_var is model() of the slots read back.
    (b) K = 3: every site equals model() replayed over the slots read back after each batch; the slot sums of a batch do not depend on
    the batch in front of it (they start from zero).  (d) a second pass gives the same bits; the averaged bank's own buffers, the
    live bank and the parameters are untouched."""
    live, mods, avg, view, _ = _banks()
    snaps = _snapshot(live), _snapshot(avg)
    fwd = _forward(view, mods, dtype, N)
    assert fwd.n_sites == 26 and fwd.launches()['rd_bn_recal'] == 1 and fwd.launches()['rd_conv'] == 27
    xs = _inputs(N, 3, dtype, 7 + N)
    # (a)
    state, seen1 = _replay(fwd, xs[:1])
    for i, s in enumerate(fwd.sites):
        o = s[8]
        assert torch.equal(_bits(s[2]), _bits(o.mean)), ('running_mean is not the saved mean', i)
        assert np.array_equal(s[2].cpu().numpy().view(np.int32), state[i][0].view(np.int32)), i
        assert np.array_equal(s[3].cpu().numpy().view(np.int32), state[i][1].view(np.int32)), i
        assert int(s[4]) == 1
        assert np.isfinite(state[i][0]).all() and (state[i][1] >= 0).all()
    assert any(sl.any() for sl in seen1[0])
    # (b)
    state, seen = _replay(fwd, xs)
    for i, s in enumerate(fwd.sites):
        assert np.array_equal(s[2].cpu().numpy().view(np.int32), state[i][0].view(np.int32)), i
        assert np.array_equal(s[3].cpu().numpy().view(np.int32), state[i][1].view(np.int32)), i
        assert int(s[4]) == 3
        # which copy a workgroup adds into depends on scheduling, the sums over the copies do not: two sums of 64 float64 terms lie
        # within 2 * 64 * 2^-53 * sum |term| of each other; statistics left over from the batch in front would be of the order of the sum
        a, b = seen[0][i].sum(0), seen1[0][i].sum(0)
        assert (np.abs(a - b) <= 64 * 2.0 ** -52 * np.abs(seen1[0][i]).sum(0)).all(), ('stale statistics', i)
    first = {k: v.detach().cpu().clone() for k, v in view.buffers.items()}
    # (d)
    _replay(fwd, xs)
    for k, v in view.buffers.items():
        assert torch.equal(_bits(v), _bits(first[k])), k
    _same(live, snaps[0], 'live')
    _same(avg, snaps[1], 'averaged')
    changed = [k for k in view.buffers if not torch.equal(_bits(view.buffers[k]), _bits(avg.buffers[k]))]
    assert changed and all(k[0] in ('enc', 'dec') for k in changed) and len(changed) == 3 * 26
    assert all(view.buffers[k] is avg.buffers[k] for k in view.buffers if k[0] == 'rec')


@pytest.mark.parametrize('N', [4, 5])
def test_the_pass_equals_an_independent_forward_on_the_cpu(N, monkeypatch):
    """(c) fp32: the oracle's encoder / decoder forward in training mode on the CPU over the same K batches and parameters, with its
    momentum set to 1 so that its running buffers hold each batch's own statistics, averaged here in float64.  All sites at
    rtol 1e-4, atol 1e-6 (the tolerance tests/test_gpu_modules.py applies to running statistics against the reference fixtures)."""
    live, mods, avg, view, (enc, dec) = _banks()
    OU = _oracle_states()[0]
    monkeypatch.setattr(OU, 'MOMENTUM', 1.0)
    K = 3
    fwd = _forward(view, mods, torch.float32, N)
    xs = _inputs(N, K, torch.float32, 21 + N)
    for k, x in enumerate(xs):
        fwd.input().copy_(x.to(DEV))
        fwd.run(k)
    torch.cuda.synchronize()
    acc = {}
    e, d = OU.clone_state(enc), OU.clone_state(dec)
    with torch.no_grad():
        for x in xs:
            feats = OU.encoder_forward(x.permute(0, 3, 1, 2).contiguous(), e, training=True)
            OU.decoder_forward(feats, d, training=True)
            for m, sd in (('enc', e), ('dec', d)):
                for key, v in sd.items():
                    if key.endswith('running_mean') or key.endswith('running_var'):
                        acc[(m, key)] = acc.get((m, key), 0) + v.double().numpy() / K
    keys = _site_keys(fwd)
    assert len(set(keys)) == 26
    for (m, key), s in zip(keys, fwd.sites):
        for leaf, got in (('running_mean', s[2]), ('running_var', s[3])):
            ref = acc[(m, key.replace('running_mean', leaf))]
            assert np.allclose(got.cpu().numpy().astype(np.float64), ref, rtol=1e-4, atol=1e-6), (m, key, leaf, float(np.abs(got.cpu().numpy() - ref).max()))
        assert int(s[4]) == K


# ------------------------------------------------------------------------------------------------------------- the trainers
from test_gpu_avg_weights import _trainer, _batches, BS, S, STEPS       # noqa: E402

K_RING = 3


def _arm(tr, composed, with_ring):
    wa = tr.enable_avg_weights('uniform', 0.999, 2)
    if composed:                                            # every stage of the tail and the other hook users, to show the hook composes
        tr.enable_grad_guard(5.0)
        tr.enable_optim(weight_decay=1e-2, lr_schedule='cosine', warmup_iters=2)
        tr.enable_grad_accum(2)
    else:
        tr.enable_step_log(health=True, rows=16)
    return wa, (tr.enable_avg_bn_recal(K_RING) if with_ring else None)


@pytest.mark.parametrize('dataset,composed', [('fundus', False), ('fundus', True), ('prostate', False), ('prostate', True)])
def test_twin_trainers_the_capture_changes_nothing_and_holds_the_clean_input(dataset, composed):
    """Twin A averages; twin B also captures the last 3 of 11 pipelined steps and re-estimates.  Live model, Adam moments and
    averaged bank are bit-identical after every step; the ring holds the first-B halves of the input slots read back at the captured
    steps (both slots occur); the pass equals a RecalForward driven by hand over those read-backs.  composed: guard + grouped Adam +
    accumulation (+ the image grids in a captured step, fundus) on both twins; otherwise the per-step ring shares the hook."""
    batches = _batches(dataset, sum(BS), S, STEPS)
    A, Bt = _trainer(dataset, BS, S), _trainer(dataset, BS, S)
    (wa, _), (wb, recal) = _arm(A, composed, False), _arm(Bt, composed, True)
    assert recal.K == K_RING and wb.bn_recal is recal and wa.bn_recal is None and wb.settings()['bn_recal'] == K_RING
    assert 'bn_recal' not in wa.settings()
    Bn = sum(BS)
    reads, slots = [], []
    recal.begin_epoch()
    for i in range(STEPS):
        captured = i >= STEPS - K_RING
        for tr in (A, Bt):
            if composed and dataset == 'fundus' and i == STEPS - 2:
                tr.arm_tb_images()
            if tr is Bt and captured:
                slot = Bt.ts._slot
                Bt.arm_bn_capture()
            tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
            if composed and dataset == 'fundus' and i == STEPS - 2:
                assert len(tr.take_tb_images().images()) == 7
        torch.cuda.synchronize()
        if captured:
            slots.append(slot)
            reads.append(Bt.ts.xbufs[slot][:Bn].clone())
        for name in ('params', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(_bits(getattr(A.bank, name)), _bits(getattr(Bt.bank, name))), (name, i)
        assert torch.equal(_bits(wa.bank.params), _bits(wb.bank.params)), i
        for k in A.bank.buffers:
            assert torch.equal(_bits(A.bank.buffers[k]), _bits(Bt.bank.buffers[k])), (k, i)
            assert torch.equal(_bits(wa.bank.buffers[k]), _bits(wb.bank.buffers[k])), (k, i)
    assert int(A.ts.iter) == int(Bt.ts.iter) and not torch.equal(wb.bank.params, Bt.bank.params)
    assert set(slots) == {0, 1} and recal.ring.count == K_RING
    assert tuple(recal.ring.buf.shape) == (K_RING, Bn, S, S, Bt.ts.xbufs[0].shape[-1]) and recal.ring.buf.dtype == Bt.ts.dtype
    for k in range(K_RING):
        assert torch.equal(recal.ring.buf[k].view(torch.int16), reads[k].view(torch.int16)), k
        assert reads[k][..., :3].float().abs().max() > 0
    # the pass, against the forward driven by hand over the read-backs
    avg_before = _snapshot(wb.bank)
    assert recal.run_pass() == K_RING
    torch.cuda.synchronize()
    _same(wb.bank, avg_before, 'the averaged bank')
    hand_bank = AB.RecalBank(wb.bank)
    mods = [('enc', Bt.modules['enc']._specs), ('dec', Bt.modules['dec']._specs)]
    hand = AB.RecalForward(hand_bank, E.WeightPack(hand_bank, mods, Bt.ts.dtype), Bt.ts.dtype, Bn, S, S)
    hand.wpack.refresh(L._stream())
    for k in range(K_RING):
        hand.input().copy_(reads[k][..., :3])
        hand.run(k)
    torch.cuda.synchronize()
    for key, v in recal.bank.buffers.items():
        assert torch.equal(_bits(v), _bits(hand_bank.buffers[key])), key
    nbt = [k for k in recal.bank.buffers if k[1].endswith('num_batches_tracked') and k[0] != 'rec']
    assert len(nbt) == 26 and all(int(recal.bank.buffers[k]) == K_RING for k in nbt)
    rm = [k for k in recal.bank.buffers if k[1].endswith('running_mean') and k[0] != 'rec']
    assert all(not torch.equal(recal.bank.buffers[k], wb.bank.buffers[k]) for k in rm)
    # what reads the result: the state_dicts (keys and order of the live model's) and the fused forward over the view
    sds, plain = wb.state_dicts(), wa.state_dicts()
    for (m, key), mod in zip(CK.MODULE_KEYS, (Bt.modules['enc'], Bt.modules['dec'], Bt.modules['rec'])):
        assert list(sds[key]) == list(mod.state_dict()) == list(plain[key])
        for name, t in sds[key].items():
            same = torch.equal(_bits(t), _bits(plain[key][name]))
            stat = name.split('.')[-1] in ('running_mean', 'running_var', 'num_batches_tracked')
            assert same == (m == 'rec' or not stat), (m, name)
    assert wb.eval_forward().bank is recal.bank and wa.eval_forward().bank is wa.bank
    # a ring that is full refuses a fourth capture of the epoch; the next epoch starts it again
    with pytest.raises(RuntimeError, match='ring holds'):
        recal.capture(0)
    recal.begin_epoch()
    assert recal.ring.count == 0 and recal.run_pass() == 0


# ------------------------------------------------------------------------------------------------------------- the CLI
from test_gpu_avg_weights import _tree, _train, _read, _models       # noqa: E402

UNI = ['--avg_weights', 'uniform']
STATS = ('running_mean', 'running_var', 'num_batches_tracked')


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_the_flag_moves_only_the_averaged_batchnorm_statistics_and_resumes(tmp_path, dataset):
    """4 epochs, --deterministic --gpu_data --fused_val --avg_weights uniform, with and without --avg_bn_recal 2: final_model.pth, both
    CSV logs of the live model and its keep-best names are the same bytes; in final_model_avg.pth every parameter and every rec_decoder
    buffer is bit-identical, every encoder / seg-decoder num_batches_tracked is 2 and a running_mean differs.  The run stopped after 2
    epochs and resumed ends in the same final_model_avg.pth, _val_log_avg.csv and model_avg_* names; a resume under another K is
    refused.  --avg_bn_recal 0 spelled out equals the flag left away."""
    data = _tree(tmp_path, dataset)
    off, zero, on, cut = (str(tmp_path / n) for n in ('off', 'zero', 'on', 'cut'))
    code, log0 = _train(data, dataset, off, UNI)
    assert code == 0 and 'avg_bn_recal: ' not in log0, log0[-3000:]
    code, log = _train(data, dataset, zero, UNI + ['--avg_bn_recal', '0'])
    assert code == 0 and 'avg_bn_recal: ' not in log, log[-3000:]
    code, log1 = _train(data, dataset, on, UNI + ['--avg_bn_recal', '2', '--ckpt_every', '1'])
    assert code == 0 and 'avg_bn_recal: the last 2 batches' in log1 and '26 BatchNorm sites' in log1, log1[-3000:]
    names = ['final_model.pth', '0_val_log.csv', 'final_model_avg.pth', '0_val_log_avg.csv']
    for name in names:
        assert _read(zero, name) == _read(off, name) is not None, name
    for name in names[:2]:
        assert _read(on, name) == _read(off, name), name
    for d in (zero, on):
        assert _models(d, 'model_') == _models(off, 'model_') and len(_models(off, 'model_')) == 1
        assert _models(zero, 'model_avg_') == _models(off, 'model_avg_')
    a, b = (torch.load(os.path.join(d, 'final_model_avg.pth'), map_location='cpu') for d in (off, on))
    assert list(a) == list(b) == [k for _, k in CK.MODULE_KEYS]
    moved = 0
    for part in a:
        assert list(a[part]) == list(b[part])
        for k in a[part]:
            leaf = k.split('.')[-1]
            assert a[part][k].dtype == b[part][k].dtype and a[part][k].shape == b[part][k].shape
            if leaf not in STATS or part.startswith('rec'):
                assert torch.equal(_bits(a[part][k]), _bits(b[part][k])), (part, k)
            elif leaf == 'num_batches_tracked':
                assert int(b[part][k]) == 2 and int(a[part][k]) > 2, (part, k)
            else:
                assert torch.isfinite(b[part][k]).all(), (part, k)
                moved += leaf == 'running_mean' and not torch.equal(a[part][k], b[part][k])
    assert moved >= 1
    assert len(_read(on, '0_val_log_avg.csv').decode().splitlines()) == 4 and len(_models(on, 'model_avg_')) == 1
    # the snapshot: the averaged ranges are what they were, K travels in meta['avg_weights']
    state = CK.load_file(os.path.join(on, 'last_state.pth'))
    assert state['meta']['avg_weights']['bn_recal'] == 2
    assert not any('recal' in e['name'] or 'ring' in e['name'] for e in state['table'])
    # stopped after 2 epochs and resumed
    code, log = _train(data, dataset, cut, UNI + ['--avg_bn_recal', '2', '--ckpt_every', '1', '--stop_after_epochs', '2'])
    assert code == 0 and 'Stopped after 2 epochs' in log, log[-3000:]
    last = os.path.join(cut, 'last_state.pth')
    if dataset == 'fundus':
        for other in (['--avg_bn_recal', '3'], []):
            code, log = _train(data, dataset, cut, UNI + other + ['--resume', last, '--ckpt_every', '1'])
            assert code != 0 and 'bn_recal' in log, log[-3000:]
    code, log = _train(data, dataset, cut, UNI + ['--avg_bn_recal', '2', '--resume', last, '--ckpt_every', '1'])
    assert code == 0 and 'continuing at epoch 2' in log, log[-3000:]
    for name in names:
        if name.endswith('.csv'):
            assert _read(cut, name) == _read(on, name) is not None, name
    assert _models(cut, 'model_avg_') == _models(on, 'model_avg_') and _models(cut, 'model_') == _models(on, 'model_')
    c = torch.load(os.path.join(cut, 'final_model_avg.pth'), map_location='cpu')
    for part in b:
        assert list(c[part]) == list(b[part])
        for k in b[part]:
            assert torch.equal(_bits(c[part][k]), _bits(b[part][k])), (part, k)
