"""CPU-only tests of resumable training (train.py --ckpt_every / --resume / --stop_after_epochs, ramdsir/ckpt.py): the descriptor
layout, the numpy model of rd_snapshot's checksums, ReplayCycle against itertools.cycle, the file (atomic replacement, corruption,
versions, the reference's state_dicts out of a snapshot), the host generators, and train.py's refusals.  No GPU call is made."""
import ctypes
import importlib.util
import itertools
import json
import os
import pickle
import random
import subprocess

import numpy as np
import pytest
import torch

import synth_data as SD
from fake_trainer import fake_state as _fake_state, fake_trainer as _fake_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from ramdsir import _lib as L, ckpt as CK       # noqa: E402

M64 = 1 << 64


def _train_module():
    spec = importlib.util.spec_from_file_location('rd_train_ckpt', os.path.join(ROOT, 'ram-dsir_amd', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------------------- descriptor, model
def test_snap_range_size_matches_the_c_compiler(tmp_path):
    src = '#include <stdio.h>\n#include "ramdsir.h"\nint main(){printf("%zu %d %d\\n", sizeof(rd_snap_range_t), RD_SNAP_CHUNK, RD_SNAP_SUM_STRIDE);return 0;}'
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, chunk, stride = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert ctypes.sizeof(L.RdSnapRange) == size == 32 and L.SNAP_CHUNK == chunk and L.SNAP_SUM_STRIDE == stride
    assert 'rd_snapshot' in L.exported_symbols()


def test_checksum_model_against_hand_computed_values():
    u4 = lambda v: np.asarray(v, dtype='<u4')       # noqa: E731
    assert CK.checksums(u4([])) == (0, 0)
    assert CK.checksums(u4([7])) == (7, 7)
    assert CK.checksums(u4([1, 2, 3])) == (6, 14)
    assert CK.checksums(u4([1, 2, 3]).tobytes()) == (6, 14)                 # bytes are read as little-endian words
    assert CK.checksums(np.array([1, 0, 0, 0, 0, 1, 0, 0], np.uint8)) == (1 + 256, 1 + 2 * 256)
    # s2 wraps 2^64 (s1 cannot below 2^32 words): 100000 words of 2^32 - 1
    m, w = 100000, (1 << 32) - 1
    s1, s2 = CK.checksums(np.full(m, w, dtype='<u4'))
    assert s1 == m * w and w * (m * (m + 1) // 2) >= M64 and s2 == (w * (m * (m + 1) // 2)) % M64
    # a permutation keeps s1 and moves s2
    a, b = CK.checksums(u4([5, 9, 11, 2])), CK.checksums(u4([9, 5, 2, 11]))
    assert a[0] == b[0] == 27 and a[1] == 5 + 18 + 33 + 8 and b[1] == 9 + 10 + 6 + 44 and a[1] != b[1]


def test_table_layout_and_chunk_column():
    arr, chunks = CK.build_table([(4096, 4, 0), (8192, 0, 16), (12288, L.SNAP_CHUNK, 16), (16384, L.SNAP_CHUNK + 4, 32 + L.SNAP_CHUNK)])
    assert [e.chunk0 for e in arr] == [0, 1, 1, 2] and chunks == 4
    t = [('a', torch.zeros(3)), ('b', torch.zeros((), dtype=torch.int64)), ('c', torch.zeros(2, 5))]
    table, total = CK.layout(t)
    assert [(e['offset'], e['bytes']) for e in table] == [(0, 12), (16, 8), (32, 40)] and total == 80
    assert table[1] == dict(name='b', dtype='int64', shape=[], offset=16, bytes=8)
    with pytest.raises(ValueError, match='multiple of 4'):
        CK.layout([('h', torch.zeros(3, dtype=torch.bfloat16))])


# ------------------------------------------------------------------------------------------------------------- ReplayCycle
def _drive(front, longest, back, epochs):
    """The training loop's zip: a cycled loader in front of the longest one loses an item in the round in which the longest ends."""
    out = []
    for _ in range(epochs):
        out.append(list(zip(front, longest, back)))
    return out


@pytest.mark.parametrize('n', [1, 2, 5])
@pytest.mark.parametrize('longest', [5, 7])
def test_replay_cycle_equals_itertools_cycle_and_round_trips(n, longest):
    items = [('item', n, i) for i in range(n)]
    long_list = list(range(100, 100 + longest))
    want = _drive(itertools.cycle(items), long_list, itertools.cycle(items), 4)
    front, back = CK.ReplayCycle(items), CK.ReplayCycle(items)
    got = _drive(front, long_list, back, 2)
    assert got == want[:2]
    # the lost item: the cycle in front has been pulled once more per epoch than the one behind
    assert front.state()[1] == (2 * (longest + 1)) % n and back.state()[1] == (2 * longest) % n
    st = pickle.loads(pickle.dumps((front.state(), back.state())))
    front2, back2 = CK.ReplayCycle.from_state(st[0]), CK.ReplayCycle.from_state(st[1])
    assert _drive(front2, long_list, back2, 2) == want[2:]
    assert _drive(front, long_list, back, 2) == want[2:]                    # state() does not disturb the cycle itself


def test_replay_cycle_state_raises_during_the_first_pass_only():
    c = CK.ReplayCycle(['a', 'b', 'c'])
    with pytest.raises(RuntimeError, match='first pass'):
        c.state()
    assert [next(c), next(c)] == ['a', 'b']
    with pytest.raises(RuntimeError, match='2 of 3'):
        c.state()
    assert next(c) == 'c'
    # exactly len(iterable) items: the iterator's end has not been seen yet, and the state is that of an exhausted one
    assert c.state() == (['a', 'b', 'c'], 0)
    d = CK.ReplayCycle.from_state(c.state())
    assert [next(c) for _ in range(4)] == [next(d) for _ in range(4)] == ['a', 'b', 'c', 'a']
    assert list(itertools.islice(CK.ReplayCycle([]), 3)) == []            # an empty iterable ends at once, as cycle's does
    # iter() of the iterable is taken at construction, as itertools.cycle takes it (a DataLoader iterator draws its seed there)
    taken = []

    class Src:
        def __len__(self):
            return 1

        def __iter__(self):
            taken.append(1)
            return iter([0])
    CK.ReplayCycle(Src())
    assert taken == [1]


# ------------------------------------------------------------------------------------------------------------- the file
@pytest.fixture(scope='module')
def fake():
    tr = _fake_trainer()
    return tr, _fake_state(tr)


def test_range_order_is_fixed(fake):
    tr, state = fake
    names = [e['name'] for e in state['table']]
    assert names[:3] == ['params', 'exp_avg', 'exp_avg_sq'] and names[-2:] == ['iter', 'hyper']
    assert names[3:-2] == ['buffer/%s/%s' % k for k in tr.bank.buffers] and any(n.endswith('num_batches_tracked') for n in names)
    assert all(e['offset'] % 16 == 0 and e['bytes'] % 4 == 0 for e in state['table'])
    ends = [e['offset'] + e['bytes'] for e in state['table']]
    assert all(e['offset'] >= end for e, end in zip(state['table'][1:], ends))


def test_file_round_trip_and_a_killed_write_leaves_the_old_file(tmp_path, fake):
    tr, state = fake
    path = str(tmp_path / 'last_state.pth')
    sec = dict(serialise=0.0, write=0.0)
    CK.write_file(path, state, sec)
    assert os.listdir(tmp_path) == ['last_state.pth'] and sec['serialise'] > 0 and sec['write'] > 0
    back = CK.load_file(path)
    assert back['table'] == state['table'] and torch.equal(back['blob'], state['blob']) and back['meta'] == state['meta']
    assert torch.equal(CK.range_tensor(back, 'exp_avg'), tr.bank.exp_avg) and int(CK.range_tensor(back, 'iter')) == 41
    # a writer killed in the middle of the next snapshot: a partial .tmp beside the file
    with open(path + '.tmp', 'wb') as f:
        f.write(open(path, 'rb').read()[:1000])
    assert torch.equal(CK.load_file(path)['blob'], state['blob'])
    # the next complete write replaces both
    newer = dict(state, meta=dict(state['meta'], epoch=2))
    CK.write_file(path, newer)
    assert os.listdir(tmp_path) == ['last_state.pth'] and CK.load_file(path)['meta']['epoch'] == 2


def test_a_flipped_byte_is_refused_with_the_range_name(tmp_path, fake):
    tr, state = fake
    first_dec_buffer = next(e['name'] for e in state['table'] if e['name'].startswith('buffer/dec/'))
    for name in ('exp_avg_sq', first_dec_buffer, 'hyper'):
        e = next(e for e in state['table'] if e['name'] == name)
        bad = dict(state, blob=state['blob'].clone())
        bad['blob'][e['offset'] + e['bytes'] // 2] ^= 0x10
        path = str(tmp_path / 'bad.pth')
        CK.write_file(path, bad)
        with pytest.raises(ValueError, match='range %s is corrupt' % e['name'].replace('.', r'\.')):
            CK.load_file(path)


def test_an_unknown_version_is_refused(tmp_path, fake):
    tr, state = fake
    path = str(tmp_path / 'v.pth')
    CK.write_file(path, dict(state, version=CK.VERSION + 1))
    with pytest.raises(ValueError, match='format version %d' % (CK.VERSION + 1)):
        CK.load_file(path)
    torch.save({'encoder_state_dict': {}}, path)
    with pytest.raises(ValueError, match='not a training-state snapshot'):
        CK.load_file(path)


def test_state_dicts_are_the_reference_keys_in_manifest_order(golden_dir, fake):
    tr, state = fake
    with open(os.path.join(golden_dir, 'state_manifest.json')) as f:
        man = json.load(f)
    sds = CK.state_dicts(state)
    assert list(sds) == ['encoder_state_dict', 'seg_decoder_state_dict', 'rec_decoder_state_dict']
    for (m, key), nm in zip(CK.MODULE_KEYS, ('encoder', 'seg_decoder', 'rec_decoder')):
        sd = sds[key]
        assert [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()] == man[nm], nm
        for k, v in sd.items():
            want = tr.bank.p(m, k) if (m, k) in tr.bank.index else tr.bank.b(m, k)
            assert torch.equal(v, want), (m, k)
    # views of the blob, not copies
    w = sds['seg_decoder_state_dict']['out1.weight']
    assert w.untyped_storage().data_ptr() == state['blob'].untyped_storage().data_ptr()


def test_fingerprint_mismatch_names_the_first_differing_field():
    a = dict(dataset='fundus', domain_idxs=[1, 2, 3], test_domain_idx=0, batch_sizes=[3, 6, 7], H=256, W=256, total_iters=40, dtype='bf16',
             consistency='kd', lambda_rec=0.1, lr=2e-3, num_classes=2, in_channels=3, activation='relu', manifest=[['enc', 'w', [1], 'param', 'float32']])
    CK.compare_fingerprints(a, dict(a))
    with pytest.raises(ValueError, match='total_iters = 40, this run has 50'):
        CK.compare_fingerprints(a, dict(a, total_iters=50, lr=1e-3))       # the first of two
    with pytest.raises(ValueError, match='manifest'):
        CK.compare_fingerprints(a, dict(a, manifest=[['enc', 'w', [2], 'param', 'float32']]))
    assert set(CK.FINGERPRINT_FIELDS) == set(a)


# ------------------------------------------------------------------------------------------------------------- generators
def test_restored_generators_reproduce_the_parameter_datasets_draws(tmp_path):
    from torch.utils.data import DataLoader
    from ramdsir import gpu_data
    base = SD.make_fundus_tree(str(tmp_path), n_train=5, n_test=1, hw=(24, 28), vary=False)
    ds = gpu_data.FundusParams(base_dir=base, split='train', domain_idx_list=[1], is_out_domain=True, test_domain_idx=0)
    dl = DataLoader(ds, batch_size=2, shuffle=True, drop_last=True, num_workers=0, collate_fn=gpu_data.collate)
    random.seed(5), np.random.seed(6), torch.manual_seed(7)
    list(dl)                                                # somewhere in the middle of the three streams
    path = str(tmp_path / 'rng.pth')
    torch.save(CK.host_rng_state(), path)
    first = [list(dl), list(dl)]
    assert first[0] != first[1]
    random.seed(1), np.random.seed(1), torch.manual_seed(1)
    assert [list(dl), list(dl)] != first
    CK.set_host_rng_state(torch.load(path, weights_only=False))
    assert [list(dl), list(dl)] == first                    # the sampler's permutation (torch), partners (numpy), crops and lambda (random)


# ------------------------------------------------------------------------------------------------------------- flags
BASE = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']


def test_parse_defaults_are_unchanged():
    T = _train_module()
    a = T.parse_args(['--save_path', 'x'])
    assert (a.ckpt_every, a.resume, a.stop_after_epochs) == (0, None, 0) and not T.uses_ckpt(a)
    assert (a.norm, a.num_workers, a.log_every, a.tb_images, a.gpu_data, a.fused_val, a.tb_every_iter, a.dtype) == \
        ('bn', 8, 20, 0, False, False, False, None)
    assert T.uses_ckpt(T.parse_args(['--save_path', 'x', '--ckpt_every', '2']))
    assert T.uses_ckpt(T.parse_args(['--save_path', 'x', '--resume', 'f.pth']))


@pytest.mark.parametrize('flags', [['--ckpt_every', '1'], ['--resume', 'f.pth'], ['--ckpt_every', '1', '--stop_after_epochs', '1']])
def test_the_flags_are_refused_with_other_norms_and_with_several_ranks(flags, monkeypatch):
    T = _train_module()
    for norm in ('gn', 'in'):
        with pytest.raises(ValueError, match='--norm %s trains through the modules' % norm):
            T.main(T.parse_args(BASE + flags + ['--norm', norm]))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match=r'one process.*WORLD_SIZE=2'):
        T.main(T.parse_args(BASE + flags))


def test_stop_after_epochs_needs_ckpt_every_and_resume_refuses_an_unknown_version(tmp_path, fake, monkeypatch):
    T = _train_module()
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match='needs --ckpt_every'):
        T.main(T.parse_args(BASE + ['--stop_after_epochs', '2']))
    with pytest.raises(ValueError, match='number of epochs'):
        T.main(T.parse_args(BASE + ['--ckpt_every', '-1']))
    path = str(tmp_path / 'future.pth')
    CK.write_file(path, dict(fake[1], version=99))
    with pytest.raises(ValueError, match='format version 99'):
        T.main(T.parse_args(BASE + ['--resume', path]))
