"""CPU-only tests of train.py --avg_weights (ramdsir/avg.py, rd_avg_step's descriptor): the struct layout, the numpy model of the
kernel's arithmetic against rows worked out in exact rational arithmetic, the range table over a CPU ParamBank, the averaged
state_dicts against the reference's manifest, train.py's refusals, and the averaged ranges in a training-state file.  No GPU call."""
import ctypes
import importlib.util
import json
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from ramdsir import _lib as L, avg as AV, ckpt as CK       # noqa: E402
from fake_trainer import fake_state as _fake_state, fake_trainer as _fake_trainer       # noqa: E402

F32 = np.float32


def _train_module():
    spec = importlib.util.spec_from_file_location('rd_train_avg', os.path.join(ROOT, 'ram-dsir_amd', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bits(a):
    return np.asarray(a, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------- descriptor
def test_avg_range_size_matches_the_c_compiler(tmp_path):
    src = '#include <stdio.h>\n#include "ramdsir.h"\nint main(){printf("%zu %d\\n", sizeof(rd_avg_range_t), RD_AVG_CHUNK);return 0;}'
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, chunk = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert ctypes.sizeof(L.RdAvgRange) == size == 40 and L.AVG_CHUNK == chunk
    assert 'rd_avg_step' in L.exported_symbols()


# ------------------------------------------------------------------------------------------------------------- the model
def _round_f32(x):
    """A Fraction rounded to the nearest float32, ties to even, by integer arithmetic (normal and denormal range, no overflow)."""
    if x == 0:
        return F32(0)
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = math.floor(math.log2(x))
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = x / ulp
    n, r = q.numerator // q.denominator, q - q.numerator // q.denominator
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return F32(sign * float(n * ulp))                       # n * ulp has at most 24 significant bits: the conversions are exact


def _fr(v):
    return Fraction(float(v))


def _three_roundings(a, p, w):
    d = _round_f32(_fr(p) - _fr(a))
    t = _round_f32(_fr(w) * _fr(d))
    return _round_f32(_fr(a) + _fr(t))


def test_model_copies_until_averaging_starts():
    a, p = np.array([1.0, -2.0, 0.0], F32), np.array([3.0, 5e-41, -0.0], F32)       # a denormal and a negative zero among the live words
    for mode in ('ema', 'uniform'):
        for s, start in ((0, 0), (1, 0), (3, 5), (6, 5)):                           # k = -1, 0, -3, 0
            out = AV.model(a, p, s, mode, decay=0.5, start=start)
            assert np.array_equal(_bits(out), _bits(p)) and out is not p, (mode, s, start)


def test_model_rows_worked_out_by_hand():
    a, p = np.array([1.0, 8.0], F32), np.array([3.0, 2.0], F32)
    # k = 1.  ema, decay 0.5: 1 + 0.5 (3 - 1) = 2, 8 + 0.5 (2 - 8) = 5; uniform: w = 1 / 2, the mean of two points
    assert AV.model(a, p, 2, 'ema', decay=0.5).tolist() == [2.0, 5.0]
    assert AV.model(a, p, 2, 'uniform').tolist() == [2.0, 5.0]
    assert AV.model(a, p, 7, 'uniform', start=5).tolist() == [2.0, 5.0]             # k = 7 - 1 - 5
    # k = 2, uniform: w = float32(1 / 3); 1 + w 2 and 8 - w 6, each product and sum rounded
    w3 = _round_f32(Fraction(1, 3))
    want = [_three_roundings(x, y, w3) for x, y in zip(a, p)]
    assert np.array_equal(_bits(AV.model(a, p, 3, 'uniform')), _bits(want))
    # ema, decay 0.75: w = 0.25 exactly; 1 + 0.5 = 1.5, 8 - 1.5 = 6.5
    assert AV.model(a, p, 9, 'ema', decay=0.75).tolist() == [1.5, 6.5]
    # the EMA weight is formed in float32: 1 - float32(0.999), not float32(0.001)
    w = AV.one_minus_decay(0.999)
    assert w.dtype == F32 and w == _round_f32(1 - _fr(F32(0.999))) and w != F32(0.001)
    assert np.array_equal(_bits(AV.model([0.0], [1.0], 5, 'ema', decay=0.999)), _bits([w]))


def test_model_at_a_million_steps():
    # uniform, k = 10^6: w = float32(1) / float32(1000001), correctly rounded; from a = 0 towards p = 1 the result is w itself
    w = _round_f32(Fraction(1, 1000001))
    assert int(_bits(w)) == 897988532
    s = 10 ** 6 + 1
    assert np.array_equal(_bits(AV.model([0.0], [1.0], s, 'uniform')), _bits([w]))
    assert np.array_equal(_bits(AV.model([0.0], [1.0], s + 4, 'uniform', start=4)), _bits([w]))
    a, p = F32(0.37521), F32(-1.25e-3)
    assert np.array_equal(_bits(AV.model([a], [p], s, 'uniform')), _bits([_three_roundings(a, p, w)]))
    # ema: k does not enter
    assert np.array_equal(_bits(AV.model([a], [p], s, 'ema', decay=0.999)), _bits(AV.model([a], [p], 2, 'ema', decay=0.999)))


def test_model_is_the_three_rounding_form_not_an_fma():
    """A row on which a + round(w d) and the single rounding of a + w d differ in the last bit."""
    a, p = np.array([-1090585060], np.int32).view(F32), np.array([1073150696], np.int32).view(F32)      # -0.49803245, 1.929532
    w = AV.one_minus_decay(0.999)
    d = _round_f32(_fr(p[0]) - _fr(a[0]))
    three = _three_roundings(a[0], p[0], w)
    fused = _round_f32(_fr(a[0]) + _fr(w) * _fr(d))
    assert int(_bits(three)) == -1090666514 and int(_bits(fused)) == -1090666515
    got = AV.model(a, p, 2, 'ema', decay=0.999)
    assert np.array_equal(_bits(got), _bits([three])) and not np.array_equal(_bits(got), _bits([fused]))


def test_model_on_random_words_equals_exact_arithmetic():
    rng = np.random.RandomState(11)
    a = np.concatenate([rng.randn(40).astype(F32), np.array([0.0, -0.0, 1e-40, -3e-42], F32)])
    p = np.concatenate([rng.randn(40).astype(F32) * F32(1e-3), np.array([-0.0, 0.0, -2e-41, 1e-38], F32)])
    for mode, s, w in (('ema', 3, AV.one_minus_decay(0.999)), ('uniform', 7, _round_f32(Fraction(1, 7)))):      # k = 6: 1 / (k + 1)
        want = [_three_roundings(x, y, w) for x, y in zip(a, p)]
        assert np.array_equal(_bits(AV.model(a, p, s, mode, decay=0.999)), _bits(want)), mode


# ------------------------------------------------------------------------------------------------------------- the table
@pytest.fixture(scope='module')
def fake():
    tr = _fake_trainer()
    return tr, AV.WeightAverage(tr, 'ema', 0.5, 7)


def test_build_table_chunk_column():
    C = L.AVG_CHUNK
    arr, chunks = AV.build_table([(4096, 8192, 4, 0), (0, 0, 0, 1), (16, 32, C, 0), (48, 64, C + 4, 1), (80, 96, 3 * C + 20, 0)])
    assert [e.chunk0 for e in arr] == [0, 1, 1, 2, 4] and chunks == 8
    assert [(e.src, e.dst, e.bytes, e.kind) for e in arr][3] == (48, 64, C + 4, 1)
    assert AV.build_table([])[1] == 0


def test_range_table_over_a_cpu_bank(fake):
    tr, wa = fake
    live, bank = tr.bank, wa.bank
    # the second bank: the live layout over its own storage, initialised as a copy, without gradient and Adam arenas
    assert bank.index is live.index and bank.n == live.n and bank.grads is None and bank.exp_avg is None
    assert bank.params.data_ptr() != live.params.data_ptr() and torch.equal(bank.params, live.params)
    assert list(bank.buffers) == list(live.buffers)
    assert all(torch.equal(bank.buffers[k], live.buffers[k]) and bank.buffers[k].data_ptr() != live.buffers[k].data_ptr() for k in live.buffers)
    assert bank.p('dec', 'out1.weight').shape == live.p('dec', 'out1.weight').shape
    # params is ONE fp32 range, then every buffer in the bank's order; kinds by dtype
    names = [r[0] for r in wa.ranges]
    assert names == ['avg/params'] + ['avg/buffer/%s/%s' % k for k in live.buffers] and wa.n == len(names) == 1 + len(live.buffers)
    kinds = {'torch.float32': L.AVG_F32, 'torch.int64': L.AVG_COPY}
    assert [r[3] for r in wa.ranges] == [L.AVG_F32] + [kinds[str(t.dtype)] for t in live.buffers.values()]
    assert {str(t.dtype) for t in live.buffers.values()} == set(kinds)
    assert all(r[3] == L.AVG_COPY for r in wa.ranges if r[0].endswith('num_batches_tracked'))
    assert all(r[3] == L.AVG_F32 for r in wa.ranges if r[0].endswith(('running_mean', 'running_var')))
    # the descriptor rows: live pointer, averaged pointer, bytes; the chunk0 column counts the chunks in front
    chunks = 0
    for e, (name, a, b, kind) in zip(wa.arr, wa.ranges):
        nbytes = a.numel() * a.element_size()
        assert (e.src, e.dst, e.bytes, e.kind, e.chunk0) == (a.data_ptr(), b.data_ptr(), nbytes, kind, chunks), name
        chunks += -(-nbytes // L.AVG_CHUNK)
    assert wa.chunks == chunks and wa.arr[1].chunk0 == -(-4 * live.n // L.AVG_CHUNK) > 100
    assert wa.table_dev.numel() == wa.n * ctypes.sizeof(L.RdAvgRange) and bytes(wa.table_dev.numpy()) == bytes(wa.arr)
    assert [n for n, _ in wa.named_ranges()] == names and all(t is r[2] for (_, t), r in zip(wa.named_ranges(), wa.ranges))
    assert wa.settings() == dict(mode='ema', decay=0.5, start=7) and wa.w == F32(0.5)
    assert AV.WeightAverage(tr, 'uniform', 0.3, 0).settings() == dict(mode='uniform', decay=None, start=0)
    assert np.array_equal(wa.model([1.0], [3.0], 9), AV.model([1.0], [3.0], 9, 'ema', 0.5, 7))


def test_weight_average_refuses_bad_settings():
    tr = _fake_trainer()
    with pytest.raises(ValueError, match='mode'):
        AV.WeightAverage(tr, 'swa')
    for decay in (0.0, 1.0, -0.5, 1.5, 1 - 1e-9):                                 # the last one rounds to 1 in float32
        with pytest.raises(ValueError, match='decay'):
            AV.WeightAverage(tr, 'ema', decay)
    with pytest.raises(ValueError, match='start'):
        AV.WeightAverage(tr, 'uniform', start=-1)


def test_state_dicts_are_the_reference_keys_in_manifest_order(golden_dir, fake):
    tr, wa = fake
    with open(os.path.join(golden_dir, 'state_manifest.json')) as f:
        man = json.load(f)
    sds = wa.state_dicts()
    assert list(sds) == ['encoder_state_dict', 'seg_decoder_state_dict', 'rec_decoder_state_dict']
    for (m, key), nm in zip(CK.MODULE_KEYS, ('encoder', 'seg_decoder', 'rec_decoder')):
        sd = sds[key]
        assert [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()] == man[nm], nm
        for k, v in sd.items():
            want = wa.bank.p(m, k) if (m, k) in wa.bank.index else wa.bank.b(m, k)
            assert torch.equal(v, want) and v.data_ptr() != want.data_ptr(), (m, k)


# ------------------------------------------------------------------------------------------------------------- flags
BASE = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']
REFUSALS = [
    (['--avg_weights', 'ema', '--norm', 'gn'], '--norm gn trains through the modules'),
    (['--avg_weights', 'uniform', '--norm', 'in'], '--norm in trains through the modules'),
    (['--avg_weights', 'ema', '--avg_decay', '0'], r'decay in \(0, 1\)'),
    (['--avg_weights', 'ema', '--avg_decay', '1'], r'decay in \(0, 1\)'),
    (['--avg_weights', 'ema', '--avg_decay', '1.5'], r'decay in \(0, 1\)'),
    (['--avg_weights', 'ema', '--avg_decay', '-0.1'], r'decay in \(0, 1\)'),
    (['--avg_weights', 'ema', '--avg_decay', '0.999999999'], r'decay in \(0, 1\)'),
    (['--avg_weights', 'ema', '--avg_start', '-1'], 'iteration number'),
    (['--avg_weights', 'uniform', '--avg_start', '-3'], 'iteration number'),
    (['--avg_decay', '0.9'], 'need --avg_weights'),
    (['--avg_start', '5'], 'need --avg_weights'),
    (['--avg_weights', 'uniform', '--avg_decay', '0.9'], 'decay of --avg_weights ema'),
]


def test_parse_defaults_and_settings():
    T = _train_module()
    a = T.parse_args(['--save_path', 'x'])
    assert (a.avg_weights, a.avg_decay, a.avg_start) == (None, None, None) and not T.uses_avg(a)
    T.check_args(T.parse_args(BASE), 1)
    a = T.parse_args(BASE + ['--avg_weights', 'ema'])
    T.check_args(a, 1)
    T.check_args(a, 8)                                      # rank-local under data parallelism: not refused
    assert T.uses_avg(a) and T.avg_settings(a) == ('ema', 0.999, 0)
    a = T.parse_args(BASE + ['--avg_weights', 'uniform', '--avg_start', '40'])
    T.check_args(a, 1)
    assert T.avg_settings(a) == ('uniform', 0.999, 40)
    a = T.parse_args(BASE + ['--avg_weights', 'ema', '--avg_decay', '0.5', '--avg_start', '0'])
    T.check_args(a, 1)
    assert T.avg_settings(a) == ('ema', 0.5, 0)
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ['--avg_weights', 'swa'])
    assert T.val_log_path(a, '_avg').endswith('3_val_log_avg.csv') and T.val_log_path(a).endswith('3_val_log.csv')


@pytest.mark.parametrize('flags,match', REFUSALS)
def test_check_args_refusals_directly_and_through_main(flags, match, monkeypatch):
    T = _train_module()
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match=match):
        T.check_args(T.parse_args(BASE + flags), 1)
    # main() refuses before it touches the data root (which does not exist), a process group or the GPU
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: pytest.fail('a GPU call was made'))
    with pytest.raises(ValueError, match=match):
        T.main(T.parse_args(BASE + flags))


def test_report_suffix_names_the_averaged_csv(tmp_path, capsys):
    T = _train_module()
    assert T.report_fundus([(0.5, 0.25)], 3, 2, str(tmp_path), 8, suffix='_avg') == T.report_fundus([(0.5, 0.25)], 3, 2, str(tmp_path), 8)
    assert T.report_prostate(0.75, 3, 2, str(tmp_path), 8, '_avg') == T.report_prostate(0.75, 3, 2, str(tmp_path), 8)
    assert sorted(os.listdir(tmp_path)) == ['2_val_log.csv', '2_val_log_avg.csv']
    lines = open(tmp_path / '2_val_log.csv').read().splitlines()
    assert open(tmp_path / '2_val_log_avg.csv').read().splitlines() == lines and len(lines) == 2


def test_keep_best_rotates_the_averaged_checkpoints_on_their_own(tmp_path, fake):
    T = _train_module()
    tr, wa = fake
    out = str(tmp_path)
    assert T.keep_best(out, None, 0.0, None, averaged=wa) == 0.0 and os.listdir(out) == []
    assert T.keep_best(out, 41.5, 0.0, None, averaged=wa) == 41.5
    assert T.keep_best(out, 40.0, 41.5, None, averaged=wa) == 41.5
    assert os.listdir(out) == ['model_avg_41.50.pth']
    assert T.keep_best(out, 43.25, 41.5, None, averaged=wa) == 43.25 and os.listdir(out) == ['model_avg_43.25.pth']
    ck = torch.load(os.path.join(out, 'model_avg_43.25.pth'))
    assert type(ck) is dict and list(ck) == [k for _, k in CK.MODULE_KEYS]
    assert torch.equal(ck['seg_decoder_state_dict']['out1.weight'], wa.bank.p('dec', 'out1.weight'))


# ------------------------------------------------------------------------------------------------------------- the state file
def _avg_meta(wa, **kw):
    return dict(epoch=1, iter_num=41, previous_best=12.5, avg_weights=dict(wa.settings(), previous_best_avg=11.25, val_log_bytes=120, **kw))


def test_averaged_ranges_round_trip_behind_the_trainers(tmp_path, fake):
    tr = fake[0]
    wa = AV.WeightAverage(tr, 'ema', 0.5, 7)                # its own: the shared one stays a copy of the live model
    wa.bank.params.mul_(0.5)                                # an average that is no longer the live model
    state = _fake_state(tr, wa, _avg_meta(wa))
    names = [e['name'] for e in state['table']]
    n = len(CK.trainer_ranges(tr))
    assert names[:n] == [nm for nm, _ in CK.trainer_ranges(tr)] and names[n - 2:n] == ['iter', 'hyper']       # the trainer's set, unmoved
    assert names[n:] == [nm for nm, _ in wa.named_ranges()] and all(nm.startswith(CK.AVG_PREFIX) for nm in names[n:])
    path = str(tmp_path / 'last_state.pth')
    CK.write_file(path, state)
    back = CK.load_file(path)                               # every range's checksums verified, the averaged ones included
    assert back['table'] == state['table'] and back['meta']['avg_weights'] == dict(mode='ema', decay=0.5, start=7, previous_best_avg=11.25,
                                                                                  val_log_bytes=120)
    assert torch.equal(CK.range_tensor(back, 'avg/params'), wa.bank.params) and not torch.equal(CK.range_tensor(back, 'params'), wa.bank.params)
    for (m, key), t in wa.bank.buffers.items():
        got = CK.range_tensor(back, 'avg/buffer/%s/%s' % (m, key))
        assert got.dtype == t.dtype and torch.equal(got, t), (m, key)
    # the live model's state_dicts come out of the file as before
    assert torch.equal(CK.state_dicts(back)['seg_decoder_state_dict']['out1.weight'], tr.bank.p('dec', 'out1.weight'))
    # a flipped byte in an averaged range is named
    e = next(e for e in state['table'] if e['name'] == 'avg/params')
    bad = dict(state, blob=state['blob'].clone())
    bad['blob'][e['offset'] + 40] ^= 0x10
    CK.write_file(path, bad)
    with pytest.raises(ValueError, match='range avg/params is corrupt'):
        CK.load_file(path)
    CK.compare_avg_weights(back, wa.settings())             # the same settings: accepted


def test_resume_refusals_name_avg_weights(fake):
    tr, wa = fake
    plain, with_avg = _fake_state(tr), _fake_state(tr, wa, _avg_meta(wa))
    CK.compare_avg_weights(plain, None)                     # neither side has it: accepted
    with pytest.raises(ValueError, match=r'no averaged model.*avg_weights'):
        CK.compare_avg_weights(plain, wa.settings())        # the flag is on, the file has no averaged ranges
    with pytest.raises(ValueError, match=r'holds an averaged model \(avg_weights.*without --avg_weights'):
        CK.compare_avg_weights(with_avg, None)              # the file has them, the flag is off
    for other, field in ((dict(mode='uniform', decay=None, start=7), 'mode'), (dict(mode='ema', decay=0.9, start=7), 'decay'),
                         (dict(mode='ema', decay=0.5, start=0), 'start')):
        with pytest.raises(ValueError, match='avg_weights %s' % field):
            CK.compare_avg_weights(with_avg, other)
