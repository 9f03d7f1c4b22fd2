"""CPU-only tests of train.py --weight_decay / --wd_mode / --lr_schedule / --warmup_iters / --enc_lr_mult (ramdsir/optim.py;
rd_optim_step in csrc/optim.hip): the struct layouts against the C compiler, the exported symbol, the range table over a CPU
ParamBank of the real three modules, the numpy model of the prepare launch against values worked out by hand, the decay model,
every validation code of the entry point (they come back before anything is launched, so no GPU is needed), train.py's refusals
and the resume refusals.  No GPU call."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from ramdsir import _lib as L, ckpt as CK, engine as E, optim as O       # noqa: E402
from fake_trainer import fake_state as _fake_state, fake_trainer as _fake_trainer       # noqa: E402
from test_cpu_grad_guard import _round_f32, _train_module       # noqa: E402

F32 = np.float32
OPT_FIELDS = [n for n, _ in L.RdOptim._fields_]
RANGE_FIELDS = [n for n, _ in L.RdOptimRange._fields_]


def _bits(x):
    return int(np.asarray(x, F32).view(np.int32))


# ------------------------------------------------------------------------------------------------------------- descriptors
def test_struct_layouts_match_the_c_compiler(tmp_path):
    offs = ''.join('printf("%%zu ", offsetof(rd_optim_t, %s));' % f for f in OPT_FIELDS) + \
        ''.join('printf("%%zu ", offsetof(rd_optim_range_t, %s));' % f for f in RANGE_FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%%zu %%zu %%d %%d ", sizeof(rd_optim_t), '
           'sizeof(rd_optim_range_t), RD_OPT_CHUNK, RD_OPT_MAX_RANGES);%s return 0;}' % offs)
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    desc, rng, chunk, max_ranges = out[:4]
    assert ctypes.sizeof(L.RdOptim) == desc == 88 and ctypes.sizeof(L.RdOptimRange) == rng == 32
    assert L.OPT_CHUNK == chunk == O.CHUNK and L.OPT_MAX_RANGES == max_ranges == 4096
    assert [getattr(L.RdOptim, f).offset for f in OPT_FIELDS] == out[4:4 + len(OPT_FIELDS)]
    assert [getattr(L.RdOptimRange, f).offset for f in RANGE_FIELDS] == out[4 + len(OPT_FIELDS):] == [0, 8, 16, 20, 24]
    # what rd_adam_t carries, without n_half_lr, and the three new fields behind it
    adam = [n for n, _ in L.RdAdam._fields_ if n not in ('n_half_lr', 'pad_')]
    assert OPT_FIELDS == adam + ['schedule', 'warmup_iters', 'wd_mode']
    assert (L.OPT_POLY, L.OPT_COSINE, L.OPT_CONSTANT, L.OPT_DECOUPLED, L.OPT_L2) == (0, 1, 2, 0, 1)


def test_the_symbol_is_exported():
    assert 'rd_optim_step' in L.exported_symbols()
    assert L.lib().rd_optim_step is not None                   # resolves in the built library
    for name in ('rd_adam_step', 'rd_adam_step_guarded'):      # untouched beside it
        assert getattr(L.lib(), name) is not None


# ------------------------------------------------------------------------------------------------------------- the table
@pytest.fixture(scope='module')
def bank():
    mods = [('enc', E.encoder_specs()), ('dec', E.decoder_specs()), ('rec', E.rec_decoder_specs(16, 3, 3))]
    return E.ParamBank(mods, 'cpu')


def test_make_table_chunk_column():
    Cn = O.CHUNK
    arr, chunks = O.make_table([(0, 1, 0.5, 0.0), (1, Cn, 1.0, 0.01), (1 + Cn, Cn + 1, 1.0, 0.0), (2 + 2 * Cn, 3 * Cn - 1, 0.25, 0.5)])
    assert [e.chunk0 for e in arr] == [0, 1, 2, 4] and chunks == 7
    assert [(e.first, e.count, e.lr_mult, e.weight_decay) for e in arr][3] == (2 + 2 * Cn, 3 * Cn - 1, 0.25, 0.5)


def test_build_table_over_a_cpu_bank_of_the_real_modules(bank):
    W, M = 0.01, 0.25
    entries = O.bank_entries(bank, M, W)
    arr, chunks = O.build_table(bank, M, W)
    assert len(arr) == len(entries) > 20 and len(entries) <= L.OPT_MAX_RANGES
    assert [(e.first, e.count) for e in arr] == [(f, c) for f, c, _, _ in entries]
    # covers [0, n) without gap or overlap
    nxt = 0
    for first, count, _, _ in entries:
        assert first == nxt and count >= 1
        nxt += count
    assert nxt == bank.n
    # the chunk0 column is the running sum of ceil(count / RD_OPT_CHUNK)
    run = 0
    for e in arr:
        assert e.chunk0 == run
        run += -(-e.count // L.OPT_CHUNK)
    assert chunks == run
    # per element: the settings of the range that holds it
    mult, decay = np.zeros(bank.n, F32), np.zeros(bank.n, F32)
    for first, count, m, d in entries:
        mult[first:first + count], decay[first:first + count] = m, d
    enc_end = bank.module_range['enc'][1]
    assert bank.module_range['enc'][0] == 0 and (mult[:enc_end] == F32(M)).all() and (mult[enc_end:] == 1).all()
    assert any(f == enc_end for f, _, _, _ in entries)          # the encoder boundary is a range boundary
    n1 = nd = 0
    for (m, key), (off, shape) in bank.index.items():
        size = int(np.prod(shape))
        want = F32(W) if len(shape) > 1 else F32(0)
        assert (decay[off:off + size] == want).all(), (m, key, shape)
        n1, nd = n1 + (len(shape) == 1), nd + (len(shape) > 1)
    assert n1 > 0 and nd > 0 and all(key.endswith('weight') for (m, key), (off, shape) in bank.index.items() if len(shape) > 1)
    # neighbours with equal settings are merged: no two adjacent ranges agree in both settings
    assert all(a[2:] != b[2:] for a, b in zip(entries, entries[1:]))


def test_default_settings_merge_to_the_two_ranges_of_the_reference(bank):
    enc_end = bank.module_range['enc'][1]
    assert O.bank_entries(bank, 0.5, 0.0) == [(0, enc_end, 0.5, 0.0), (enc_end, bank.n - enc_end, 1.0, 0.0)]
    arr, chunks = O.build_table(bank)
    assert len(arr) == 2 and chunks == -(-enc_end // L.OPT_CHUNK) + -(-(bank.n - enc_end) // L.OPT_CHUNK)
    assert O.bank_entries(bank, 1.0, 0.0) == [(0, bank.n, 1.0, 0.0)]
    assert O.DEFAULTS == dict(CK.OPTIM_DEFAULTS) == _train_module().OPTIM_DEFAULTS


# ------------------------------------------------------------------------------------------------------------- the models
BASE, TOTAL = 2e-3, 40


def _exact(fr):
    """base_lr (as the float32 the descriptor holds) times a rational factor, rounded once to float32."""
    return _round_f32(Fraction(float(F32(BASE))) * fr)


def _ulps(a, b):
    return abs(_bits(a) - _bits(b))


def test_schedule_model_poly_is_the_existing_expression():
    b = float(F32(BASE))
    assert _bits(O.schedule_model(0, BASE, TOTAL)) == _bits(F32(BASE))
    assert _bits(O.schedule_model(1, BASE, TOTAL)) == _bits(F32(BASE))                  # (1 - 0 / total) ^ 0.9 = 1: the one-iteration lag
    for it in (2, 17, TOTAL - 1):
        assert _bits(O.schedule_model(it, BASE, TOTAL, 'poly')) == _bits(F32(b * (1.0 - (it - 1) / TOTAL) ** 0.9)), it
    last = O.schedule_model(TOTAL - 1, BASE, TOTAL)
    assert _ulps(last, F32(b * (2.0 / TOTAL) ** 0.9)) <= 1 and 0 < last < BASE / 10


def test_schedule_model_cosine_constant_and_warmup():
    b = float(F32(BASE))
    assert _bits(O.schedule_model(0, BASE, TOTAL, 'cosine')) == _bits(F32(BASE))        # cos 0 = 1: no lag
    half = O.schedule_model(TOTAL // 2, BASE, TOTAL, 'cosine')
    assert _ulps(half, _exact(Fraction(1, 2))) <= 1                                      # cos(pi / 2) is 6e-17 in float64
    quarter = O.schedule_model(TOTAL // 4, BASE, TOTAL, 'cosine')
    assert _ulps(quarter, F32(b * 0.5 * (1 + math.sqrt(0.5)))) <= 1
    assert float(O.schedule_model(TOTAL, BASE, TOTAL, 'cosine')) == 0.0                  # cos pi = -1 exactly
    assert float(O.schedule_model(TOTAL + 5, BASE, TOTAL, 'cosine')) == 0.0              # min(it, total)
    vals = [float(O.schedule_model(it, BASE, TOTAL, 'cosine')) for it in range(TOTAL + 1)]
    assert all(x > y for x, y in zip(vals, vals[1:]))
    for it in (0, 1, TOTAL - 1, TOTAL + 3):
        assert _bits(O.schedule_model(it, BASE, TOTAL, 'constant')) == _bits(F32(BASE))
    # warm-up over N = 3 iterations: (it + 1) / N up to 1
    N = 3
    assert _bits(O.schedule_model(0, BASE, TOTAL, 'constant', N)) == _bits(_exact(Fraction(1, 3)))
    assert _bits(O.schedule_model(1, BASE, TOTAL, 'constant', N)) == _bits(_exact(Fraction(2, 3)))
    assert _bits(O.schedule_model(N - 1, BASE, TOTAL, 'constant', N)) == _bits(F32(BASE))
    assert _bits(O.schedule_model(N, BASE, TOTAL, 'constant', N)) == _bits(F32(BASE))
    # with poly: the factor multiplies the lagged rate; behind the warm-up the plain poly value
    assert _bits(O.schedule_model(0, BASE, TOTAL, 'poly', N)) == _bits(_exact(Fraction(1, 3)))
    assert _bits(O.schedule_model(1, BASE, TOTAL, 'poly', N)) == _bits(_exact(Fraction(2, 3)))
    assert _ulps(O.schedule_model(2, BASE, TOTAL, 'poly', N), F32(b * (1 - 1 / TOTAL) ** 0.9)) == 0
    assert _bits(O.schedule_model(9, BASE, TOTAL, 'poly', N)) == _bits(O.schedule_model(9, BASE, TOTAL, 'poly', 0))
    assert _ulps(O.schedule_model(1, BASE, TOTAL, 'cosine', 4), F32(b * 0.5 * (1 + math.cos(math.pi / TOTAL)) * 0.5)) <= 1
    # the numeric codes of the descriptor name the same schedules
    for name, code in O.SCHEDULES.items():
        assert _bits(O.schedule_model(7, BASE, TOTAL, code, 2)) == _bits(O.schedule_model(7, BASE, TOTAL, name, 2))


def test_decay_model_on_rows_worked_out_by_hand():
    p = np.array([1.0, -2.0, 0.75, 0.0, -0.0, 3.0], F32)
    g = np.array([0.5, 0.25, -1.0, 2.0, 0.0, 0.0], F32)
    # decoupled, lr 2^-9, multiplier 0.5, decay 0.5: keep = 1 - 2^-11 exactly; the gradient is not touched
    q, h = O.decay_model(p, g, 2.0 ** -9, 0.5, 0.5, 'decoupled')
    assert q.dtype == h.dtype == F32 and np.array_equal(h, g)
    assert q.tolist() == [1 - 2.0 ** -11, -2 * (1 - 2.0 ** -11), 0.75 * (1 - 2.0 ** -11), 0.0, -0.0, 3 * (1 - 2.0 ** -11)]
    assert np.signbit(q[4])
    # three separately rounded operations: lr_g * D rounds before the subtraction
    lr, D = F32(1e-3), F32(0.01)
    keep = F32(1) - F32(F32(F32(0.5) * lr) * D)
    q, _ = O.decay_model(p, g, lr, 0.5, D, 0)
    assert np.array_equal(q, (p * keep).astype(F32)) and _bits(keep) == _bits(_round_f32(1 - Fraction(float(F32(F32(0.5) * lr) * D))))
    # l2: one fma -- the product is not rounded on its own.  D = p = 1 + 2^-12, g = -1: D p = 1 + 2^-11 + 2^-24 exactly, so the fma
    # gives 2^-11 + 2^-24 (a float32); a product rounded first (the tie goes to 1 + 2^-11) would give 2^-11
    D1 = F32(1 + 2.0 ** -12)
    q, h = O.decay_model(np.array([D1], F32), np.array([-1.0], F32), 1e-3, 1.0, D1, 'l2')
    assert q[0] == D1 and float(h[0]) == 2.0 ** -11 + 2.0 ** -24 != float(F32(D1 * D1) - F32(1))
    q, h = O.decay_model(p, g, 1e-3, 1.0, 0.5, 1)
    assert np.array_equal(q, p) and h.tolist() == [1.0, -0.75, -0.625, 2.0, 0.0, 1.5]
    # decay 0: neither operation
    q, h = O.decay_model(p, g, 1e-3, 1.0, 0.0, 'l2')
    assert np.array_equal(q, p) and np.array_equal(h, g)


# ------------------------------------------------------------------------------------------------------------- validation codes
class HostRig:
    """A descriptor and a table whose pointers are HOST arrays: every call below is refused before a launch, nothing is dereferenced."""

    def __init__(self, n=10000):
        self.keep = [np.zeros(n, F32) for _ in range(4)] + [np.zeros(4, np.int32), np.zeros(4, F32)]
        d = self.desc = L.RdOptim()
        d.param, d.grad, d.exp_avg, d.exp_avg_sq = (a.ctypes.data for a in self.keep[:4])
        d.n, d.iter, d.hyper_out = n, self.keep[4].ctypes.data, self.keep[5].ctypes.data
        d.base_lr, d.total_iters, d.beta1, d.beta2, d.eps = 2e-3, 40, 0.9, 0.999, 1e-8
        self.entries = [(0, 5000, 0.5, 0.0), (5000, 1, 1.0, 0.01), (5001, n - 5001, 1.0, 0.0)]
        self.arr, self.chunks = O.make_table(self.entries)
        self.dev = np.zeros(len(self.arr) * 4, np.int64)         # stands for the device copy: never read on a refusal

    def code(self, table=True, dev=True, n_ranges=3, chunks=None, desc=True, rng=None, **edit):
        d = L.RdOptim.from_buffer_copy(self.desc)
        for k, v in edit.items():
            setattr(d, k, v)
        arr = (L.RdOptimRange * 3).from_buffer_copy(self.arr)
        for i, k, v in rng or ():
            setattr(arr[i], k, v)
        return L.lib().rd_optim_step(ctypes.byref(d) if desc else None, arr if table else None, self.dev.ctypes.data if dev else None,
                                     n_ranges, self.chunks if chunks is None else chunks, None, None)


def test_every_validation_code_comes_back_before_a_launch():
    r = HostRig()
    assert r.chunks == 2 + 1 + 2
    assert r.code(desc=False) == -1 and r.code(table=False) == -1 and r.code(dev=False) == -1
    for f in ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'iter', 'hyper_out'):
        assert r.code(**{f: None}) == -1, f
    assert r.code(n=0) == -1 and r.code(n=-3) == -1 and r.code(n_ranges=0) == -1 and r.code(n_ranges=4097) == -1
    assert r.code(schedule=3) == -4 and r.code(schedule=-1) == -4 and r.code(wd_mode=2) == -4 and r.code(wd_mode=-1) == -4
    assert r.code(warmup_iters=-1) == -4 and r.code(warmup_iters=40) == -4 and r.code(warmup_iters=41) == -4
    assert r.code(total_iters=0) == -4
    assert r.code(rng=[(1, 'count', 0)]) == -2 and r.code(rng=[(1, 'count', -1)]) == -2
    assert r.code(rng=[(1, 'first', 4999)]) == -2 and r.code(rng=[(1, 'first', 5001)]) == -2 and r.code(rng=[(0, 'first', 1)]) == -2
    assert r.code(n=10001) == -2 and r.code(n=9999) == -2 and r.code(n_ranges=2, chunks=3) == -2
    assert r.code(rng=[(2, 'count', 5000)]) == -2
    for bad in (0.0, -0.5, float('nan'), float('inf')):
        assert r.code(rng=[(0, 'lr_mult', bad)]) == -3, bad
    for bad in (-0.01, float('nan'), float('inf')):
        assert r.code(rng=[(2, 'weight_decay', bad)]) == -3, bad
    assert r.code(rng=[(1, 'chunk0', 1)]) == -5 and r.code(rng=[(2, 'chunk0', 2)]) == -5 and r.code(rng=[(0, 'chunk0', 1)]) == -5
    assert r.code(chunks=4) == -5 and r.code(chunks=6) == -5 and r.code(chunks=0) == -5
    assert all(not a.any() for a in r.keep)


# ------------------------------------------------------------------------------------------------------------- flags
BASE_ARGS = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']
REFUSALS = [
    (['--weight_decay', '-0.1'], '--weight_decay takes a decay'),
    (['--weight_decay', 'nan'], '--weight_decay takes a decay'),
    (['--weight_decay', 'inf'], '--weight_decay takes a decay'),
    (['--weight_decay', '1e39'], '--weight_decay takes a decay'),
    (['--wd_mode', 'l2'], '--wd_mode shapes the weight decay: it needs --weight_decay'),
    (['--wd_mode', 'l2', '--weight_decay', '0'], 'it needs --weight_decay'),
    (['--warmup_iters', '-1'], '--warmup_iters takes a number of iterations'),
    (['--enc_lr_mult', '0'], '--enc_lr_mult takes a positive finite multiplier'),
    (['--enc_lr_mult', '-0.5'], '--enc_lr_mult takes a positive finite multiplier'),
    (['--enc_lr_mult', 'nan'], '--enc_lr_mult takes a positive finite multiplier'),
    (['--enc_lr_mult', 'inf'], '--enc_lr_mult takes a positive finite multiplier'),
    (['--enc_lr_mult', '1e-60'], '--enc_lr_mult takes a positive finite multiplier'),
    (['--weight_decay', '0.01', '--norm', 'gn'], '--norm gn trains through the modules'),
    (['--lr_schedule', 'cosine', '--norm', 'in'], '--norm in trains through the modules'),
    (['--warmup_iters', '3', '--norm', 'gn'], '--norm gn trains through the modules'),
    (['--enc_lr_mult', '1', '--norm', 'gn'], '--norm gn trains through the modules'),
]


def test_parse_defaults_uses_optim_and_help(capsys):
    T = _train_module()
    a = T.parse_args(BASE_ARGS)
    assert T.optim_settings(a) == T.OPTIM_DEFAULTS == O.DEFAULTS and not T.uses_optim(a)
    spelled = T.parse_args(BASE_ARGS + ['--weight_decay', '0', '--wd_mode', 'decoupled', '--lr_schedule', 'poly', '--warmup_iters', '0',
                                        '--enc_lr_mult', '0.5'])
    T.check_args(spelled, 1)
    assert not T.uses_optim(spelled)
    T.check_args(T.parse_args(BASE_ARGS + ['--norm', 'gn']), 1)             # the defaults do not touch the module trainer
    for flags in (['--weight_decay', '0.01'], ['--weight_decay', '0.01', '--wd_mode', 'l2'], ['--lr_schedule', 'cosine'],
                  ['--lr_schedule', 'constant'], ['--warmup_iters', '3'], ['--enc_lr_mult', '1']):
        a = T.parse_args(BASE_ARGS + flags)
        T.check_args(a, 1)
        T.check_args(a, 8)                                                  # not refused under data parallelism
        assert T.uses_optim(a), flags
    a = T.parse_args(BASE_ARGS + ['--weight_decay', '0.01', '--wd_mode', 'l2', '--lr_schedule', 'cosine', '--warmup_iters', '3',
                                  '--enc_lr_mult', '0.25', '--clip_grad_norm', '1', '--avg_weights', 'uniform', '--ckpt_every', '1'])
    T.check_args(a, 1)
    assert T.optim_settings(a) == dict(weight_decay=0.01, wd_mode='l2', lr_schedule='cosine', warmup_iters=3, enc_lr_mult=0.25)
    with pytest.raises(SystemExit):
        T.parse_args(BASE_ARGS + ['--lr_schedule', 'cyclic'])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    for flag in ('--weight_decay W', '--wd_mode {decoupled,l2}', '--lr_schedule {poly,cosine,constant}', '--warmup_iters N', '--enc_lr_mult M'):
        assert flag in text, flag
    assert 'tensors with more than one dimension' in text and 'BatchNorm weight and bias) are exempt' in text     # the decay rule


@pytest.mark.parametrize('flags,match', REFUSALS)
def test_check_args_refusals_directly_and_through_main(flags, match, monkeypatch):
    T = _train_module()
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match=match):
        T.check_args(T.parse_args(BASE_ARGS + flags), 1)
    # main() refuses before it touches the data root (which does not exist), a process group or the GPU
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: pytest.fail('a GPU call was made'))
    with pytest.raises(ValueError, match=match):
        T.main(T.parse_args(BASE_ARGS + flags))


def test_warmup_is_refused_where_the_length_of_the_run_is_known():
    T = _train_module()
    a = T.parse_args(BASE_ARGS + ['--warmup_iters', '40'])
    T.check_args(a, 1)                                          # not known yet
    T.check_warmup(a, 41)
    for total in (40, 39, 1):
        with pytest.raises(ValueError, match=r'--warmup_iters 40 is not below the %d iterations' % total):
            T.check_warmup(a, total)
    # enable_optim refuses in front of the trainer: nothing is constructed
    trainer = type('T', (), dict(enable_optim=lambda self, **k: pytest.fail('constructed')))()
    with pytest.raises(ValueError, match='--warmup_iters 40'):
        T.enable_optim(a, trainer, 40)
    with pytest.raises(ValueError, match='warmup_iters 5 is not below the 5 iterations'):
        O.check_settings(0.0, 'decoupled', 'poly', 5, 0.5, total_iters=5)
    for bad in (dict(weight_decay=-1.0), dict(weight_decay=float('nan')), dict(wd_mode='adamw'), dict(lr_schedule='step'),
                dict(warmup_iters=-2), dict(enc_lr_mult=0.0), dict(enc_lr_mult=float('inf'))):
        with pytest.raises(ValueError, match='optim: %s' % next(iter(bad))):
            O.check_settings(**dict(O.DEFAULTS, **bad))
    O.check_settings(**O.DEFAULTS)


# ------------------------------------------------------------------------------------------------------------- the state file
WD = dict(weight_decay=0.01, wd_mode='decoupled', lr_schedule='cosine', warmup_iters=0, enc_lr_mult=0.5)


def test_resume_refusals_name_the_optim_field(tmp_path):
    tr = _fake_trainer()
    plain = _fake_state(tr)
    with_optim = _fake_state(tr, None, dict(epoch=1, iter_num=41, previous_best=12.5, optim=dict(WD)))
    # the record adds no range: the table of a file with it is the table of one without
    assert [e['name'] for e in with_optim['table']] == [e['name'] for e in plain['table']] and 'optim' not in plain['meta']
    path = str(tmp_path / 'last_state.pth')
    CK.write_file(path, with_optim)
    back = CK.load_file(path)
    assert back['meta']['optim'] == WD
    CK.compare_optim(back, dict(WD))                            # the same settings: accepted
    CK.compare_optim(plain, None)                               # neither side has a record: accepted
    CK.compare_optim(plain, dict(O.DEFAULTS))                   # a record-less file under the default options spelled out
    with pytest.raises(ValueError, match=r'optim weight_decay = 0.01, this run has 0.02'):
        CK.compare_optim(back, dict(WD, weight_decay=0.02))     # a changed --weight_decay
    with pytest.raises(ValueError, match=r"optim lr_schedule = 'cosine', this run has 'constant'"):
        CK.compare_optim(back, dict(WD, lr_schedule='constant'))            # a changed schedule
    with pytest.raises(ValueError, match=r'optim weight_decay = 0.0, this run has 0.01'):
        CK.compare_optim(plain, dict(WD))                       # a record-less file under non-default flags
    with pytest.raises(ValueError, match=r'optim weight_decay = 0.01, this run has 0.0'):
        CK.compare_optim(back, None)                            # the file has a record, the run has the defaults
    for k, v in (('wd_mode', 'l2'), ('warmup_iters', 3), ('enc_lr_mult', 1.0)):
        with pytest.raises(ValueError, match='optim %s' % k):
            CK.compare_optim(back, dict(WD, **{k: v}))
