"""CPU-only tests of train.py --clip_grad_norm / --skip_nonfinite (ramdsir/guard.py; rd_grad_guard, rd_adam_step_guarded,
rd_guard_sync): the struct layouts, the numpy model of the two guard launches against rows worked out in exact rational arithmetic,
the shadow range table over a CPU ParamBank, train.py's refusals, the resume refusals and the guard's range in a training-state file.
No GPU call."""
import ctypes
import importlib.util
import math
import os
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from ramdsir import _lib as L, ckpt as CK, guard as G       # noqa: E402
from fake_trainer import fake_state as _fake_state, fake_trainer as _fake_trainer       # noqa: E402

F32 = np.float32


def _train_module():
    spec = importlib.util.spec_from_file_location('rd_train_guard', os.path.join(ROOT, 'ram-dsir_amd', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bits(a):
    return np.asarray(a, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------- descriptors
def test_struct_sizes_match_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include "ramdsir.h"\nint main(){printf("%zu %zu %zu %d %d\\n", sizeof(rd_guard_state_t), '
           'sizeof(rd_guard_range_t), sizeof(rd_grad_guard_t), RD_GUARD_CHUNK, RD_LOG_CHUNK);return 0;}')
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    state, rng, desc, chunk, log_chunk = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert ctypes.sizeof(L.RdGuardState) == state == 40 == G.STATE_BYTES
    assert ctypes.sizeof(L.RdGuardRange) == rng == 32
    assert ctypes.sizeof(L.RdGradGuard) == desc == 40
    assert L.GUARD_CHUNK == chunk and G.CHUNK == log_chunk == L.LOG_CHUNK
    assert [(n, getattr(L.RdGuardState, n).offset) for n in G.STATE_FIELDS] == [
        ('norm', 0), ('scale', 4), ('skip', 8), ('nonfinite', 12), ('steps', 16), ('clipped', 24), ('skipped', 32)]
    for name in ('rd_grad_guard', 'rd_adam_step_guarded', 'rd_guard_sync', 'rd_grad_guard_workspace'):
        assert name in L.exported_symbols()
    assert G.workspace_bytes(1) == 16 and G.workspace_bytes(4096) == 16 and G.workspace_bytes(4097) == 32 and G.workspace_bytes(0) == 0


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
    return F32(sign * float(n * ulp))


def _fr(v):
    return Fraction(float(v))


def _scale_by_hand(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) as two separately rounded float32 operations, in exact rational arithmetic."""
    d = _round_f32(_fr(F32(norm)) + _fr(F32(1e-6)))
    return min(_round_f32(_fr(F32(max_norm)) / _fr(d)), F32(1))


def test_model_zero_gradient():
    for n in (1, 5, 4096, 4097):
        for max_norm in (0.0, 1.0):
            m = G.model(np.zeros(n, F32), max_norm)
            assert m == dict(norm=0.0, scale=1.0, skip=0, nonfinite=0, steps=1, clipped=0, skipped=0), (n, max_norm)


def test_model_norm_at_and_above_max_norm():
    # 3, 4 -> 5 exactly.  norm == max_norm: the divisor is 5 + 1e-6 rounded (5 plus two ulps), so the scale is just below 1 -- torch's
    # clip_grad_norm_ formula clips there too -- and the step counts as clipped
    at = _scale_by_hand(5, 5)
    assert at < 1 and int(_bits(at)) == int(_bits(F32(1))) - 3      # 5 / (5 + 2 ulp(5)) = 1 - 3.2 ulp(1/2) rounds three floats below 1
    m = G.model(np.array([3, 0, -4], F32), 5.0)
    assert (m['norm'], m['skip'], m['clipped']) == (5.0, 0, 1) and int(_bits(m['scale'])) == int(_bits(at))
    # max_norm one float below the norm
    below = np.nextafter(F32(5), F32(0))
    m = G.model(np.array([3, 0, -4], F32), below)
    assert m['clipped'] == 1 and int(_bits(m['scale'])) == int(_bits(_scale_by_hand(5, below))) and m['scale'] < float(at)
    # 5, 12 -> 13 against max_norm 5, and against a max_norm far above: exactly 1, not clipped
    m = G.model(np.array([5, 12], F32), 5.0)
    assert m['norm'] == 13.0 and int(_bits(m['scale'])) == int(_bits(_scale_by_hand(13, 5))) and 0.38 < m['scale'] < 0.39 and m['clipped'] == 1
    m = G.model(np.array([5, 12], F32), 1e30)
    assert (m['scale'], m['clipped'], m['skip']) == (1.0, 0, 0)
    # max_norm 0 switches clipping off
    m = G.model(np.array([5, 12], F32), 0.0)
    assert (m['norm'], m['scale'], m['clipped'], m['skip']) == (13.0, 1.0, 0, 0)


def test_model_nonfinite_rows():
    for bad in (np.nan, np.inf, -np.inf):
        m = G.model(np.array([3, bad, 4], F32), 1.0)
        # the norm is that of the finite elements; a skipped step is not scaled and not counted as clipped
        assert m == dict(norm=5.0, scale=1.0, skip=1, nonfinite=1, steps=1, clipped=0, skipped=1), bad
    m = G.model(np.array([np.nan, np.inf, 1, -np.inf], F32), 0.0)
    assert (m['nonfinite'], m['skip'], m['norm']) == (3, 1, 1.0)


def test_model_squares_that_overflow_float_but_not_double():
    x = F32(1e30)                                               # x * x = 1e60 is infinite as a float, exact as a double
    m = G.model(np.array([x, -x, x, x], F32), 1.0)              # sqrt(4 x^2) = 2 x exactly
    assert m['norm'] == float(F32(2) * x) and m['skip'] == 0 and m['nonfinite'] == 0
    assert int(_bits(m['scale'])) == int(_bits(_scale_by_hand(F32(2) * x, 1.0))) and 0 < m['scale'] < 1e-29 and m['clipped'] == 1
    # every element finite, the norm 2 y above the largest float: not finite as a float -> skipped
    y = F32(3e38)
    m = G.model(np.array([y, y, -y, y], F32), 1.0)
    assert m['norm'] == math.inf and m == dict(norm=math.inf, scale=1.0, skip=1, nonfinite=0, steps=1, clipped=0, skipped=1)


def test_model_counters_over_a_sequence():
    rows = [(np.zeros(3, F32), 0, 0), (np.array([3, 4], F32), 1, 0), (np.array([np.nan, 1], F32), 0, 1), (np.array([1, 0], F32), 0, 0),
            (np.array([np.inf], F32), 0, 1), (np.array([5, 12], F32), 1, 0)]
    state, clipped, skipped = None, 0, 0
    for k, (g, c, s) in enumerate(rows):
        state = G.model(g, 2.0, state)
        clipped, skipped = clipped + c, skipped + s
        assert (state['steps'], state['clipped'], state['skipped'], state['skip']) == (k + 1, clipped, skipped, s), k
    assert (clipped, skipped) == (2, 2)
    assert G.state_dict_of(bytes(L.RdGuardState(1.5, 0.25, 1, 7, 10, 3, 2))) == dict(norm=1.5, scale=0.25, skip=1, nonfinite=7, steps=10,
                                                                                   clipped=3, skipped=2)


def test_model_over_chunks_and_alignments():
    """Integer data: every partial sum is exact, so the model's summation order cannot show -- the totals must be the exact ones for
    every alignment of the arena, every chunk count and a ragged last chunk."""
    for n in (16384, 4096 * 65, 4097, 3):
        g = np.ones(n, F32)
        for a in range(4):
            sums, counts = G.partial_sums(g, a)
            assert sums.tolist() == [float(min(4096, n - c * 4096)) for c in range(-(-n // 4096))] and not counts.any()
            m = G.model(g, 0.0, align_words=a)
            assert m['norm'] == float(F32(math.sqrt(n))) and (n != 16384 or m['norm'] == 128.0)
    g = np.arange(1, 4096 * 2 + 6, dtype=np.float32)            # squares up to 6.7e7, sums below 2^53: exact in fp64
    g[[0, 4095, 4096, 8196]] = [np.nan, np.inf, -np.inf, np.nan]
    for a in range(4):
        sums, counts = G.partial_sums(g, a)
        k = np.arange(1, 4096 * 2 + 6, dtype=np.int64)
        k[[0, 4095, 4096, 8196]] = 0
        assert sums.tolist() == [float((k[:4096] ** 2).sum()), float((k[4096:8192] ** 2).sum()), float((k[8192:] ** 2).sum())]
        assert counts.tolist() == [2, 1, 1]


# ------------------------------------------------------------------------------------------------------------- the table
@pytest.fixture(scope='module')
def fake():
    tr = _fake_trainer()
    return tr, G.GradGuard(tr, 2.5)


def test_build_table_chunk_column():
    C = L.GUARD_CHUNK
    arr, chunks = G.build_table([(4096, 8192, 4), (0, 0, 0), (16, 32, C), (48, 64, C + 4), (80, 96, 3 * C + 20)])
    assert [e.chunk0 for e in arr] == [0, 1, 1, 2, 4] and chunks == 8
    assert [(e.live, e.shadow, e.bytes) for e in arr][3] == (48, 64, C + 4)
    assert G.build_table([])[1] == 0


def test_shadow_table_over_a_cpu_bank(fake):
    tr, gd = fake
    live = tr.bank
    # every BatchNorm buffer once, in the bank's order, the int64 counters among them; each shadow a copy in its own storage
    assert [r[0] for r in gd.ranges] == ['guard/shadow/%s/%s' % k for k in live.buffers] and gd.n == len(live.buffers) > 30
    assert len({r[1].data_ptr() for r in gd.ranges}) == gd.n == len({r[2].data_ptr() for r in gd.ranges})
    dtypes = {str(r[1].dtype) for r in gd.ranges}
    assert dtypes == {'torch.float32', 'torch.int64'}
    tracked = [r for r in gd.ranges if r[0].endswith('num_batches_tracked')]
    assert tracked and all(r[1].dtype == torch.int64 and r[1].numel() * r[1].element_size() == 8 for r in tracked)
    assert {m for (m, _) in live.buffers} == {'enc', 'dec', 'rec'}
    for suffix in ('running_mean', 'running_var', 'num_batches_tracked'):
        assert sum(r[0].endswith(suffix) for r in gd.ranges) * 3 == gd.n
    chunks = 0
    for e, (name, a, b) in zip(gd.arr, gd.ranges):
        nbytes = a.numel() * a.element_size()
        assert a is live.buffers[tuple(name.split('/')[2:])] and b is not a and torch.equal(a, b) and a.dtype == b.dtype
        assert (e.live, e.shadow, e.bytes, e.chunk0) == (a.data_ptr(), b.data_ptr(), nbytes, chunks), name
        chunks += -(-nbytes // L.GUARD_CHUNK)
    assert gd.chunks == chunks
    assert gd.table_dev.numel() == gd.n * ctypes.sizeof(L.RdGuardRange) and bytes(gd.table_dev.numpy()) == bytes(gd.arr)
    # the descriptor of rd_grad_guard: the whole gradient arena, the state word, a workspace of the library's size
    d = gd.desc
    assert (d.grad, d.n, d.max_norm, d.state, d.workspace) == (live.grads.data_ptr(), live.n, 2.5, gd.state.data_ptr(), gd.workspace.data_ptr())
    assert gd.state.numel() * 8 == 40 and not gd.state.any() and gd.workspace.numel() * 8 == G.workspace_bytes(live.n)
    assert gd.settings() == dict(max_norm=2.5) and gd.read() == dict.fromkeys(G.STATE_FIELDS, 0)
    assert [n for n, _ in gd.named_ranges()] == ['guard/state'] and gd.named_ranges()[0][1] is gd.state
    # sync_shadow: shadow <- live
    k = next(iter(live.buffers))
    keep = live.buffers[k].clone()
    live.buffers[k].add_(1)
    assert not torch.equal(gd.shadows[k], live.buffers[k])
    gd.sync_shadow()
    assert all(torch.equal(gd.shadows[q], t) for q, t in live.buffers.items())
    live.buffers[k].copy_(keep)
    gd.sync_shadow()


def test_grad_guard_refuses_bad_max_norm():
    tr = _fake_trainer()
    for bad in (-1.0, float('nan'), float('inf'), 1e39):
        with pytest.raises(ValueError, match='max_norm'):
            G.GradGuard(tr, bad)
    assert G.GradGuard(tr, 0.0).settings() == dict(max_norm=0.0)


# ------------------------------------------------------------------------------------------------------------- flags
BASE = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']
REFUSALS = [
    (['--clip_grad_norm', '0'], 'positive finite norm'),
    (['--clip_grad_norm', '-1'], 'positive finite norm'),
    (['--clip_grad_norm', 'nan'], 'positive finite norm'),
    (['--clip_grad_norm', 'inf'], 'positive finite norm'),
    (['--clip_grad_norm', '1e39', '--skip_nonfinite'], 'positive finite norm'),
    (['--clip_grad_norm', '1', '--norm', 'gn'], '--norm gn trains through the modules'),
    (['--skip_nonfinite', '--norm', 'in'], '--norm in trains through the modules'),
]


def test_parse_defaults_and_help(capsys):
    T = _train_module()
    a = T.parse_args(['--save_path', 'x'])
    assert (a.clip_grad_norm, a.skip_nonfinite) == (None, False) and not T.uses_guard(a)
    assert not T.uses_guard(T.parse_args(BASE))
    a = T.parse_args(BASE + ['--clip_grad_norm', '2.5'])
    T.check_args(a, 1)
    T.check_args(a, 8)                                      # the same decision on every rank: not refused under data parallelism
    assert T.uses_guard(a) and T.guard_max_norm(a) == 2.5
    a = T.parse_args(BASE + ['--skip_nonfinite'])
    T.check_args(a, 1)
    assert T.uses_guard(a) and T.guard_max_norm(a) == 0.0   # the guard with clipping off
    a = T.parse_args(BASE + ['--skip_nonfinite', '--clip_grad_norm', '1e30', '--ckpt_every', '1', '--avg_weights', 'ema', '--tb_health'])
    T.check_args(a, 1)
    assert T.guard_max_norm(a) == 1e30
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--clip_grad_norm X' in text and '--skip_nonfinite' in text and 'implies --skip_nonfinite' in text
    g = dict(norm=1.5, scale=0.5, skip=0, nonfinite=0, steps=9, clipped=4, skipped=1)
    assert T.guard_pairs(g) == [('guard/grad_norm', 1.5), ('guard/scale', 0.5), ('guard/clipped', 4.0), ('guard/skipped', 1.0)]
    assert T.guard_suffix(g) == ' grad_norm 1.5 scale 0.5 clipped 4 skipped 1'


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


def test_train_log_reports_and_warns(capsys):
    """TrainLog.guard_report: suffix and scalars from the state word; one warning when every step since the last report was skipped."""
    T = _train_module()
    words = iter([dict(norm=0.0, scale=1.0, skip=0, nonfinite=0, steps=0, clipped=0, skipped=0),
                  dict(norm=2.0, scale=0.5, skip=0, nonfinite=0, steps=5, clipped=3, skipped=1),
                  dict(norm=1.0, scale=1.0, skip=1, nonfinite=2, steps=10, clipped=3, skipped=6)])
    log = T.TrainLog.__new__(T.TrainLog)
    log.guard = types.SimpleNamespace(read=lambda: next(words))
    log.guard_mark = log.guard.read()
    suffix, pairs = log.guard_report(4)
    assert suffix == ' grad_norm 2 scale 0.5 clipped 3 skipped 1' and dict(pairs)['guard/skipped'] == 1.0
    assert 'warning' not in capsys.readouterr().out
    suffix, pairs = log.guard_report(9)
    assert dict(pairs) == {'guard/grad_norm': 1.0, 'guard/scale': 1.0, 'guard/clipped': 3.0, 'guard/skipped': 6.0}
    assert 'every one of the 5 steps up to iteration 9 was skipped' in capsys.readouterr().out
    log.guard = None
    assert log.guard_report(10) == ('', [])


# ------------------------------------------------------------------------------------------------------------- the state file
def _guard_meta(gd):
    return dict(epoch=1, iter_num=41, previous_best=12.5, grad_guard=gd.settings())


def test_guard_state_is_in_a_state_built_with_the_guard_only(tmp_path, fake):
    tr = fake[0]
    gd = G.GradGuard(tr, 2.5)
    gd.state.copy_(torch.from_numpy(np.frombuffer(bytes(L.RdGuardState(3.5, 0.75, 0, 0, 41, 7, 2)), np.int64).copy()))
    plain, state = _fake_state(tr), _fake_state(tr, gd, _guard_meta(gd))
    names = [e['name'] for e in state['table']]
    assert names[:-1] == [e['name'] for e in plain['table']] and names[-1] == 'guard/state'       # the trainer's set, unmoved
    assert not any(n.startswith(CK.GUARD_PREFIX) for n in names[:-1]) and 'grad_guard' not in plain['meta']
    assert state['table'][-1]['bytes'] == 40 and state['table'][-1]['dtype'] == 'int64'
    # the ranges in front keep their offsets: a file without the flag is byte for byte what it was
    assert [(e['name'], e['offset'], e['bytes'], e['s1'], e['s2']) for e in state['table'][:-1]] == \
        [(e['name'], e['offset'], e['bytes'], e['s1'], e['s2']) for e in plain['table']]
    path = str(tmp_path / 'last_state.pth')
    CK.write_file(path, state)
    back = CK.load_file(path)
    assert back['meta']['grad_guard'] == dict(max_norm=2.5)
    assert G.state_dict_of(CK.range_tensor(back, 'guard/state').numpy()) == dict(norm=3.5, scale=0.75, skip=0, nonfinite=0, steps=41,
                                                                                   clipped=7, skipped=2)
    CK.compare_grad_guard(back, gd.settings())              # the same settings: accepted


def test_resume_refusals_name_grad_guard(fake):
    tr, gd = fake
    plain, with_guard = _fake_state(tr), _fake_state(tr, gd, _guard_meta(gd))
    CK.compare_grad_guard(plain, None)                      # neither side has it: accepted
    with pytest.raises(ValueError, match=r'holds no guard state.*grad_guard'):
        CK.compare_grad_guard(plain, gd.settings())         # the flag is on, the file has no guard state
    with pytest.raises(ValueError, match=r'holds a guard state \(grad_guard.*without --clip_grad_norm'):
        CK.compare_grad_guard(with_guard, None)             # the file has one, the flags are off
    with pytest.raises(ValueError, match=r'grad_guard max_norm = 2.5, this run has 1.0'):
        CK.compare_grad_guard(with_guard, dict(max_norm=1.0))
    with pytest.raises(ValueError, match='grad_guard max_norm'):
        CK.compare_grad_guard(with_guard, dict(max_norm=0.0))       # --skip_nonfinite alone against a clipped run
