"""CPU-only test of the optimizer tail of the training step (ramdsir/step.py TrainStep.enqueue_tail): which library calls it makes, in
which order, on which stream and under which state word, for every combination of gradient accumulation, the guard and the grouped
Adam -- and that one refusal names every enabled stage in front of a captured graph.  The library is replaced by a recorder: no GPU
call and no launch is made.  The expected sequences are those of the step before it had one tail (four arms in TrainStep.step(), the
guard's own tail, the data-parallel step's three)."""
import types

import pytest

from fake_trainer import fake_trainer
from ramdsir import _lib as L, accum as A, guard as G, optim as O, step as S

STREAM = 1234
# (guard, optim) -> the calls behind the accumulation
TAILS = {
    (False, False): ['rd_adam_step', 'repack'],
    (True, False): ['rd_grad_guard', 'rd_adam_step_guarded', 'repack', 'rd_guard_sync'],
    (False, True): ['rd_optim_step', 'repack'],
    (True, True): ['rd_grad_guard', 'rd_optim_step', 'repack', 'rd_guard_sync'],
}


class Recorder:
    """Stands in for the loaded library: every attribute is a function that records (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def names(self):
        return [name for name, _ in self.calls]

    def args_of(self, name):
        return [args for n, args in self.calls if n == name]


@pytest.fixture(scope='module')
def stages():
    """The fake trainer with one real GradGuard and one real GroupedAdam over it (both construct on the CPU)."""
    tr = fake_trainer()
    return tr, G.GradGuard(tr, 2.5), O.GroupedAdam(tr, weight_decay=0.01)


def _step(tr, rec, guard=None, optim=None, accum=None):
    ts = S.TrainStep.__new__(S.TrainStep)
    ts.bank, ts.ad, ts.graph = tr.bank, tr.ts.ad, None
    ts.wpack = types.SimpleNamespace(refresh=lambda stream: rec.calls.append(('repack', (stream,))))
    ts._guard, ts._optim, ts._accum = guard, optim, accum
    return ts


@pytest.mark.parametrize('with_optim', [False, True], ids=['adam', 'optim'])
@pytest.mark.parametrize('with_guard', [False, True], ids=['open', 'guard'])
@pytest.mark.parametrize('accum', ['off', 'micro0', 'micro1'])
def test_enqueue_tail_calls(stages, monkeypatch, accum, with_guard, with_optim):
    tr, gd, op = stages
    rec = Recorder()
    monkeypatch.setattr(L, 'lib', lambda: rec)
    acc = A.GradAccum(tr, 2) if accum != 'off' else None
    ts = _step(tr, rec, gd if with_guard else None, op if with_optim else None, acc)
    tail = TAILS[(with_guard, with_optim)]
    if accum == 'off':
        assert ts.enqueue_tail(STREAM) is True
        assert rec.names() == tail
    else:
        assert ts.enqueue_tail(stream=STREAM) is False
        assert rec.names() == ['rd_grad_accum']             # the window is open: nothing but the accumulation
        if accum == 'micro1':
            assert ts.enqueue_tail(stream=STREAM) is True
            assert rec.names() == ['rd_grad_accum', 'rd_grad_accum'] + tail
        # rd_grad_accum(grad, acc, n, k, steps, 1 / steps, stream)
        assert [a[3] for a in rec.args_of('rd_grad_accum')] == [0, 1][:len(rec.args_of('rd_grad_accum'))]
        assert all(a[:3] == (tr.bank.grads.data_ptr(), acc.acc.data_ptr(), tr.bank.n) and a[4] == 2 for a in rec.args_of('rd_grad_accum'))
    assert all(args[-1] == STREAM for _, args in rec.calls)
    state = gd.state.data_ptr()
    # rd_optim_step(desc, table, table_dev, ranges, chunks, guard state, stream): None without the guard
    assert [a[-2] for a in rec.args_of('rd_optim_step')] == ([state if with_guard else None] if 'rd_optim_step' in rec.names() else [])
    # rd_adam_step_guarded(ad, guard state, stream); rd_guard_sync(table, table_dev, n, chunks, guard state, stream)
    assert all(a[1] == state for a in rec.args_of('rd_adam_step_guarded'))
    assert all(a[-2] == state and a[2:4] == (gd.n, gd.chunks) for a in rec.args_of('rd_guard_sync'))


def test_one_refusal_names_every_enabled_stage(stages, monkeypatch):
    tr, gd, op = stages
    rec = Recorder()
    monkeypatch.setattr(L, 'lib', lambda: rec)
    ts = _step(tr, rec)
    assert ts._tail_stages() == []
    ts.refuse_fixed_list('capture()')                       # nothing enabled: nothing to refuse
    ts.enable_optim(op)
    ts.enable_grad_accum(A.GradAccum(tr, 2))
    ts.enable_grad_guard(gd)                                # whatever the order of enabling: guard, optim, accum
    assert (ts._guard, ts._optim) == (gd, op) and ts._accum is not None
    named = ts._tail_stages()
    assert len(named) == 3 and ['guarded tail' in named[0], 'grouped Adam' in named[1], 'gradient accumulation' in named[2]] == [True] * 3
    ts.graph = object()                                     # (what capture() leaves)
    with pytest.raises(RuntimeError) as e:
        ts.capture()
    assert all(phrase in str(e.value) for phrase in ('hipGraph', 'guarded tail', 'grouped Adam', 'gradient accumulation'))
    for enable, stage in ((ts.enable_grad_guard, 'guarded tail'), (ts.enable_optim, 'grouped Adam'), (ts.enable_grad_accum, 'gradient accumulation')):
        with pytest.raises(RuntimeError, match='hipGraph') as e:
            enable(object())
        assert stage in str(e.value)
    assert (ts._guard, ts._optim) == (gd, op)               # a refused enable replaces nothing
    assert rec.calls == []
