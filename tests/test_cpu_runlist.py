"""CPU-only: the launch list's one walk (csrc/runlist.hip) and the Python launch loop over it (engine.Plan.run_lanes), pinned by traces
taken from the code BEFORE the three interpreters of a list became one walk.  Neither golden is ever regenerated from the code under test.

tests/golden/runlist_trace.json is the output of tests/runlist_harness.cpp (its header says what is recorded) linked against the
runlist.hip of the commit before rd_run_list_schedule existed; the harness uses the public ABI only, so in a checkout PARENT of that commit:

    hipcc -O2 -std=c++17 --offload-host-only -c PARENT/ram-dsir_amd/csrc/runlist.hip -o runlist.o
    clang++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/runlist_harness.cpp runlist.o -pthread -o harness
    ./harness > tests/golden/runlist_trace.json          # three runs, byte-identical: the threaded cases are deterministic per stream

tests/golden/run_lanes_trace.json is run_lanes_trace() below on that commit's engine.py (it needs no library there):

    cp tests/test_cpu_runlist.py PARENT/tests/ && python PARENT/tests/test_cpu_runlist.py > tests/golden/run_lanes_trace.json
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'ram-dsir_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cxx = os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++')
    d = tmp_path_factory.mktemp('runlist')
    obj, exe = str(d / 'runlist.o'), str(d / 'harness')
    subprocess.check_call([HIPCC, '-O2', '-std=c++17', '--offload-host-only', '-c',
                           os.path.join(ROOT, 'ram-dsir_amd', 'csrc', 'runlist.hip'), '-o', obj])
    subprocess.check_call([cxx if os.path.exists(cxx) else 'g++', '-O1', '-std=c++17', '-D__HIP_PLATFORM_AMD__', '-I', os.path.join(rocm, 'include'),
                           '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'runlist_harness.cpp'), obj, '-pthread', '-o', exe])
    return exe


def test_walk_traces_equal_the_three_interpreters_they_replace(harness):
    """Every case of the harness -- each op with distinct values in every argument slot, wrong argument counts, unknown ops, the lane
    rules, errors on the main and on a side lane, 0 / 1 / 32 / 33 streams, rd_join_lanes; bind on / off x worker threads on / off x
    capture active / none -- gives, byte for byte, the return code, bad_index, open mask, fork counts and per-stream operations that
    the single-threaded loop, run_list_threaded and the 40-case switch gave."""
    got = subprocess.run([harness], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(GOLDEN, 'runlist_trace.json')) as f:
        want = f.read()
    g, w = json.loads(got), json.loads(want)
    assert sorted(g) == sorted(w) and len(w) == 210
    for k in w:
        assert g[k] == w[k], k
    assert got == want


def test_schedule_is_the_direct_walk_and_fork_plan_is_its_carries(harness):
    """rd_run_list_schedule (the recorder) against the operations the single-threaded walk really issued on the same lists, in issue
    order: step for step the same launches (entry, lane, a fork's event offered), main -> lane and lane -> main edges, open mask, and
    for a malformed list the same error and bad_index.  A list whose entry point fails at run time stops there; the schedule, which
    launches nothing, goes on: the walk's steps are then its prefix.  (The list with a lane on the main stream's handle is not here: a
    schedule speaks of lanes, not of stream handles.)  rd_run_list_fork_plan is the schedule's `carries`, by entry."""
    out = json.loads(subprocess.run([harness, 'schedule'], check=True, capture_output=True, text=True).stdout)
    assert len(out) == 24
    seen = set()
    for name, c in out.items():
        seen.add(c['direct_rc'])
        if c['direct_rc'] in (0, -1):
            assert (c['rc'], c['bad'], c['open'], c['steps']) == (c['direct_rc'], c['direct_bad'], c['direct_open'], c['direct']), name
        else:
            assert c['rc'] == 0 and c['steps'][:len(c['direct'])] == c['direct'] and len(c['steps']) > len(c['direct']), name
        carries = [0] * len(c['plan'])
        for s in c['steps']:
            w = s.split()
            if w[0] == 'launch':
                carries[int(w[1])] = int(w[5])
                assert int(w[5]) == 0 or int(w[3]) == 0, name           # only a main-lane launch carries
        assert c['plan_rc'] == 0 and c['plan'] == carries, name
    assert seen == {0, -1, 77}
    assert out['packing1']['plan'] == [1, 0, 0, 0, 0, 0] and out['packing2']['plan'] == [0, 1, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ Plan.run_lanes
class FakeStream:
    def __init__(self, name, log):
        self.name, self.log, self.cuda_stream = name, log, 'handle:' + name

    def wait_stream(self, other):
        self.log.append('%s waits for %s' % (self.name, other.name))


class FakeFn:
    """Stands for an entry point of the library: its name and argument types, and a call that records instead of launching."""

    def __init__(self, name, log):
        from ramdsir import _lib as L
        self.__name__, self.argtypes, self.log = name, L._SIGS[name][1], log

    def __call__(self, *args):
        self.log.append('%s%r' % (self.__name__, args))
        return 0


def run_lanes_ops(log):
    from ramdsir import engine as E
    f = {n: FakeFn(n, log) for n in ('rd_conv', 'rd_wgrad', 'rd_pool_fwd', 'rd_colsum', 'rd_adam_step', 'rd_bn_finalize_fwd')}
    return [(f['rd_conv'], (11, 1), dict(kernel='a')),
            (f['rd_bn_finalize_fwd'], (12,)),                                           # no meta at all
            E.sync_op('join', 'rec'),                                                   # not open: nothing
            E.sync_op('fork', 'rec'),
            (f['rd_pool_fwd'], (13, None, None, 0.25, 14, 4, 5, 6, 16, 2, 15, 1, None, 0), dict(lane='rec')),
            (f['rd_wgrad'], (16, 1), dict(side=True, side_idx=0)),
            (f['rd_wgrad'], (17, 1), dict(side=True, side_idx=1)),                      # same main position: a second side lane
            (f['rd_conv'], (18, 1), {}),
            (f['rd_wgrad'], (19, 1), dict(side=True, side_idx=2)),                      # beyond the side lanes that exist: side0
            (f['rd_wgrad'], (20, 1), dict(side=True, side_idx=3, lane='rec')),          # rec wins where it exists
            (f['rd_colsum'], (21, 22, 23, 1 << 33, 2, 0, 0.5, 1), dict(side=True)),     # side_idx defaults to 0
            E.sync_op('join', 'side1'),
            E.sync_op('join', 'rec'),
            (f['rd_conv'], (24, 1), dict(lane='rec')),                                  # after the join: the lane is not reopened by a launch
            E.sync_op('fork', 'side1'),
            E.sync_op('join', 'nowhere'),
            (f['rd_adam_step'], (25,))]


RUN_LANES_CASES = {'all_lanes': ('side0', 'side1', 'rec'), 'rec_missing': ('side0', 'side1'), 'no_lanes': (), 'side0_only': ('side0',),
                   'rec_only': ('rec',), 'side1_without_side0': ('side1', 'rec')}


def run_lanes_trace():
    """Per case and for wrap = a recorder / None: what Plan.run_lanes did, in order -- stream waits, wrap(op, stream, launch) calls by op
    index and stream (launch() is not called), or the entry point's call with its arguments and stream handle -- and the lanes it
    returned as open."""
    from ramdsir import engine as E
    out = {}
    for name, lane_names in RUN_LANES_CASES.items():
        for wrapped in (True, False):
            log = []
            ops = run_lanes_ops(log)
            main, lanes = FakeStream('main', log), {n: FakeStream(n, log) for n in lane_names}

            def wrap(op, st, launch):
                assert callable(launch)
                log.append('wrap op %d on %s' % ([i for i, o in enumerate(ops) if o is op][0], st.name))
            opened = E.Plan.run_lanes(ops, main, lanes, wrap if wrapped else None)
            out['%s/%s' % (name, 'wrap' if wrapped else 'plain')] = dict(log=list(log), open=sorted(opened))
            del log[:]                                                                  # the same ops again (a list of its own, as
            assert E.Plan.run_lanes(list(ops), main, lanes, wrap if wrapped else None) == opened      # run_segment(a + b) passes)
            assert log == out['%s/%s' % (name, 'wrap' if wrapped else 'plain')]['log']
    return out


def test_run_lanes_equals_the_python_interpreter_it_replaces():
    """Plan.run_lanes over LaunchList + rd_run_list_schedule does what the hand-written loop did: all lanes present, `rec` missing, no
    lanes, side_idx beyond the lanes that exist (and a side lane without side0, which sends the side ops to the main stream)."""
    with open(os.path.join(GOLDEN, 'run_lanes_trace.json')) as f:
        want = json.load(f)
    got = run_lanes_trace()
    assert sorted(got) == sorted(want) and len(want) == 12
    for k in want:
        assert got[k] == want[k], k


def test_launch_list_keeps_the_index_of_the_op_behind_each_entry():
    from ramdsir import _lib as L, engine as E
    ops = run_lanes_ops([])
    ll = E.LaunchList(ops, ('side0', 'rec'), pack=False)
    assert ll.n == len(ll.op_index) == 14 and ll.op_index == [i for i in range(17) if i not in (11, 14, 15)]
    for e, k in zip(ll.arr[:ll.n], ll.op_index):
        assert (e.op in (L.OP_FORK, L.OP_JOIN)) == (ops[k][0] is None)
        assert ops[k][0] is None or e.op == L.op_code(ops[k][0].__name__)
    steps, mask = ll.schedule()
    assert [k for kind, lane, k in steps if kind == L.STEP_LAUNCH] == [k for k in range(17) if ops[k][0] is not None]
    assert all(k == -1 for kind, lane, k in steps if kind != L.STEP_LAUNCH) and ll.schedule() is ll._schedule
    assert mask == 0b010 and ctypes.sizeof(L.RdStep) == 16


if __name__ == '__main__':
    json.dump(run_lanes_trace(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
