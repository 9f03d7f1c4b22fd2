"""-m gpu: the bits of the fixed-order sum of squares (csrc/sumsq_pass.h) as rd_grad_guard and rd_step_log's health pass leave them,
pinned to digests in tests/golden/sumsq_bits.json.

The two entry points run the same pass: over one group that starts at the arena's first element they cut the same chunks, so (a)
their workspaces hold the same records and (b) the row's first norm is the state word's, bit for bit, non-finite counts included.
(c) The sha256 of each workspace's exact rd_*_workspace(n) bytes (prefilled with a sentinel: the step log writes ceil(n / 4096) of
its n / 4096 + 3 records), of row words 28..31 and of the state word's norm / nonfinite equals the committed digest.  The summation
order is fixed by the indices and the library is built without fused or reassociated arithmetic the source does not write, so these
bits are a function of the source, not of the device: an edit that moves one addition shows up here.

Only entry points of the library are used.  Regenerate after an INTENDED change of the order, on the commit whose bits are wanted:
    RD_REGEN_SUMSQ=1 python -m pytest tests/test_gpu_sumsq_bits.py -m gpu      (rewrites tests/golden/sumsq_bits.json in place;
    RD_REGEN_SUMSQ=<path> writes that file instead, to be copied there)"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'sumsq_bits.json')
DEV = 'cuda:0'

from ramdsir import _lib as L, guard as G, step_log as SL       # noqa: E402

F32 = np.float32
CHUNK, SENT = L.LOG_CHUNK, 0xA5
SIZES = [1, 3, 4095, 4096, 4097, 64 * 4096 + 5, 600 * 4096 + 1]     # test_gpu_grad_guard.py's; the last takes the fold's second trip
GROUPS = (4097, 1, 8191)        # the second and third group start off a 16-byte boundary and off a chunk boundary


def _data(n, seed):
    """Random normal float32 at a random scale, with a NaN and an infinity planted where there is room."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n) * 10.0 ** rng.uniform(-3, 2)).astype(F32)
    if n > 3:
        x[n // 3], x[n - 2] = np.nan, -np.inf
    return x


def _view(x, align):
    """x on the device, its first element `align` words behind a 16-byte boundary."""
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    grad = buf[align:align + x.size]
    grad.copy_(torch.from_numpy(x))
    return grad


def _guard(grad):
    """One rd_grad_guard call over `grad` -> (the workspace's bytes, the state word as a dict, norm and nonfinite as bytes)."""
    n = grad.numel()
    ws = torch.full((L.lib().rd_grad_guard_workspace(n),), SENT, dtype=torch.uint8, device=DEV)
    state = torch.zeros(G.STATE_BYTES // 8, dtype=torch.int64, device=DEV)
    d = L.RdGradGuard()
    d.grad, d.n, d.max_norm, d.workspace, d.state = grad.data_ptr(), n, 0.0, ws.data_ptr(), state.data_ptr()
    assert G.run_guard(d) == 0
    torch.cuda.synchronize()
    raw = state.cpu().numpy().tobytes()
    return ws.cpu().numpy().tobytes(), G.state_dict_of(raw), raw[0:4] + raw[12:16]


def _step_log(grad, ranges):
    """One rd_step_log call with the health pass -> (the workspace's bytes, row words 28..31)."""
    dev = lambda k: torch.zeros(k, dtype=torch.float32, device=DEV)       # noqa: E731
    log = SL.StepLog(dev(8), dev(3), dev(4), grad, ranges, rows=1)
    assert log.partial.numel() * 8 == L.lib().rd_step_log_workspace(ranges[3] - ranges[0])
    log.partial.view(torch.uint8).fill_(SENT)
    log._launch(0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return log.partial.view(torch.uint8).cpu().numpy().tobytes(), log.ring[0, 28:32].cpu().numpy()


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def _bits(x):
    return int(np.asarray(x, F32).view(np.int32))


def _against_the_golden(entries):
    regen = os.environ.get('RD_REGEN_SUMSQ')
    if regen:
        out = GOLDEN if regen == '1' else os.path.abspath(regen)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        got = json.load(open(out)) if os.path.exists(out) else {}
        got.update(entries)
        json.dump(got, open(out, 'w'), indent=1, sort_keys=True)
        return
    ref = json.load(open(GOLDEN))
    for key, digest in entries.items():
        assert ref[key] == digest, '%s: other bits than the committed digest' % key


@pytest.mark.parametrize('n', SIZES)
def test_guard_and_health_pass_leave_the_same_pinned_bits(n):
    x = _data(n, n % 1000)
    chunks, entries = -(-n // CHUNK), {}
    for align in range(4):
        grad = _view(x, align)
        g_ws, word, g_raw = _guard(grad)
        l_ws, row = _step_log(grad, [0, n, n, n])
        assert len(g_ws) == 16 * chunks and len(l_ws) == 16 * (n // CHUNK + 3)
        assert g_ws == l_ws[:16 * chunks], (n, align, 'the records of the two first launches differ')
        assert l_ws[16 * chunks:] == bytes([SENT]) * (len(l_ws) - 16 * chunks)
        assert _bits(row[0]) == _bits(word['norm']) and row[3] == word['nonfinite'] == (2 if n > 3 else 0), (n, align, row, word)
        assert _bits(row[1]) == _bits(row[2]) == 0 and np.isfinite(row[0])
        entries.update({'%d/%d/guard_workspace' % (n, align): _sha(g_ws), '%d/%d/log_workspace' % (n, align): _sha(l_ws),
                        '%d/%d/row' % (n, align): _sha(row.tobytes()), '%d/%d/state' % (n, align): _sha(g_raw)})
    _against_the_golden(entries)


def test_three_groups_off_every_boundary():
    """Lengths (4097, 1, 8191): chunks are counted from the start of their group, so each group's norm is the guard's over that slice
    at that slice's alignment."""
    n = sum(GROUPS)
    x = _data(n, 77)
    ranges = [0, GROUPS[0], GROUPS[0] + GROUPS[1], n]
    entries = {}
    for align in range(4):
        grad = _view(x, align)
        l_ws, row = _step_log(grad, ranges)
        bad = 0
        for k in range(3):
            _, word, _ = _guard(grad[ranges[k]:ranges[k + 1]])
            assert _bits(row[k]) == _bits(word['norm']), (align, k, row, word)
            bad += word['nonfinite']
        assert row[3] == bad == 2
        entries.update({'groups/%d/log_workspace' % align: _sha(l_ws), 'groups/%d/row' % align: _sha(row.tobytes())})
    _against_the_golden(entries)
