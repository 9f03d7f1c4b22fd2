"""CPU-only tests of the shared range-table code (ramdsir/range_table.py; csrc/range_walk.h walk_table): the chunk0 column of all
four table types against a table worked out by hand, and the table-validation codes of rd_snapshot, rd_avg_step and rd_guard_sync
driven with made-up pointer values -- every call below comes back before a launch, nothing is dereferenced (as test_cpu_optim.py
relies on for rd_optim_step).  The expected codes are those of the `code(...)` calls of tests/test_gpu_ckpt.py,
test_gpu_avg_weights.py and test_gpu_grad_guard.py; where two things are wrong the earlier one wins: ranges in table order, within a
range the order include/ramdsir.h lists the codes in (-2, -3, -4, then the chunk0 column, -5).  No valid non-empty table is passed.
rd_snapshot with only empty ranges launches its clear, so its empty call here is n == 0 alone."""
import pytest

from ramdsir import _lib as L, avg as AV, ckpt as CK, guard as G, optim as O, range_table as R       # noqa: E402

BASE, DEV, STAGE, SUMS, WORD = 0x7f0000100000, 0x7f0000200000, 0x7f0000400000, 0x7f0000800000, 0x7f0000900000
SIZES = lambda C: [4, 0, C, C + 4, 3 * C + 20]      # noqa: E731 -- 1, 0, 1, 2 and 4 chunks: chunk0 = 0, 1, 1, 2, 4 and 8 in all
TABLES = [
    (L.RdSnapRange, L.SNAP_CHUNK, 65536, 'bytes', lambda s, i: dict(ptr=BASE + 16 * i, bytes=s, offset=64 * i),
     lambda rows: CK.build_table([(r['ptr'], r['bytes'], r['offset']) for r in rows])),
    (L.RdAvgRange, L.AVG_CHUNK, 16384, 'bytes', lambda s, i: dict(src=BASE + 16 * i, dst=DEV + 16 * i, bytes=s, kind=i & 1),
     lambda rows: AV.build_table([(r['src'], r['dst'], r['bytes'], r['kind']) for r in rows])),
    (L.RdGuardRange, L.GUARD_CHUNK, 16384, 'bytes', lambda s, i: dict(live=BASE + 16 * i, shadow=DEV + 16 * i, bytes=s),
     lambda rows: G.build_table([(r['live'], r['shadow'], r['bytes']) for r in rows])),
    (L.RdOptimRange, L.OPT_CHUNK, 4096, 'count', lambda s, i: dict(first=1000 * i, count=s, lr_mult=0.5, weight_decay=0.25 * i),
     lambda rows: O.make_table([(r['first'], r['count'], r['lr_mult'], r['weight_decay']) for r in rows])),
]


@pytest.mark.parametrize('struct,chunk,value,size_field,row,bound', TABLES, ids=[t[0].__name__ for t in TABLES])
def test_build_against_a_table_worked_out_by_hand(struct, chunk, value, size_field, row, bound):
    assert chunk == value
    rows = [row(s, i) for i, s in enumerate(SIZES(chunk))]
    for arr, chunks in (R.build(struct, chunk, rows, size_field), bound(rows)):        # the shared function and the module's binding
        assert isinstance(arr, struct * 5) and chunks == 8
        assert [e.chunk0 for e in arr] == [0, 1, 1, 2, 4]
        for e, r in zip(arr, rows):
            assert all(getattr(e, k) == v for k, v in r.items()), r
    # an empty list still yields a one-entry array, all zero; a negative size counts no chunk (the entry point refuses it)
    for arr, chunks in (R.build(struct, chunk, [], size_field), bound([])):
        assert len(arr) == 1 and chunks == 0 and bytes(arr) == bytes(len(bytes(arr)))
    arr, chunks = R.build(struct, chunk, [row(-4, 0), row(chunk + 1, 1)], size_field)
    assert [e.chunk0 for e in arr] == [0, 0] and chunks == 2


def test_rd_snapshot_table_codes():
    lib, CH = L.lib(), L.SNAP_CHUNK
    good = [(BASE, 64, 0), (BASE + 4096, CH + 8, 64), (BASE + 3 * CH, 16, 2 * CH)]

    def code(entries=good, n=None, total=None, staging_bytes=4 * CH, direction=0, chunk0=None, stage=STAGE, sums_ptr=SUMS, dev=True):
        arr, chunks = CK.build_table(entries)
        for i, v in (chunk0 or {}).items():
            arr[i].chunk0 = v
        n = len(entries) if n is None else n
        return lib.rd_snapshot(arr, DEV if dev else None, n, chunks if total is None else total, stage, staging_bytes, sums_ptr,
                               direction, None)
    assert CK.build_table(good)[1] == 4
    assert code(n=-1) == -1 and code(stage=None) == -1 and code(sums_ptr=None) == -1 and code(dev=False) == -1
    assert code([(BASE, 6, 0)]) == -2 and code([(BASE, -4, 0)]) == -2
    assert code([(BASE + 2, 8, 0)]) == -3 and code([(BASE, 8, 2)]) == -3 and code(stage=STAGE + 2) == -3 and code([(None, 8, 0)]) == -3
    assert code([(BASE, 64, 0), (BASE + 4096, 64, 60)]) == -4                 # overlap
    assert code([(BASE, 64, 64), (BASE + 4096, 64, 0)]) == -4                 # descending
    assert code(staging_bytes=2 * CH + 12) == -4 and code([(BASE, 64, 4 * CH - 60)]) == -4 and code([(BASE, 8 * CH, 0)]) == -4
    assert code(total=3) == -5 and code(total=5) == -5 and code(chunk0={1: 0}) == -5 and code(chunk0={2: 2}) == -5
    # two things wrong: the earlier range wins, and within a range -2, -3, -4, -5 in this order
    assert code([(BASE + 2, 6, 2)], staging_bytes=4, chunk0={0: 1}) == -2
    assert code([(BASE + 2, 8, 0)], staging_bytes=4, chunk0={0: 1}) == -3
    assert code([(BASE, 8, 0)], staging_bytes=4, chunk0={0: 1}) == -4
    assert code([(BASE, 64, 0), (BASE + 64, 6, 64)], chunk0={0: 1}) == -5     # range 0's column in front of range 1's byte count
    assert code([(BASE, 64, 64), (BASE + 2, 64, 0)]) == -3                    # range 1: misaligned in front of descending
    assert code([(BASE, 64, 0), (BASE + 64, 64, 0), (BASE + 128, 6, 128)]) == -4      # range 1's overlap in front of range 2's count
    assert code(total=5, chunk0={2: 2}) == -5 and code(total=5, staging_bytes=2 * CH + 12) == -4
    assert code(n=-1, stage=STAGE + 2) == -1 and code(stage=STAGE + 2, entries=[(BASE, 6, 0)]) == -3      # the arguments in front of the table
    # n == 0 succeeds without a table, a staging buffer or sums
    assert lib.rd_snapshot(None, None, 0, 0, None, 0, None, 0, None) == 0 and lib.rd_snapshot(None, None, 0, 0, None, 0, None, 1, None) == 0


def _edited(struct, base, edit):
    arr = (struct * 3).from_buffer_copy(base)
    for k, (i, v) in edit.items():
        setattr(arr[i], k, v)
    return arr


def test_rd_avg_step_table_codes():
    lib, CH, w = L.lib(), L.AVG_CHUNK, float(AV.one_minus_decay(0.9))
    base, chunks0 = AV.build_table([(BASE, DEV + 4096, CH + 4, L.AVG_F32), (BASE + 2 * CH, DEV + 2 * CH, 0, L.AVG_F32),
                                    (BASE + 3 * CH + 4, DEV + 3 * CH + 8, 64, L.AVG_COPY)])
    assert chunks0 == 3

    def code(table=True, dev=True, n=3, chunks=None, iter_ptr=WORD, mode=0, w=w, start=0, **edit):
        return lib.rd_avg_step(_edited(L.RdAvgRange, base, edit) if table else None, DEV if dev else None, n,
                               chunks0 if chunks is None else chunks, iter_ptr, mode, w, start, None)
    assert code(table=False) == -1 and code(dev=False) == -1 and code(iter_ptr=None) == -1 and code(n=-1) == -1
    assert code(n=0, iter_ptr=None) == -1
    assert code(bytes=(0, -4)) == -2 and code(bytes=(0, CH + 6)) == -2 and code(bytes=(2, 63)) == -2
    assert code(src=(0, BASE + 2)) == -3 and code(dst=(2, DEV + 1)) == -3
    assert code(src=(0, None)) == -3 and code(dst=(2, None)) == -3 and code(iter_ptr=WORD + 2) == -3
    assert code(kind=(0, 2)) == -4 and code(kind=(2, -1)) == -4
    assert code(chunk0=(1, 1)) == -5 and code(chunk0=(0, 1)) == -5 and code(chunks=chunks0 + 1) == -5 and code(chunks=0) == -5
    assert code(bytes=(0, CH)) == -5                        # one chunk fewer than the column says
    # two things wrong: the earlier range wins, and within a range -2, -3, -4, -5 in this order
    assert code(bytes=(0, 6), src=(0, BASE + 2), kind=(0, 2), chunk0=(0, 1)) == -2
    assert code(src=(0, BASE + 2), kind=(0, 2), chunk0=(0, 1)) == -3
    assert code(kind=(0, 2), chunk0=(0, 1)) == -4
    assert code(chunk0=(0, 1), bytes=(1, 6)) == -5 and code(kind=(1, 3), bytes=(2, 6)) == -4 and code(dst=(1, DEV + 2), kind=(2, 2)) == -3
    assert code(chunks=0, kind=(2, 2)) == -4 and code(chunks=0, chunk0=(2, 1)) == -5
    assert code(n=-1, iter_ptr=WORD + 2) == -1 and code(iter_ptr=WORD + 2, bytes=(0, 6)) == -3           # the arguments in front of the table
    # the empty calls succeed and launch nothing
    assert code(n=0) == 0 and code(n=0, table=False, dev=False, chunks=0) == 0
    assert code(n=1, chunks=0, bytes=(0, 0)) == 0           # every range empty


def test_rd_guard_sync_table_codes():
    lib, CH = L.lib(), L.GUARD_CHUNK
    base, chunks0 = G.build_table([(BASE, DEV + 4096, CH + 4), (BASE + 2 * CH, DEV + 2 * CH, 0), (BASE + 3 * CH + 4, DEV + 3 * CH + 8, 64)])
    assert chunks0 == 3 and CH == 16384

    def code(table=True, dev=True, n=3, chunks=None, state=WORD, **edit):
        return lib.rd_guard_sync(_edited(L.RdGuardRange, base, edit) if table else None, DEV if dev else None, n,
                                 chunks0 if chunks is None else chunks, state, None)
    assert code(table=False) == -1 and code(dev=False) == -1 and code(state=None) == -1 and code(n=-1) == -1 and code(n=0, state=None) == -1
    assert code(bytes=(0, -4)) == -2 and code(bytes=(0, 16384 + 6)) == -2 and code(bytes=(2, 63)) == -2
    assert code(live=(0, BASE + 2)) == -3 and code(shadow=(2, DEV + 1)) == -3
    assert code(live=(0, None)) == -3 and code(shadow=(2, None)) == -3 and code(state=WORD + 4) == -3
    assert code(chunk0=(1, 1)) == -5 and code(chunk0=(0, 1)) == -5 and code(chunks=chunks0 + 1) == -5 and code(chunks=0) == -5
    assert code(bytes=(0, 16384)) == -5
    # two things wrong: the earlier range wins, and within a range -2, -3, -5 in this order
    assert code(bytes=(0, 6), live=(0, BASE + 2), chunk0=(0, 1)) == -2 and code(live=(0, BASE + 2), chunk0=(0, 1)) == -3
    assert code(chunk0=(0, 1), bytes=(1, 6)) == -5 and code(shadow=(1, DEV + 2), bytes=(2, 6)) == -3
    assert code(chunks=0, bytes=(2, 6)) == -2 and code(chunks=0, chunk0=(2, 1)) == -5
    assert code(n=-1, state=WORD + 4) == -1 and code(state=WORD + 4, bytes=(0, 6)) == -3                 # the arguments in front of the table
    assert code(n=0) == 0 and code(n=0, table=False, dev=False, chunks=0) == 0 and code(n=1, chunks=0, bytes=(0, 0)) == 0
