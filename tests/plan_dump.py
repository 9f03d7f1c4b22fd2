"""Canonical dump of the launch plans ramdsir.engine.Plan builds, taken on the CPU (helper of test_cpu_launch_plan.py).

Plan construction launches nothing: ParamBank / WeightPack / Plan / Act and the graph builders work on CPU tensors, the host-side
queries Plan.build calls (rd_conv_honours_src_out, rd_conv_bwd_fused_ok, the workspace sizes, rd_packed_elems) are plain C, and
without a device the library assumes the MI355X's 256 compute units -- so the plan built here is the plan an MI355X gets.

A dump is JSON-serialisable and free of addresses.  Per plan:
  fwd / bwd   the launch lists in order: entry-point name, every argument, the meta dict.  A descriptor passed by reference is written
              field by field (nested rd_src_t / rd_dst_t and the per-group pointer arrays included), a float as float.hex(), a gstart
              array by value, and EVERY pointer as "buffer name+byte offset" (None for null) against a registry of all the memory a
              plan may point into.  A non-null pointer the registry does not know is an error, never skipped.
  tables      fwd_split, bwd_split, bwd_node_start, ws_bytes
  keep        shape and dtype of each tensor, type name of each descriptor, in order: the allocation order, which on the GPU fixes
              the buffers' addresses
It is taken after bind_workspace (descriptors are still edited after they are appended: wg.partial, side_idx, fin_flags).

tests/golden/launch_plan.json holds, per case and plan, one SHA-256 for each of the four parts plus the launch counts by entry point
(so a failure says roughly where to look).  It was generated from the commit BEFORE Plan took its options as an argument and must
never be regenerated from later code: a differing digest means the later code builds another plan.  To see what differs, write the
full dumps of two trees and diff them:

    python tests/plan_dump.py OUT_DIR            # one OUT_DIR/<case>.json per case
"""
import bisect
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'ram-dsir_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                            # noqa: E402

from ramdsir import _lib as L           # noqa: E402
from ramdsir import engine as E         # noqa: E402
from ramdsir import step as S           # noqa: E402
from ramdsir import tuning as T         # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'launch_plan.json')
PARTS = ('fwd', 'bwd', 'keep', 'tables')


# ------------------------------------------------------------------------------------------------ pointer registry
class Registry:
    """Named, non-overlapping byte ranges; sym(address) -> 'name+offset'."""

    def __init__(self):
        self.starts, self.spans = [], []

    def add(self, name, start, nbytes):
        i = bisect.bisect_left(self.starts, start)
        if i < len(self.starts) and self.starts[i] == start:
            return                                   # the same buffer registered twice (a plan's tensor seen through another plan)
        self.starts.insert(i, start)
        self.spans.insert(i, (start, start + max(int(nbytes), 1), name))

    def tensor(self, name, t):
        self.add(name, t.data_ptr(), t.numel() * t.element_size())

    def bank(self, bank, wpack):
        self.tensor('params', bank.params)
        self.tensor('grads', bank.grads)
        for (m, k), t in bank.buffers.items():
            self.tensor('buffer[%s.%s]' % (m, k), t)
        self.tensor('packed', wpack.packed)

    def plan(self, name, plan, workspaces):
        self.tensor(name + '.stat', plan.stat_arena)
        for i, k in enumerate(plan.keep):
            if torch.is_tensor(k):
                self.tensor('%s.keep[%d]' % (name, i), k)
            else:
                self.add('%s.keep[%d]:%s' % (name, i, type(k).__name__), C.addressof(k), C.sizeof(k))
        for key, t in plan._consts.items():
            self.tensor('%s.const[%s,%d]' % (name, float(key[0]).hex(), key[1]), t)
        for i, w in enumerate(workspaces):
            self.tensor('%s.ws[%d]' % (name, i), w)

    def sym(self, addr, where):
        if not addr:
            return None
        i = bisect.bisect_right(self.starts, addr) - 1
        if i >= 0:
            start, end, name = self.spans[i]
            if addr < end:
                return '%s+%d' % (name, addr - start)
        raise AssertionError('%s: pointer 0x%x is in no registered buffer' % (where, addr))


# ------------------------------------------------------------------------------------------------ canonical forms
def _f(v):
    return float(C.c_float(v).value).hex()


def _value(v, t, reg, where):
    if t is C.c_void_p:
        return reg.sym(v, where)
    if t is C.c_float:
        return _f(v)
    if isinstance(t, type) and issubclass(t, C.Structure):
        return _struct(v, reg, where)
    if isinstance(t, type) and issubclass(t, C.Array):
        return [_value(v[i], t._type_, reg, '%s[%d]' % (where, i)) for i in range(t._length_)]
    return int(v)


def _struct(obj, reg, where):
    return {'_type': type(obj).__name__,
            **{name: _value(getattr(obj, name), t, reg, '%s.%s' % (where, name)) for name, t in obj._fields_}}


def _op(op, reg, where):
    fn, args = op[0], op[1]
    types = fn.argtypes[:-1]                            # without the trailing stream
    assert len(types) == len(args), (where, fn.__name__, len(types), len(args))
    out = []
    for i, (v, t) in enumerate(zip(args, types)):
        w = '%s %s arg %d' % (where, fn.__name__, i)
        if hasattr(v, '_obj'):                          # byref(descriptor)
            out.append(_struct(v._obj, reg, w))
        elif isinstance(v, C.Array):                    # gstart
            out.append([int(x) for x in v])
        else:
            out.append(_value(v, t, reg, w))
    return {'fn': fn.__name__, 'args': out, 'meta': dict(op[2]) if len(op) > 2 else None}


def dump_plan(name, plan, reg):
    keep = [['tensor', list(k.shape), str(k.dtype)] if torch.is_tensor(k) else ['desc', type(k).__name__] for k in plan.keep]
    tables = {'fwd_split': dict(getattr(plan, 'fwd_split', {})), 'bwd_split': dict(getattr(plan, 'bwd_split', {})),
              'bwd_node_start': {'%s/%s' % k: v for k, v in getattr(plan, 'bwd_node_start', {}).items()},
              'ws_bytes': int(plan.ws_bytes)}
    return {'fwd': [_op(op, reg, '%s.fwd[%d]' % (name, i)) for i, op in enumerate(plan.fwd)],
            'bwd': [_op(op, reg, '%s.bwd[%d]' % (name, i)) for i, op in enumerate(plan.bwd)],
            'keep': keep, 'tables': tables}


def digest(plan_dump):
    """What the golden keeps of one plan's dump."""
    out = {p: hashlib.sha256(json.dumps(plan_dump[p], sort_keys=True).encode()).hexdigest() for p in PARTS}
    counts = {}
    for lst in ('fwd', 'bwd'):
        c = counts[lst] = {}
        for op in plan_dump[lst]:
            c[op['fn']] = c.get(op['fn'], 0) + 1
    out['launches'] = counts
    return out


# ------------------------------------------------------------------------------------------------ the plans
def step_plans(dtype, batch_sizes, size, options):
    """The training step's two plans, built as TrainStep.__init__ builds them (seg first: the restoration decoder reads feats[4] of the
    seg plan, and which plan owns a folded finalize depends on that order), with the compute-unit budgets pinned (cu_budget needs a
    device)."""
    bs, B, H = list(batch_sizes), sum(batch_sizes), size
    bank, mods = S.make_bank('cpu', 3, 16, 2, len(bs))
    wpack = E.WeightPack(bank, mods, dtype)
    opt = T.options(options)
    seg = E.Plan(bank, dtype, 2 * B, [0, B, 2 * B], options=opt, fused_step=True, pad_narrow=True, side_cus=96, dgrad_cus=160)
    slot = seg.slot_channels()
    x = E.Act(seg, 2 * B, H, H, 3, name='input', cstride=slot if 3 < slot else None)
    feats = E.build_encoder(seg, x, n=16)
    E.build_decoder(seg, feats, n=16, num_classes=2)
    gs = [0]
    for b in bs:
        gs.append(gs[-1] + b)
    rec = E.Plan(bank, dtype, B, gs, options=opt, fused_step=True, pad_narrow=True, side_cus=128, conv_cus=128)
    E.build_rec_decoder(rec, feats[4], n_off=B, g_fixed=1, domains=list(range(len(bs))), n=16, num_classes=3)
    seg.build(wpack)
    rec.build(wpack)
    seg_ws = [E.workspace(max(seg.ws_bytes, 4) // 4 + 1, 'cpu')]
    rec_ws = E.workspace(max(rec.ws_bytes, 4) // 4 + 1, 'cpu')
    seg.bind_workspace(seg_ws)
    rec.bind_workspace(rec_ws)
    reg = Registry()
    reg.bank(bank, wpack)
    reg.plan('seg', seg, seg_ws)
    reg.plan('rec', rec, [rec_ws])
    return {'seg': dump_plan('seg', seg, reg), 'rec': dump_plan('rec', rec, reg)}


def module_plan(mods, dtype, N, gstart, training, graph):
    """A module called on its own (networks.unet._plan_for): the Plan defaults, one workspace."""
    bank = E.ParamBank(mods, 'cpu')
    wpack = E.WeightPack(bank, mods, dtype)
    pl = E.Plan(bank, dtype, N, gstart, slope=0.0, training=training)
    graph(pl)
    pl.build(wpack)
    ws = E.workspace(pl.ws_bytes // 4, 'cpu')
    pl.bind_workspace(ws)
    reg = Registry()
    reg.bank(bank, wpack)
    reg.plan('pl', pl, [ws])
    return {'pl': dump_plan('pl', pl, reg)}


def _raw(pl, N, Cc, H, W, name):
    a = E.Act(pl, N, H, W, Cc, name=name)
    a.needs_grad = True
    return a


def encoder_plan(norm, training):
    N = 3

    def graph(pl):
        pl.x_in = E.Act(pl, N, 32, 32, 3, name='input')
        pl.feats = E.build_encoder(pl, pl.x_in, n=16, mname='enc', norm=norm)
        for a in pl.feats:
            a.g_written = True
    gs = list(range(N + 1)) if norm in ('gn', 'in') else [0, N]
    return module_plan([('enc', E.encoder_specs(3, 16, norm))], torch.float32, N, gs, training, graph)


def convd_plan():
    def graph(pl):
        pl.x_in = _raw(pl, 2, 16, 32, 32, 'input')
        pl.out = E.build_convd(pl, pl.x_in, L.SRC_POOL, 32, '', 'convd', 'bn')
        pl.out.g_written = True
    return module_plan([('convd', E.convd_specs(16, 32))], torch.bfloat16, 2, [0, 2], True, graph)


def convu_plan():
    def graph(pl):
        pl.x_in, pl.prev_in = _raw(pl, 2, 128, 8, 8, 'x'), _raw(pl, 2, 32, 16, 16, 'prev')
        pl.out = E.build_convu(pl, pl.x_in, pl.prev_in, 64, False, '', 'convu', 'bn')
        pl.out.g_written = True
    return module_plan([('convu', E.convu_specs(64, False))], torch.bfloat16, 2, [0, 2], True, graph)


def rec_decoder_plan():
    def graph(pl):
        pl.x_in = _raw(pl, 2, 256, 4, 4, 'bottleneck')
        pl.out = E.build_rec_decoder(pl, pl.x_in, 0, -1, [1], n=16, num_classes=3, mname='rec')
        pl.out.g_written = True
    return module_plan([('rec', E.rec_decoder_specs(16, 3, 3))], torch.bfloat16, 2, [0, 2], True, graph)


# ------------------------------------------------------------------------------------------------ the pinned cases
STEP_OPTIONS = [{}] + [dict(fold_finalize=v) for v in range(6)] + [
    dict(fold_fwd_kinds=1), dict(fused_bwd=False), dict(pool_mat=False), dict(up_mat=False), dict(mat_dz_min_c=64),
    dict(mat_dz_min_c=64, mat_dz_wide=False), dict(mat_min_c=64), dict(mat_min_c=64, up_mat=False), dict(split_wide_dgrad=True),
    dict(fold_finalize=1, fold_wgrad_behind=True)]
# rd_conv_honours_src_out refuses every launch below 256 x 256, where the option then does nothing
STORE_OPTIONS = [{}, dict(store_wgrad_operands=3, store_wgrad_min_c=64), dict(store_wgrad_operands=1, store_wgrad_min_c=64)]


def _tag(options):
    return ','.join('%s=%s' % (k, int(v)) for k, v in options.items()) or 'default'


def cases():
    """name -> function returning {plan name: dump}; the smallest shapes at which each option still changes the plan."""
    out = {}
    for dname, dtype in (('bf16', torch.bfloat16), ('f32', torch.float32)):
        for o in STEP_OPTIONS:
            out['step32.%s.%s' % (dname, _tag(o))] = lambda dtype=dtype, o=o: step_plans(dtype, (1, 2, 1), 32, o)
    for o in STORE_OPTIONS:
        out['step256.bf16.%s' % _tag(o)] = lambda o=o: step_plans(torch.bfloat16, (1, 1, 1), 256, o)
    for norm in ('bn', 'gn', 'in'):
        for training in (True, False):
            out['encoder.%s.%s' % (norm, 'train' if training else 'eval')] = lambda n=norm, t=training: encoder_plan(n, t)
    out['convd.pool'] = convd_plan
    out['convu'] = convu_plan
    out['rec_decoder'] = rec_decoder_plan
    return out


def main(argv):
    if len(argv) != 2:
        sys.exit('usage: plan_dump.py OUT_DIR   (full dumps, one file per case, and OUT_DIR/launch_plan.json in the golden\'s format)')
    for k in [k for k in os.environ if k.startswith('RD_') or k == 'RAMDSIR_DEBUG_LIB']:
        del os.environ[k]
    os.makedirs(argv[1], exist_ok=True)
    golden = {}
    for name, fn in cases().items():
        d = fn()
        with open(os.path.join(argv[1], name + '.json'), 'w') as f:
            json.dump(d, f, indent=1, sort_keys=True)
        golden[name] = {p: digest(v) for p, v in d.items()}
    with open(os.path.join(argv[1], 'launch_plan.json'), 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(golden[k], sort_keys=True)) for k in sorted(golden)) + '\n}\n')


if __name__ == '__main__':
    main(sys.argv)
