"""Which kernel rd_conv / rd_wgrad / rd_conv_bwd_fused(_reduce) launch for a descriptor, and with what grid, block, LDS size and integer
arguments: taken on the CPU through the library's routing queries (include/ramdsir.h rd_conv_route, rd_wgrad_route,
rd_conv_bwd_fused_route), which run the same host function the entry points launch from.  Helper of test_cpu_conv_routes.py.

Nothing is launched and no data pointer is dereferenced, so descriptors carry fake addresses; without a device the library assumes the
MI355X's 256 compute units, so the routes taken here are the routes an MI355X gets.  Three parts:
  plan     every rd_conv / rd_wgrad / rd_conv_bwd_fused / rd_conv_bwd_fused_reduce op of the fwd / bwd lists of all plan_dump.cases(),
           in list order, after bind_workspace
  sweep    descriptors built directly over the network's channel pairs, the bench geometries at every U-Net level, both dtypes and
           tap counts, every source mode / destination kind / accumulate / src.out / cu_limit / alignment rule, the fits32 and
           RD_CONV_NB1_BELOW thresholds, and the same for rd_wgrad_t and the fused backward; descriptors that fail validation are
           recorded with their return code
  forced   a fixed subset of the sweep under each dispatch-switch environment of forced_dispatch.ENVS (debug library, child process)
An entry is {desc: a label, rc, routes: [{kernel, grid, block, lds, iarg}], + honours (rd_conv_honours_src_out) or ws (workspace bytes)}.

tests/golden/conv_routes.json holds one SHA-256 and a count by kernel name per group.  It was generated from the commit BEFORE the
routing functions existed, by recording what that commit's entry points handed to its launch wrapper (the recipe is in the message of
the commit that added this file), and must never be regenerated from later code: a differing digest means the later code routes a
launch differently.  To see what differs, write the full routes of two trees and diff them:

    python tests/route_dump.py OUT_DIR            # OUT_DIR/plan.json, sweep.json, forced.json + conv_routes.json in the golden's format
"""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'ram-dsir_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ramdsir import _lib as L           # noqa: E402
import forced_dispatch                  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')
BF16, F32 = L.RD_BF16, L.RD_F32
CHILD = [sys.executable, os.path.abspath(__file__)]       # the process forced() starts


# ------------------------------------------------------------------------------------------------ kernel names
def _mangled_args(s, i):
    """Template arguments of an Itanium-mangled name from s[i] == 'I' to the matching 'E' (the few forms the kernels use)."""
    out, i = [], i + 1
    while s[i] != 'E':
        if s.startswith('DF16b', i):
            out.append('bf16')
            i += 5
        elif s[i] == 'f':
            out.append('float')
            i += 1
        else:
            m = re.match(r'L([ib])(n?\d+)E', s[i:])
            assert m, s[i:]
            v = m.group(2).replace('n', '-')
            out.append(v if m.group(1) == 'i' else ('true' if v == '1' else 'false'))
            i += m.end()
    return out


def norm_kernel(name):
    """One spelling per instantiation, from the source's spelling ('conv_kernel<bf16_t, 9, 2>') or from the mangled symbol of its host handle or stub
    ('_ZN12_GLOBAL__N_111conv_kernelIDF16bLi9ELi2EEEv...', '..._126__device_stub__conv_kernelI...'): 'conv_kernel<bf16, 9, 2>'."""
    if name.startswith('_Z'):
        m = re.search(r'_GLOBAL__N_1L?(\d+)(__device_stub__)?', name)
        n = int(m.group(1)) - len(m.group(2) or '')
        base, rest = name[m.end():m.end() + n], m.end() + n
        args = _mangled_args(name, rest) if name[rest] == 'I' else []
    else:
        base, _, a = name.partition('<')
        args = [x.strip().replace('bf16_t', 'bf16') for x in a.rstrip('> ').split(',')] if a else []
    return base + ('<%s>' % ', '.join(args) if args else '')


# ------------------------------------------------------------------------------------------------ the library's answers
def _rec(r):
    return {'kernel': norm_kernel(r.kernel.decode()), 'grid': list(r.grid), 'block': r.block, 'lds': r.lds, 'iarg': list(r.iarg)}


class Routes:
    """The routing queries of the library under test.  Each method returns (return code, route records [, extra fields])."""

    def __init__(self):
        self.lib = L.lib()

    def conv(self, p, dt):
        r = L.RdRoute()
        rc = self.lib.rd_conv_route(C.byref(p), dt, C.byref(r))
        honours = self.lib.rd_conv_honours_src_out(C.byref(p), dt)
        assert honours == (r.stores_sources if rc == 0 else 0), 'rd_conv_honours_src_out disagrees with the route'
        return rc, [_rec(r)] if rc == 0 else [], {'honours': honours if rc == 0 else None}    # a refused launch writes nothing: not compared

    def wgrad(self, w, dt):
        r = (L.RdRoute * 2)()
        n = self.lib.rd_wgrad_route(C.byref(w), dt, r)
        return n, [_rec(r[i]) for i in range(max(n, 0))], {'ws': self.lib.rd_wgrad_workspace(C.byref(w), dt) if n > 0 else None}

    def fused(self, p, w, dt):
        """Both launches of the pair: [rd_conv_bwd_fused, rd_conv_bwd_fused_reduce]."""
        r = (L.RdRoute * 2)()
        n = self.lib.rd_conv_bwd_fused_route(C.byref(p), C.byref(w), dt, r)
        return n, [_rec(r[i]) for i in range(max(n, 0))], {'ws': self.lib.rd_conv_bwd_fused_workspace(C.byref(p), C.byref(w), dt)}


def entry(label, answer):
    rc, routes, extra = answer
    return dict(desc=label, rc=rc, routes=routes, **extra)


def check_workspace(e, taps):
    """The workspace the library asks for is the one the routed launches address: nsplit x taps x pads of the split reduction."""
    if e.get('ws') is not None and len(e['routes']) == 2:
        a = e['routes'][1]['iarg']
        assert e['ws'] == a[0] * a[1] * a[4] * a[5] * 4 and a[1] == taps, e


# ------------------------------------------------------------------------------------------------ part a: the plans' launches
def plan_routes(routes):
    """case name -> entries, one per conv-family op of every plan of the case, in list order."""
    import plan_dump as PD
    out, sink, dts = {}, [], {}
    real = PD.dump_plan

    def capture(name, plan, reg):
        for lst in ('fwd', 'bwd'):
            for i, op in enumerate(getattr(plan, lst)):
                fn, a = op[0].__name__, op[1]
                where = '%s.%s[%d] %s' % (name, lst, i, fn)
                if fn == 'rd_conv':
                    sink.append(entry(where, routes.conv(a[0]._obj, a[1])))
                elif fn == 'rd_wgrad':
                    sink.append(entry(where, routes.wgrad(a[0]._obj, a[1])))
                    check_workspace(sink[-1], a[0]._obj.taps)
                elif fn in ('rd_conv_bwd_fused', 'rd_conv_bwd_fused_reduce'):
                    rc, r, extra = routes.fused(a[0]._obj, a[1]._obj, a[2])
                    assert rc == 2, where
                    sink.append(entry(where, (rc, r[:1] if fn == 'rd_conv_bwd_fused' else r[1:], extra)))
                    check_workspace(dict(sink[-1], routes=r), 9)
        return real(name, plan, reg)

    PD.dump_plan = capture
    try:
        for name, fn in PD.cases().items():
            del sink[:]
            fn()
            out[name] = list(sink)
    finally:
        PD.dump_plan = real
    return out


# ------------------------------------------------------------------------------------------------ part b: descriptors built directly
PAIRS = [(3, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256),
         (384, 128), (192, 64), (96, 32), (48, 16),           # the decoder's concatenated inputs (upsampled + skip)
         (32, 2), (16, 3)]
SIDES = [24, 25, 48, 50, 96, 100, 192, 200, 384, 400, 512]
BATCHES = [2, 8, 10, 16, 20]
PLAIN = (L.SRC_RAW, L.SRC_AFF, L.SRC_AFFACT)
_next = [0]


def fake(misaligned=False):
    """A fresh fake address: 16-byte aligned (4 bytes off when `misaligned`), far from every other."""
    _next[0] += 1
    return 0x100000000 + _next[0] * 0x10000000 + (4 if misaligned else 0)


def gstart(N, G):
    return L.gstart_array([i * N // G for i in range(G)] + [N])


def src(mode, Cc, bad=None):
    s = L.RdSrc()
    s.ptr, s.mode, s.C, s.slope, s.g_fixed = fake(bad == 'ptr'), mode, Cc, 0.0, -1
    if mode != L.SRC_RAW:
        s.scale, s.shift = fake(bad == 'scale'), fake()
    if mode == L.SRC_BNBWD:
        s.ptr2, s.q = fake(bad == 'ptr2'), fake(bad == 'q')
    return s


def conv_desc(dt, taps, cin, cout, N, side, emode=0, modes=(L.SRC_AFFACT,), split=None, kinds=(L.DST_PLAIN,), accumulate=0, out=False,
              cu_limit=0, G=1, bad=None, w_tap_rows=0, stat_slots=0, H=None):
    """One rd_conv_t.  Forward (emode 0): `cin` channels from one source or, with two modes, from two sources of split / cin - split
    channels.  Gradient (emode 1): `cin` channels of dz -> `cout` channels of input gradient, into one destination or two (c_split)."""
    ck = 32 if dt == BF16 else 16
    p = L.RdConv()
    p.nsrc, p.taps, p.w, p.bias = len(modes), taps, fake(bad == 'w'), fake()
    widths = [cin] if len(modes) == 1 else [split, cin - split]
    for i, m in enumerate(modes):
        p.src[i] = src(m, widths[i], bad if i == 0 else None)
        if out:
            p.src[i].out = fake()
    p.Cin, p.Cout, p.CinPad, p.CoutPad = cin, cout, (cin + ck - 1) // ck * ck, (cout + 31) // 32 * 32
    p.N, p.H, p.W, p.G, p.gstart = N, H or side, side, G, gstart(N, G)
    p.emode, p.cu_limit, p.w_tap_rows, p.stat_slots = emode, cu_limit, w_tap_rows, stat_slots
    if emode == 0:
        p.out, p.stats, p.c_split = fake(bad == 'out'), fake(), cout
    else:
        p.c_split = cout if len(kinds) == 1 else cout // 2
        for i in range(2):
            d = p.dst[i]
            d.kind = kinds[i] if i < len(kinds) else L.DST_NONE
            if d.kind == L.DST_NONE:
                continue
            d.g, d.z, d.scale, d.shift, d.bstats = fake(bad == 'g' and i == 0), fake(), fake(), fake(), fake()
            d.act, d.accumulate, d.slope, d.g_fixed = 1, accumulate, 0.0, -1
            d.Cd = cout if len(kinds) == 1 else (p.c_split if i == 0 else cout - p.c_split)
    return p


def wgrad_desc(taps, cin, cout, N, side, amodes=(L.SRC_AFFACT,), split=None, dzmode=L.SRC_BNBWD, G=1, cu_limit=0, bad=None):
    w = L.RdWgrad()
    w.na, w.taps = len(amodes), taps
    widths = [cin] if len(amodes) == 1 else [split, cin - split]
    for i, m in enumerate(amodes):
        w.a[i] = src(m, widths[i])
    w.dz = src(dzmode, cout)
    w.N, w.H, w.W, w.Cin, w.Cout, w.G, w.gstart = N, side, side, cin, cout, G, gstart(N, G)
    w.partial, w.dW, w.beta, w.cu_limit = fake(bad == 'partial'), fake(), 1.0, cu_limit
    return w


def fused_pair(cin, cout, N, side, dzmode=L.SRC_BNBWD, two=False, cu_limit=0, tweak=None):
    """The gradient rd_conv_t and the rd_wgrad_t of one small-channel 3x3 conv with `cin` inputs and `cout` outputs, as
    rd_conv_bwd_fused_ok wants them: the same dz, the destinations' producers as the weight gradient's operands."""
    p = conv_desc(BF16, 9, cout, cin, N, side, emode=1, modes=(dzmode,), kinds=(L.DST_PLAIN, L.DST_PLAIN) if two else (L.DST_PLAIN,),
                  cu_limit=cu_limit)
    if two:
        p.c_split = cin // 2
        p.dst[0].Cd, p.dst[1].Cd = p.c_split, cin - p.c_split
    w = wgrad_desc(9, cin, cout, N, side, amodes=(L.SRC_AFFACT,) * (2 if two else 1), split=cin // 2, dzmode=dzmode)
    w.dz = p.src[0]
    for i in range(w.na):
        d = p.dst[i]
        w.a[i].ptr, w.a[i].scale, w.a[i].shift, w.a[i].slope, w.a[i].n_off, w.a[i].g_fixed = d.z, d.scale, d.shift, d.slope, d.n_off, d.g_fixed
    if tweak == 'w_tap_rows':
        p.w_tap_rows = 32
    if tweak == 'misaligned_g':
        p.dst[0].g += 4
    return p, w


def sweep(routes):
    """group name -> entries."""
    out = {}

    def conv(group, label, dt, *a, **k):
        p = conv_desc(dt, *a, **k)
        out.setdefault(group, []).append(entry(label, routes.conv(p, dt)))

    # every channel pair at every bench geometry: the forward launch and the input-gradient launch of the same conv
    for dname, dt in (('bf16', BF16), ('f32', F32)):
        for taps in (9, 1):
            for cin, cout in PAIRS:
                for side in SIDES:
                    for N in BATCHES:
                        lab = '%d->%d %dx%dx%d' % (cin, cout, N, side, side)
                        conv('geometry.%s.taps%d.forward' % (dname, taps), lab, dt, taps, cin, cout, N, side)
                        conv('geometry.%s.taps%d.gradient' % (dname, taps), lab, dt, taps, cout, cin, N, side, emode=1, modes=(L.SRC_BNBWD,))
    # the options, over one geometry per U-Net level and a small-channel, a 32-wide and two 64-wide pairs
    levels = [(2, 400), (8, 200), (16, 100), (10, 50), (20, 25), (8, 24)]
    for dname, dt in (('bf16', BF16), ('f32', F32)):
        for taps in (9, 1):
            g = 'options.%s.taps%d.' % (dname, taps)
            for cin, cout in ((16, 16), (32, 32), (64, 96), (64, 64), (128, 128), (16, 3)):
                for N, side in levels:
                    lab = '%d->%d %dx%dx%d ' % (cin, cout, N, side, side)
                    for m in (L.SRC_RAW, L.SRC_AFF, L.SRC_AFFACT, L.SRC_POOL, L.SRC_UP):
                        for o in (False, True):
                            conv(g + 'sources', lab + 'mode%d out%d' % (m, o), dt, taps, cin, cout, N, side, modes=(m,), out=o)
                    for m in (L.SRC_BNBWD, L.SRC_RAW):
                        for o in (False, True):
                            conv(g + 'sources', lab + 'grad mode%d out%d' % (m, o), dt, taps, cin, cout, N, side, emode=1, modes=(m,), out=o)
                    if cin >= 16:
                        for ms in ((L.SRC_AFFACT, L.SRC_AFFACT), (L.SRC_UP, L.SRC_AFFACT), (L.SRC_AFF, L.SRC_RAW)):
                            for o in (False, True):
                                conv(g + 'sources', lab + 'two %d,%d out%d' % (ms + (o,)), dt, taps, cin, cout, N, side, modes=ms, split=cin // 2, out=o)
                        conv(g + 'sources', lab + 'two ragged', dt, taps, cin, cout, N, side, modes=(L.SRC_AFFACT, L.SRC_AFFACT), split=cin // 2 - 4)
                    for kinds in ((L.DST_PLAIN,), (L.DST_POOL,), (L.DST_UPY,), (L.DST_NONE,), (L.DST_PLAIN, L.DST_PLAIN), (L.DST_PLAIN, L.DST_UPY),
                                  (L.DST_POOL, L.DST_UPY), (L.DST_NONE, L.DST_PLAIN)):
                        for acc in (0, 1):
                            for m in (L.SRC_BNBWD, L.SRC_RAW):
                                conv(g + 'destinations', lab + 'kinds%s acc%d mode%d' % (list(kinds), acc, m), dt, taps, cin, cout, N, side, emode=1,
                                     modes=(m,), kinds=kinds, accumulate=acc)
                    for cu in (0, 96, 128, 160):
                        for G in (1, 3):
                            conv(g + 'budget', lab + 'cu%d G%d' % (cu, G), dt, taps, cin, cout, N, side, cu_limit=cu, G=G)
                            conv(g + 'budget', lab + 'grad cu%d G%d' % (cu, G), dt, taps, cin, cout, N, side, emode=1, modes=(L.SRC_BNBWD,), cu_limit=cu, G=G)
                    for bad in ('ptr', 'scale', 'w', 'out'):
                        conv(g + 'alignment', lab + 'misaligned ' + bad, dt, taps, cin, cout, N, side, bad=bad)
                    for bad in ('ptr', 'ptr2', 'q', 'scale', 'g'):
                        conv(g + 'alignment', lab + 'grad misaligned ' + bad, dt, taps, cin, cout, N, side, emode=1, modes=(L.SRC_BNBWD,), bad=bad)
                    for rows in (0, 32, 64, 16):
                        conv(g + 'validation', lab + 'w_tap_rows%d' % rows, dt, taps, cin, cout, N, side, emode=1, modes=(L.SRC_BNBWD,), w_tap_rows=rows)
                        conv(g + 'validation', lab + 'forward w_tap_rows%d' % rows, dt, taps, cin, cout, N, side, w_tap_rows=rows)
    # thresholds: RD_CONV_NB1_BELOW (300 workgroups of 64 channels), one tile per CU (conv_pp_kernel), the 32-bit offsets of conv_ws_kernel
    # (2^24 pixels, 2^32 bytes) and of the small-channel forward kernel (2^31 elements), 72 KB of LDS (CinPad), the coefficient table (G)
    for N in range(1, 21):
        for side in (50, 100):
            for cout in (64, 128):
                conv('thresholds.workgroups', '64->%d %dx%dx%d' % (cout, N, side, side), BF16, 9, 64, cout, N, side)
                conv('thresholds.workgroups', 'grad 64->%d %dx%dx%d' % (cout, N, side, side), BF16, 9, cout, 64, N, side, emode=1, modes=(L.SRC_BNBWD,))
    for N, side, H in ((1, 4096, 4095), (1, 4096, 4096), (4, 2048, 2048), (4, 2048, 2047), (16, 1024, 1023), (16, 1024, 1024), (2, 4096, 2048)):
        for cin, cout in ((64, 64), (64, 128), (64, 256), (32, 32), (16, 16)):
            conv('thresholds.fits32', '%d->%d %dx%dx%d' % (cin, cout, N, H, side), BF16, 9, cin, cout, N, side, H=H)
            conv('thresholds.fits32', 'grad %d->%d %dx%dx%d' % (cin, cout, N, H, side), BF16, 9, cout, cin, N, side, H=H, emode=1, modes=(L.SRC_BNBWD,))
    for cin in (512, 544, 1024, 1056, 2048, 4096, 8192):
        for cout in (32, 64):
            conv('thresholds.lds', '%d->%d' % (cin, cout), BF16, 9, cin, cout, 8, 100)
            conv('thresholds.lds', '1x1 %d->%d' % (cin, cout), BF16, 1, cin, cout, 8, 100)
            conv('thresholds.lds', 'grad %d->%d' % (cin, cout), BF16, 9, cin, cout, 8, 100, emode=1, modes=(L.SRC_BNBWD,))
    for G in (1, 2, 4, 8, 12, 16):
        conv('thresholds.groups', 'G%d' % G, BF16, 9, 64, 64, 16, 100, G=G)
        conv('thresholds.groups', 'grad G%d' % G, BF16, 9, 256, 256, 16, 100, emode=1, modes=(L.SRC_BNBWD,), G=G)
    # descriptors rd_conv refuses
    for dname, dt in (('bf16', BF16), ('f32', F32)):
        for lab, k in (('taps3', dict(taps=3)), ('G0', dict(G=0)), ('G17', dict(G=17)), ('nsrc0', dict(nsrc=0)), ('nsrc3', dict(nsrc=3)),
                       ('CinPad ragged', dict(CinPad=72)), ('CoutPad ragged', dict(CoutPad=48)), ('CinPad small', dict(Cin=80)),
                       ('CoutPad small', dict(Cout=80)), ('stat_slots-1', dict(stat_slots=-1)), ('stat_slots65', dict(stat_slots=65)),
                       ('stat_slots8', dict(stat_slots=8))):
            p = conv_desc(dt, 9, 64, 64, 8, 100)
            for f, v in k.items():
                setattr(p, f, v)
            out.setdefault('validation', []).append(entry('%s %s' % (dname, lab), routes.conv(p, dt)))
    # ---- rd_wgrad
    for dname, dt in (('bf16', BF16), ('f32', F32)):
        for taps in (9, 1):
            g = 'wgrad.%s.taps%d.' % (dname, taps)
            for cin, cout in PAIRS:
                for side in SIDES:
                    for N in (2, 8, 16, 20):
                        for dz in (L.SRC_BNBWD, L.SRC_RAW):
                            w = wgrad_desc(taps, cin, cout, N, side, dzmode=dz)
                            out.setdefault(g + 'geometry', []).append(entry('%d->%d %dx%dx%d dz%d' % (cin, cout, N, side, side, dz), routes.wgrad(w, dt)))
            for cin, cout in ((16, 16), (32, 16), (32, 32), (64, 64), (128, 128), (256, 128), (192, 64), (3, 16)):
                for N, side in levels:
                    lab = '%d->%d %dx%dx%d ' % (cin, cout, N, side, side)
                    ws = []
                    for am in ((L.SRC_RAW,), (L.SRC_AFF,), (L.SRC_POOL,), (L.SRC_UP,), (L.SRC_AFFACT, L.SRC_AFFACT), (L.SRC_UP, L.SRC_AFFACT)):
                        if len(am) == 2 and cin < 16:
                            continue
                        for split in ((cin // 2, cin // 4 * 3, cin // 2 - 4) if len(am) == 2 else (None,)):
                            for dz in (L.SRC_BNBWD, L.SRC_RAW):
                                ws.append(('a%s split%s dz%d' % (list(am), split, dz), dict(amodes=am, split=split, dzmode=dz)))
                    for G in (1, 3, 8, 9, 16):
                        for cu in (0, 96, 128, 160):
                            ws.append(('G%d cu%d' % (G, cu), dict(G=G, cu_limit=cu)))
                    ws.append(('partial misaligned', dict(bad='partial')))
                    for l2, k in ws:
                        w = wgrad_desc(taps, cin, cout, N, side, **k)
                        out.setdefault(g + 'options', []).append(entry(lab + l2, routes.wgrad(w, dt)))
            for lab, k in (('taps3', dict(taps=3)), ('G0', dict(G=0)), ('G17', dict(G=17)), ('na0', dict(na=0)), ('na3', dict(na=3))):
                w = wgrad_desc(taps, 64, 64, 8, 100)
                for f, v in k.items():
                    setattr(w, f, v)
                out.setdefault(g + 'options', []).append(entry('refused ' + lab, routes.wgrad(w, dt)))
            w = wgrad_desc(taps, 64, 64, 8, 100)
            w.a[0].fin = fake()
            out.setdefault(g + 'options', []).append(entry('refused a.fin', routes.wgrad(w, dt)))
    for g in [g for g in out if g.startswith('wgrad.')]:
        for e in out[g]:
            check_workspace(e, int(g.split('taps')[1].split('.')[0]))
    # ---- the fused backward of the small-channel 3x3 convs
    for cin, cout in ((3, 16), (8, 16), (16, 16), (16, 32), (32, 32), (32, 16), (32, 8), (16, 3), (32, 2), (64, 32)):
        for side in SIDES:
            for N in BATCHES:
                for dz in (L.SRC_BNBWD, L.SRC_RAW):
                    for cu in (0, 96, 128, 160):
                        p, w = fused_pair(cin, cout, N, side, dzmode=dz, cu_limit=cu)
                        e = entry('%d->%d %dx%dx%d dz%d cu%d' % (cin, cout, N, side, side, dz, cu), routes.fused(p, w, BF16))
                        check_workspace(e, 9)
                        out.setdefault('fused', []).append(e)
    for N, side in levels:
        for two in (False, True):
            for tweak in (None, 'w_tap_rows', 'misaligned_g'):
                p, w = fused_pair(32, 32, N, side, two=two, tweak=tweak)
                out.setdefault('fused', []).append(entry('32->32 %dx%dx%d two%d %s' % (N, side, side, two, tweak), routes.fused(p, w, BF16)))
        p, w = fused_pair(32, 32, N, side)
        out.setdefault('fused', []).append(entry('32->32 %dx%dx%d f32' % (N, side, side), routes.fused(p, w, F32)))
    return out


# ------------------------------------------------------------------------------------------------ part c: forced switches
def forced_subset(routes):
    """~50 bf16 3x3 descriptors: every 64-wide and every small-channel pair forward, and the 64-wide gradients, above and below the
    workgroup threshold of the 64-channel tiles."""
    out = []
    for cin, cout in PAIRS:
        small = cin <= 32 and cout <= 32
        if not small and cout % 64:
            continue
        for N, side in ((8, 100), (2, 50)):
            lab = '%d->%d %dx%dx%d' % (cin, cout, N, side, side)
            out.append(entry(lab, routes.conv(conv_desc(BF16, 9, cin, cout, N, side), BF16)))
            if not small:
                out.append(entry('grad ' + lab, routes.conv(conv_desc(BF16, 9, cout, cin, N, side, emode=1, modes=(L.SRC_BNBWD,)), BF16)))
    out.append(entry('grad staged 64->64', routes.conv(conv_desc(BF16, 9, 64, 64, 8, 100, emode=1, modes=(L.SRC_BNBWD,), kinds=(L.DST_POOL,)), BF16)))
    out.append(entry('1x1 64->64', routes.conv(conv_desc(BF16, 1, 64, 64, 8, 100), BF16)))
    return out


def forced(env):
    """The subset's routes in a child process that loads the debug library under `env` (the switches are read once per process)."""
    e = {k: v for k, v in os.environ.items() if not k.startswith('RD_')}
    e.update(env, RAMDSIR_DEBUG_LIB='1')
    r = subprocess.run(CHILD + ['--forced-child'], env=e, stdout=subprocess.PIPE, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])          # the last line: a runtime may print notices first


def forced_all():
    out = {'default': forced({})}
    for env, name in zip(forced_dispatch.ENVS, forced_dispatch.IDS):
        out[name] = forced(env)
    return out


# ------------------------------------------------------------------------------------------------ the golden's form
def digest(entries):
    counts = {}
    for e in entries:
        for r in e['routes']:
            counts[r['kernel']] = counts.get(r['kernel'], 0) + 1
        if not e['routes']:
            counts['rc %d' % e['rc']] = counts.get('rc %d' % e['rc'], 0) + 1
    return {'sha256': hashlib.sha256(json.dumps(entries, sort_keys=True).encode()).hexdigest(), 'n': len(entries), 'kernels': counts}


def kernel_names(entries):
    return sorted({r['kernel'] for e in entries for r in e['routes']})


def clear_environment():
    for k in [k for k in os.environ if k.startswith('RD_') or k == 'RAMDSIR_DEBUG_LIB']:
        del os.environ[k]


def main(argv, make_routes=Routes):
    if len(argv) == 2 and argv[1] == '--forced-child':
        _next[0] = 0
        print('\n' + json.dumps(forced_subset(make_routes())))
        return
    if len(argv) != 2:
        sys.exit('usage: route_dump.py OUT_DIR   (full routes: plan.json, sweep.json, forced.json, and conv_routes.json in the golden\'s format)')
    clear_environment()
    os.makedirs(argv[1], exist_ok=True)
    routes = make_routes()
    parts = {'plan': plan_routes(routes), 'sweep': sweep(routes), 'forced': forced_all()}
    golden = {}
    for part, groups in parts.items():
        with open(os.path.join(argv[1], part + '.json'), 'w') as f:
            json.dump(groups, f, indent=1, sort_keys=True)
        golden[part] = {g: digest(v) for g, v in groups.items()}
    with open(os.path.join(argv[1], 'conv_routes.json'), 'w') as f:
        f.write('{\n' + ',\n'.join('%s: {\n%s\n}' % (json.dumps(p), ',\n'.join(
            ' %s: %s' % (json.dumps(g), json.dumps(golden[p][g], sort_keys=True)) for g in sorted(golden[p]))) for p in sorted(golden)) + '\n}\n')


if __name__ == '__main__':
    main(sys.argv)
