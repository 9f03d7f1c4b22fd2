"""CPU-only tests of the host side: the C-ABI library loads and exports every symbol the header declares
(no compute calls without a GPU), the parameter layout equals the reference's state_dict manifest, the
gradient-bucket exchange averages correctly across 2 gloo ranks."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    txt = open(os.path.join(ROOT, 'include', 'ramdsir.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(rd_[a-z0-9_]+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    from ramdsir import _lib
    assert os.path.exists(_lib.LIB_PATH), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decl = _declared_functions()
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(lib, name), name
    assert sorted(_lib.exported_symbols()) == decl          # the ctypes binding covers the whole header


def test_ctypes_struct_sizes_match_the_c_compiler(tmp_path):
    """sizeof() of every descriptor struct as gcc lays it out == ctypes' layout (catches field drift)."""
    from ramdsir import _lib as L
    names = {'rd_src_t': L.RdSrc, 'rd_dst_t': L.RdDst, 'rd_conv_t': L.RdConv, 'rd_wgrad_t': L.RdWgrad, 'rd_bn_fwd_t': L.RdBnFwd,
             'rd_bn_bwd_t': L.RdBnBwd, 'rd_seg_loss_t': L.RdSegLoss, 'rd_adam_t': L.RdAdam, 'rd_pack_entry_t': L.RdPackEntry,
             'rd_ram_t': L.RdRam, 'rd_launch_t': L.RdLaunch, 'rd_route_t': L.RdRoute}
    src = '#include <stdio.h>\n#include "ramdsir.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + 'return 0;}'
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert ctypes.sizeof(cls) == sizes[n], n


def test_launch_list_packing_and_lanes():
    """engine.LaunchList (-> rd_run_list): entries in list order, lane / wait_main as Plan.run_lanes routes them, arguments packed as
    include/ramdsir.h says (pointers and integers as they are, a float as its bit pattern); no GPU call is made."""
    import struct
    from ramdsir import _lib as L, engine as E
    lib = L.lib()
    assert ctypes.sizeof(L.RdLaunch) == 16 + 8 * 18
    assert L.pack_arg(1.5, L.f32) == struct.unpack('<I', struct.pack('<f', 1.5))[0]
    assert L.pack_arg(-1, ctypes.c_int) == 0xFFFFFFFFFFFFFFFF and L.pack_arg(None, L.vp) == 0 and L.pack_arg(4096, L.vp) == 4096
    p, gs = L.RdConv(), L.gstart_array([0, 2, 4])
    assert L.pack_arg(ctypes.byref(p), ctypes.POINTER(L.RdConv)) == ctypes.addressof(p)
    assert L.pack_arg(gs, ctypes.POINTER(L.i32)) == ctypes.addressof(gs)
    ops = [(lib.rd_conv, (ctypes.byref(p), 1), dict(kernel='x')),
           E.sync_op('fork', 'rec'),
           (lib.rd_pool_fwd, (0x1000, None, None, 0.25, 0x2000, 4, 5, 6, 16, 2, gs, 1, None, 0), dict(lane='rec')),
           (lib.rd_wgrad, (ctypes.byref(L.RdWgrad()), 1), dict(side=True, side_idx=0)),
           E.sync_op('join', 'rec'),
           (lib.rd_adam_step, (ctypes.byref(L.RdAdam()),))]
    ll = E.LaunchList(ops, ('side0', 'rec'))
    got = [(e.op, e.lane, e.wait_main, e.nargs) for e in ll.arr[:ll.n]]
    oc = {n: L.op_code(n) for n in ('rd_conv', 'rd_pool_fwd', 'rd_wgrad', 'rd_adam_step')}
    assert got == [(oc['rd_conv'], 0, 0, 2), (L.OP_FORK, 2, 0, 0), (oc['rd_pool_fwd'], 2, 0, 14), (oc['rd_wgrad'], 1, 1, 2),
                   (L.OP_JOIN, 2, 0, 0), (oc['rd_adam_step'], 0, 0, 1)]
    e = ll.arr[2]
    assert e.a[0] == 0x1000 and e.a[1] == 0 and e.a[3] == L.pack_arg(0.25, L.f32) and e.a[10] == ctypes.addressof(gs) and e.a[11] == 1
    # without lanes everything runs on the main stream and the fork / join entries vanish (Plan.run_lanes' fallback)
    l0 = E.LaunchList(ops, ())
    assert [(e.op, e.lane, e.wait_main) for e in l0.arr[:l0.n]] == [(oc['rd_conv'], 0, 0), (oc['rd_pool_fwd'], 0, 0), (oc['rd_wgrad'], 0, 0),
                                                                    (oc['rd_adam_step'], 0, 0)]
    # which main-lane launches carry the event of the fork behind them on their own dispatch packet (rd_run_list_bind_fork_events):
    # the conv (a fork of `rec` and a lane entry with wait_main follow before the main stream moves on), not Adam (nothing follows)
    carries = (ctypes.c_ubyte * ll.n)()
    assert lib.rd_run_list_fork_plan(ll.arr, ll.n, carries) == 0
    assert list(carries) == [1, 0, 0, 0, 0, 0]
    ops2 = [(lib.rd_conv, (ctypes.byref(p), 1), dict(kernel='a')),                           # followed by another main-lane launch: no
            (lib.rd_conv, (ctypes.byref(p), 1), dict(kernel='b')),                           # followed by a weight gradient on the side lane: yes
            (lib.rd_wgrad, (ctypes.byref(L.RdWgrad()), 1), dict(side=True, side_idx=0)),
            (lib.rd_wgrad, (ctypes.byref(L.RdWgrad()), 1), dict(side=True, side_idx=0)),     # same position of the main stream: served by b's event
            (lib.rd_conv, (ctypes.byref(p), 1), dict(kernel='c')),                           # a join first: the main stream's position changes: no
            E.sync_op('join', 'side0'),
            (lib.rd_wgrad, (ctypes.byref(L.RdWgrad()), 1), dict(side=True, side_idx=0)),
            (lib.rd_adam_step, (ctypes.byref(L.RdAdam()),))]
    l2 = E.LaunchList(ops2, ('side0', 'rec'))
    c2 = (ctypes.c_ubyte * l2.n)()
    assert lib.rd_run_list_fork_plan(l2.arr, l2.n, c2) == 0
    assert list(c2) == [0, 1, 0, 0, 0, 0, 0, 0]
    # the op codes of the binding are the library's table (include/ramdsir.h RD_LAUNCH_OPS): these 24 names with these values, which are ABI
    names = ('rd_conv', 'rd_wgrad', 'rd_conv_bwd_fused', 'rd_conv_bwd_fused_reduce', 'rd_pack_weights_batched',
             'rd_bn_finalize_fwd', 'rd_bn_finalize_bwd', 'rd_gn_finalize_fwd', 'rd_gn_finalize_bwd',
             'rd_up_stats', 'rd_bn_stats', 'rd_up_bwd', 'rd_pool_fwd', 'rd_pool_bwd', 'rd_bn_apply',
             'rd_nchw_to_nhwc', 'rd_nhwc_to_nchw', 'rd_grad_in', 'rd_colsum',
             'rd_seg_loss', 'rd_rec_loss', 'rd_adam_step', 'rd_zero', 'rd_ram_mix')
    values = (10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33)
    assert [lib.rd_op_code(n.encode()) for n in names] == list(values) == [L.op_code(n) for n in names]
    for other in ('rd_wgrad_reduce', 'rd_run_list', 'rd_conv_route', 'rd_con', 'rd_convx', ''):
        assert lib.rd_op_code(other.encode()) == -1
    assert lib.rd_op_code(None) == -1 and (L.OP_FORK, L.OP_JOIN) == (1, 2)
    with pytest.raises(KeyError):
        L.op_code('rd_wgrad_reduce')
    txt = open(os.path.join(ROOT, 'include', 'ramdsir.h')).read()
    table = re.search(r'#define RD_LAUNCH_OPS\(X\)(.*?)\n#define', txt, re.S).group(1)
    assert tuple(re.findall(r'X\(\w+, (\w+)\)', table)) == names            # the header's rows, in this order
    assert [s.upper() for s in re.findall(r'X\((\w+), rd_', table)] == [n[3:].upper() for n in names]


def test_parameter_layout_equals_reference_manifest(golden_dir):
    from ramdsir import engine as E
    with open(os.path.join(golden_dir, 'state_manifest.json')) as f:
        man = json.load(f)
    for nm, specs in (('encoder', E.encoder_specs()), ('seg_decoder', E.decoder_specs()),
                      ('rec_decoder', E.rec_decoder_specs(16, 3, 3))):
        got = [[k, list(shape), str(dt)] for k, shape, kind, dt in specs]
        assert got == man[nm], nm
    bank = E.ParamBank([('enc', E.encoder_specs()), ('dec', E.decoder_specs()), ('rec', E.rec_decoder_specs(16, 3, 3))], 'cpu')
    assert bank.n == 3800021 and bank.module_range['enc'] == (0, 1967904)
    w = bank.p('dec', 'out1.weight')
    w.fill_(3.0)
    off, shape = bank.index[('dec', 'out1.weight')]
    assert float(bank.params[off]) == 3.0 and tuple(shape) == (2, 32, 3, 3)     # views alias the arena


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'ram-dsir_amd', 'ramdsir')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            assert 'oracle' not in open(os.path.join(pkg, fn)).read(), fn


def test_product_library_contains_no_packed_fp32(tmp_path):
    """THE ERRATUM BEHIND BOTH WRONG-RESULT BUGS of rounds 5 and 6 (scripts/probe/pk_canary.hip + mfma_spin.hip,
    profiles/r06_pk_opsel_erratum.txt): a packed fp32 instruction whose op_sel makes the LOW result read the HIGH dword of a source reads 0
    for it while a wave of ANOTHER kernel executes MFMAs on the same SIMD.  The compiler forms such instructions from complex arithmetic
    (the RAM butterflies) and from swapped bias adds (the conv epilogues) through the SLP vectorizer; the library is built with
    -fno-slp-vectorize -fno-vectorize, and the DEVICE CODE of the shipped library -- not only the flags -- is checked here: no packed fp32
    arithmetic, no packed instruction with op_sel at all.  (v_permlane32_swap, blamed in round 5, is exonerated and in use.)"""
    import shutil
    from ramdsir import _lib
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not os.path.exists(objdump):
        pytest.skip('llvm-objdump not in this image')
    so = shutil.copy(_lib.LIB_PATH, tmp_path / 'lib.so')
    subprocess.run([objdump, '--offloading', str(so)], cwd=tmp_path, check=True, capture_output=True)
    objs = [f for f in os.listdir(tmp_path) if f.endswith('gfx950')]
    assert objs, 'no gfx950 code objects found in the library'
    n_inst, n_mfma, n_pkf32, n_opsel = 0, 0, 0, 0
    for f in objs:
        dis = subprocess.run([objdump, '-d', str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        n_inst += dis.count('v_permlane32_swap')
        n_mfma += dis.count('v_mfma_f32_32x32x16_bf16')
        n_pkf32 += len(re.findall(r'v_pk_(?:fma|mul|add)_f32', dis))
        n_opsel += len(re.findall(r'v_pk_\w+ [^\n]*op_sel', dis))
    assert n_mfma > 100                                     # the disassembly is the real thing
    assert n_inst > 0                                       # the regroup instruction is back (exonerated: conv_device.h rd_half_swap)
    assert n_pkf32 == 0, f'{n_pkf32} packed fp32 instructions in the product library (build flags lost?)'
    assert n_opsel == 0, f'{n_opsel} packed instructions with op_sel in the product library'


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path[:0] = [%r, %r]
from ramdsir.ddp import GradBuckets
rank, world = int(sys.argv[1]), int(sys.argv[3])
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=sys.argv[2], RANK=str(rank), WORLD_SIZE=str(world))
dist.init_process_group('gloo', rank=rank, world_size=world)
g = torch.arange(10, dtype=torch.float32) * (rank + 1)
b = GradBuckets(g, [0, 1, 4, 10])
assert len(b) == 3
ws = [b.reduce(2, async_op=True), b.reduce(1, async_op=True), b.reduce(0, async_op=False)]
for w in ws:
    if w is not None: w.wait()
exp = torch.arange(10, dtype=torch.float32) * (world + 1) / 2.0          # mean over the ranks of (rank + 1)
assert torch.allclose(g, exp), (g, exp)
# the loss scalars train.py logs: one all-reduce, the mean over the ranks (every rank calls it)
l = torch.full((8,), float(rank))
dist.all_reduce(l)
assert torch.allclose(l / world, torch.full((8,), (world - 1) / 2.0))
# DistributedSampler shards of one domain's file list (train.py:216-225): disjoint, equal length, reshuffled per epoch
from torch.utils.data.distributed import DistributedSampler
ds = list(range(103))
sp = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=1337, drop_last=True)
sp.set_epoch(0)
mine = torch.tensor(list(sp))
allr = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(allr, mine)
flat = torch.cat(allr).tolist()
assert len(mine) == 103 // world and len(set(flat)) == len(flat), (len(mine), len(flat))
sp.set_epoch(1)
assert list(sp) != mine.tolist()
dist.destroy_process_group()
print('ok')
'''


def test_every_kernel_launch_goes_through_rd_launch():
    """csrc/common.h rd_launch is the ONE launch site of the library: the launch list binds a lane fork's event to the producing launch's
    own dispatch packet through it (rd_run_list_bind_fork_events).  Behind a raw hipLaunchKernelGGL / <<< >>> elsewhere in a
    multi-launch entry point, a bound fork would wait for the launch BEFORE it only.  (rd_zero's hipMemsetAsync fallback reports
    that it bound nothing, and the fork records.)"""
    import glob
    csrc = os.path.join(ROOT, 'ram-dsir_amd', 'csrc')
    offenders = []
    for f in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        if os.path.basename(f) == 'common.h':
            continue
        for n, line in enumerate(open(f), 1):
            code = line.split('//')[0]
            if 'hipLaunchKernelGGL' in code or '<<<' in code or 'hipExtLaunchKernelGGL' in code or 'hipModuleLaunchKernel' in code:
                offenders.append('%s:%d' % (os.path.basename(f), n))
    assert not offenders, offenders
    txt = open(os.path.join(csrc, 'common.h')).read()
    assert 'hipExtLaunchKernelGGL(kernel, grid, block' in txt and 'rd_tls_stop_used = 1' in txt


@pytest.mark.parametrize('world', [2, 8])
def test_gradient_buckets_average_over_gloo_ranks(tmp_path, world):
    """ramdsir.ddp.GradBuckets (three buckets, asynchronous + synchronous reduce), the loss-scalar mean and the DistributedSampler
    shards at world 2 and at the node's real rank count 8, gloo on CPU."""
    script = tmp_path / 'w.py'
    script.write_text(_WORKER % (ROOT, os.path.join(ROOT, 'ram-dsir_amd')))
    port = str(29500 + (os.getpid() + 17 * world) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), port, str(world)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and 'ok' in o, o


def test_dataloader_worker_cap_divides_the_host_between_ranks_and_domains():
    """train.py: 8 workers per domain loader on one GPU (the reference's num_workers, train.py:558); under torchrun the
    host's cores are shared by ranks x domain loaders."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('rd_train', os.path.join(ROOT, 'ram-dsir_amd', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.worker_cap(8, 1, 3, cpus=64) == 8
    assert m.worker_cap(8, 8, 3, cpus=128) == 5             # 8 ranks x 3 loaders x 5 = 120 <= 128 (uncapped: 192)
    assert m.worker_cap(8, 8, 3, cpus=16) == 1
    assert m.worker_cap(0, 8, 3, cpus=128) == 0             # in-process loading stays in-process
    assert m.worker_cap(2, 2, 3, cpus=256) == 2


def test_tuning_options_and_cu_budget_defaults():
    from ramdsir import tuning as T
    o = T.options(dict(side_cus=0, rec_cus=None))
    assert o['side_cus'] == 0 and o['rec_cus'] == -1 and o['ddp_own_comm_stream'] == -1 and o['dgrad_cus'] == 160
    assert T.cu_budget(96, None) == 96 and T.cu_budget(0, None) == 0
    with pytest.raises(KeyError):
        T.options(dict(no_such_option=1))


def test_pmc_aggregation_of_the_bench_line():
    """bench.pmc_aggregate (shared by the live PMC child run and scripts/pmc_traffic.py): FETCH_SIZE / WRITE_SIZE rows of separate
    passes -> bytes = (2 * FETCH + WRITE) * 1024 per launch of a kernel family (a weight-gradient launch = MFMA kernel + its reduce)
    and per step (= per dispatch of the once-per-step Adam kernel; the tensor library's fills excluded)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('rd_bench_t', os.path.join(ROOT, 'bench.py'))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    ws = 'void (anonymous namespace)::wgrad_ws_kernel<2, 0>(rd_wgrad_t, int, int, int)'
    red = 'void (anonymous namespace)::wgrad_reduce_kernel<32>(float const*, float*, int)'
    adam = 'void (anonymous namespace)::adam_update_kernel(rd_adam_t)'
    fill = '_ZN2at6native29vectorized_elementwise_kernelIfill'
    rows = []
    for step in range(2):
        for c, (v_ws, v_red, v_adam) in (('FETCH_SIZE', (100.0, 10.0, 5.0)), ('WRITE_SIZE', (40.0, 2.0, 3.0))):
            rows += [dict(Kernel_Name=ws, Counter_Name=c, Counter_Value=str(v_ws)), dict(Kernel_Name=ws, Counter_Name=c, Counter_Value=str(v_ws)),
                     dict(Kernel_Name=red, Counter_Name=c, Counter_Value=str(v_red)), dict(Kernel_Name=red, Counter_Name=c, Counter_Value=str(v_red)),
                     dict(Kernel_Name=adam, Counter_Name=c, Counter_Value=str(v_adam)), dict(Kernel_Name=fill, Counter_Name=c, Counter_Value='1000')]
    out = B.pmc_aggregate(rows, 8, 'bf16', 400)
    w = out['wgrad']
    assert w['launches_profiled'] == 4                                        # the reduce kernels are not launches of their own
    assert w['traffic_bytes_per_launch'] == (2 * 110.0 + 42.0) * 1024
    st = out['step']
    assert st['steps_profiled'] == 2 and st['batch'] == 8 and st['dtype'] == 'bf16'
    assert st['traffic_bytes_per_step'] == (2 * (2 * 110.0 + 5.0) + (2 * 42.0 + 3.0)) * 1024        # the at:: fill is not ours
    assert 'conv64' not in out                                                # a family without dispatches is absent, not zero


def test_sq_counter_aggregation_of_the_bench_line():
    """bench.sq_aggregate: matrix-pipe busy fraction = MFMA busy cycles / (1024 SIMDs x kernel cycles), kernel cycles = GRBM_GUI_ACTIVE / 8
    XCDs, weighted over dispatches; LDS conflict ratio = SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('rd_bench_s', os.path.join(ROOT, 'bench.py'))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    acc = {('void (anonymous namespace)::conv_ws_kernel<1, 1, false, false>(rd_conv_t, int)', '131072', '512'):
           {'GRBM_GUI_ACTIVE': [8000.0, 8000.0], 'SQ_VALU_MFMA_BUSY_CYCLES': [256000.0, 256000.0], 'SQ_LDS_BANK_CONFLICT': [10.0, 30.0],
            'SQ_LDS_IDX_ACTIVE': [1000.0, 1000.0]},
           ('void (anonymous namespace)::adam_update_kernel(rd_adam_t)', '1048576', '256'): {'GRBM_GUI_ACTIVE': [800.0], 'SQ_VALU_MFMA_BUSY_CYCLES': [0.0]}}
    out = B.sq_aggregate(acc)
    c = out['conv64']
    assert c['dispatches'] == 2 and c['mfma_busy'] == round(256000.0 / (1024 * 1000.0), 4) == 0.25
    assert c['mfma_busy_occupied'] == 0.25 and c['lds_conflict_ratio'] == 0.02          # 256 workgroups occupy the whole device
    assert 'wgrad' not in out


def test_dsbn_module_keeps_the_reference_surface():
    """code/networks/dsbn.py:4-34: the base-class name, reset_running_stats / reset_parameters over every domain, the 4-D check and
    the checkpoint keys (bns.{d}.*) -- on CPU, no compute call."""
    from torch import nn
    from networks import dsbn
    m = dsbn.DomainSpecificBatchNorm2d(6, num_domains=3)
    assert issubclass(dsbn.DomainSpecificBatchNorm2d, dsbn._DomainSpecificBatchNorm)
    assert sorted(m.state_dict()) == sorted('bns.%d.%s' % (d, k) for d in range(3)
                                            for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'))
    assert all(isinstance(b, nn.BatchNorm2d) for b in m.bns)
    for b in m.bns:
        b.running_mean.fill_(3.0); b.running_var.fill_(5.0); b.num_batches_tracked.fill_(7)
        with torch.no_grad():
            b.weight.fill_(2.0); b.bias.fill_(1.0)
    m.reset_running_stats()
    for b in m.bns:
        assert float(b.running_mean.abs().max()) == 0 and float(b.running_var.min()) == 1 and int(b.num_batches_tracked) == 0
        assert float(b.weight.min()) == 2.0                    # parameters untouched
    m.reset_parameters()
    for b in m.bns:
        assert float(b.weight.min()) == 1.0 and float(b.bias.abs().max()) == 0.0
    with pytest.raises(ValueError):
        m(torch.zeros(2, 6, 4), torch.zeros(2, dtype=torch.long))
