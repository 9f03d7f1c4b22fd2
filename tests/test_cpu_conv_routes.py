"""CPU-only: the kernel, grid, block, LDS size and integer arguments of every conv / weight-gradient launch are, descriptor for
descriptor, the ones pinned in tests/golden/conv_routes.json (tests/route_dump.py says what is recorded, where the golden comes from
and how to diff two trees when a digest differs).  Needs the built libraries, like test_cpu_host.py; no launch is made.  The golden is
never regenerated from the code under test."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forced_dispatch                                      # noqa: E402
import route_dump as RD                                     # noqa: E402

with open(RD.GOLDEN) as _f:
    GOLDEN = json.load(_f)
HINT = ' (python tests/route_dump.py DIR on both trees, then diff)'


@pytest.fixture(autouse=True)
def _no_tuning_environment(monkeypatch):
    for k in [k for k in os.environ if k.startswith('RD_') or k == 'RAMDSIR_DEBUG_LIB']:
        monkeypatch.delenv(k)


def _compare(part, got):
    want = GOLDEN[part]
    assert sorted(got) == sorted(want)
    for g in sorted(got):
        d = RD.digest(got[g])
        assert d['kernels'] == want[g]['kernels'], '%s %s: launches by kernel differ%s' % (part, g, HINT)
        assert d == want[g], '%s %s: the same kernels with other grids / LDS sizes / arguments%s' % (part, g, HINT)


@pytest.fixture(scope='module')
def routes():
    return RD.Routes()


def test_plan_launches_match_golden(routes):
    """Every conv-family op of all plan_dump cases; route_dump also checks rd_wgrad_workspace / rd_conv_bwd_fused_workspace /
    rd_conv_honours_src_out against the same routes."""
    import plan_dump as PD
    got = RD.plan_routes(routes)
    assert sorted(got) == sorted(PD.cases()) and len(got) == 46
    _compare('plan', got)


def test_descriptor_sweep_matches_golden(routes):
    got = RD.sweep(routes)
    _compare('sweep', got)
    names = {k for g in got.values() for k in RD.kernel_names(g)}
    # the sweep reaches every family: the small-channel kernels, the persistent 64-wide one, both chunk-pipelined forms, the generic
    # kernel; 16 x 16, symmetric, warp-specialised, transpose-read and plain weight gradients, all three reductions; the fused backward.
    # (conv_pp_kernel wants at most one tile per CU and 64-channel tiles, which RD_CONV_NB1_BELOW's default keeps apart: it is reached
    # under the `pp_staged` switches only, see the forced part.)
    for family in ('conv_small_fwd_kernel', 'conv_small_kernel', 'conv_small_stage_kernel', 'conv_ws_kernel',
                   'conv_pf_kernel', 'conv_kernel', 'wgrad_c16_tr_kernel', 'wgrad_sym_kernel', 'wgrad_ws_kernel', 'wgrad_tr_kernel',
                   'wgrad_kernel', 'wgrad_reduce_kernel<8, 1>', 'wgrad_reduce_kernel<32, 4>', 'wgrad_reduce_kernel<32, 1>',
                   'conv_small_bwd_fused_kernel'):
        assert any(n.startswith(family) for n in names), family
    assert any(e['rc'] < 0 for e in got['validation']) and any(e['honours'] for g in got.values() for e in g if 'honours' in e)


# environments that name no kernel: RD_SW_TPW changes tiles per workgroup only, RD_SW_NWV=4 is the compiled-in default
SAME_KERNELS = ('small_fwd_tpw5', 'small_fwd_tpw2', 'small_fwd_nwv4', 'small_fwd_nwv4_tpw5')
SAME_ROUTES = ('small_fwd_nwv4',)


@pytest.fixture(scope='module')
def forced_default():
    return RD.forced({})


@pytest.mark.parametrize('name', ['default'] + forced_dispatch.IDS)
def test_forced_switches_reach_the_router(name, forced_default):
    """The debug library under each environment of test_conv_kernels_under_forced_dispatch routes the fixed subset as pinned, and NOT as
    the default environment does: another set of kernel names -- or, for the switches that only change tiles per workgroup, other route
    records; RD_SW_NWV=4 restates the default and must route exactly like it.  This is what shows that a switch still reaches the router
    (the GPU test would pass on the default kernels otherwise)."""
    got = forced_default if name == 'default' else RD.forced(forced_dispatch.ENVS[forced_dispatch.IDS.index(name)])
    _compare_one = RD.digest(got)
    want = GOLDEN['forced'][name]
    assert _compare_one['kernels'] == want['kernels'], '%s: launches by kernel differ%s' % (name, HINT)
    assert _compare_one == want, name + HINT
    assert 45 <= len(got) <= 60
    if name == 'default':
        return
    if name == 'pp_staged':
        assert 'conv_pp_kernel' in RD.kernel_names(got)
    assert (RD.kernel_names(got) == RD.kernel_names(forced_default)) == (name in SAME_KERNELS), name
    assert (got == forced_default) == (name in SAME_ROUTES), name
