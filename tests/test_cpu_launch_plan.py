"""CPU-only: the launch plans engine.Plan builds are, descriptor for descriptor, the ones pinned in tests/golden/launch_plan.json
(tests/plan_dump.py says what a dump holds and how to diff two trees when a digest differs).  Needs the built library, like
test_cpu_host.py; no launch is made.  The golden is never regenerated from the code under test."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_dump as PD                                      # noqa: E402

CASES = PD.cases()
with open(PD.GOLDEN) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(autouse=True)
def _no_tuning_environment(monkeypatch):
    for k in [k for k in os.environ if k.startswith('RD_') or k == 'RAMDSIR_DEBUG_LIB']:
        monkeypatch.delenv(k)


def _launches(d, plan):
    return tuple(sum(d[plan]['launches'][lst].values()) for lst in ('fwd', 'bwd'))


def test_golden_covers_exactly_the_pinned_cases():
    assert sorted(GOLDEN) == sorted(CASES)
    # the launch counts the dump tool was validated with, on the commit the golden comes from
    for dt, seg, rec in (('bf16', (35, 82), (17, 40)), ('f32', (35, 88), (17, 43))):
        assert (_launches(GOLDEN['step32.%s.default' % dt], 'seg'), _launches(GOLDEN['step32.%s.default' % dt], 'rec')) == (seg, rec)
        g0 = GOLDEN['step32.%s.fold_finalize=0' % dt]
        assert (_launches(g0, 'seg'), _launches(g0, 'rec')) == ((61, 88), (29, 43))


@pytest.mark.parametrize('name', sorted(CASES))
def test_launch_plan_matches_golden(name):
    got = {plan: PD.digest(d) for plan, d in CASES[name]().items()}
    want = GOLDEN[name]
    assert sorted(got) == sorted(want)
    for plan in sorted(got):
        assert got[plan]['launches'] == want[plan]['launches'], (name, plan)
        for part in PD.PARTS:
            assert got[plan][part] == want[plan][part], '%s: %s.%s differs (python tests/plan_dump.py DIR on both trees, then diff)' % (name, plan, part)


def test_stored_operand_cases_are_not_vacuous():
    """store_wgrad_operands only bites where rd_conv_honours_src_out accepts a launch (256 x 256): both settings must pin a plan that
    differs from the default's, and option 3 keeps three more tensors in the seg plan."""
    base = GOLDEN['step256.bf16.default']
    for tag in ('store_wgrad_operands=3,store_wgrad_min_c=64', 'store_wgrad_operands=1,store_wgrad_min_c=64'):
        g = GOLDEN['step256.bf16.' + tag]
        assert g['seg']['fwd'] != base['seg']['fwd'] and g['seg']['keep'] != base['seg']['keep'], tag
    d = {tag: CASES['step256.bf16.' + tag]()['seg']['keep'] for tag in ('default', 'store_wgrad_operands=3,store_wgrad_min_c=64')}
    n = {tag: sum(1 for k in keep if k[0] == 'tensor') for tag, keep in d.items()}
    assert n['store_wgrad_operands=3,store_wgrad_min_c=64'] == n['default'] + 3
