"""Every SHT plan the default grids reach below L = 64 on the MI355X (tests/sht_plan_cases.py): per representative the transforms
against the oracle and 2 HIO + SW + 2 ER against the oracle's loop, fused and in reference order, at a plan key that is asserted
from the context before anything runs; the kernel families of the fused step; the MTIP_SHT_TIER caps whose kernels are not the
forms of 64 x L16, each in a child process.  The census that ties the representatives to plan_sht runs on the CPU
(tests/test_emul_sht_plan.py)."""
import os
import subprocess
import sys

import pytest

import sht_plan_cases as SP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def default_tiers(monkeypatch):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)


def _child(call, cap, shape):
    code = 'import sys; sys.path[:0] = [%r, %r]; import sht_plan_cases as SP; SP.%s(%d, %r)' % (HERE, os.path.dirname(HERE), call, cap, shape)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_SHT_TIER=str(cap)), capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize('shape', SP.CASES, ids=SP.case_id)
def test_transforms(shape):
    SP.check_transforms(shape, None)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
@pytest.mark.parametrize('shape', SP.CASES, ids=SP.case_id)
def test_loop_vs_oracle(shape, fused):
    SP.check_loop(shape, None, fused)


@pytest.mark.parametrize('cap,shape', sorted(SP.CAPPED_TRANSFORMS), ids=lambda v: SP.case_id(v) if isinstance(v, tuple) else 'cap%d' % v)
def test_capped_transforms(cap, shape):
    assert 'SHT plan capped transforms ok' in _child('run_capped_transforms', cap, shape)


@pytest.mark.parametrize('cap,shape', sorted(SP.CAPPED_LOOP), ids=lambda v: SP.case_id(v) if isinstance(v, tuple) else 'cap%d' % v)
def test_capped_loop_vs_oracle(cap, shape):
    assert 'SHT plan capped loop ok' in _child('run_capped_loop', cap, shape)
