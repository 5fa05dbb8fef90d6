"""CPU side of tests/sht_plan_cases.py, on the emulator build of the unchanged kernel sources: the census -- the plan keys of
L = 1..63 on their default grids are exactly those with a representative, every representative and every capped entry has the key it
stands for --, the transforms of every representative, the short schedule against the oracle at L = 20, 28 and 49, and one run of it
with every device allocation ending at an inaccessible page."""
import os
import subprocess
import sys

import pytest

import sht_plan_cases as SP

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(autouse=True)
def default_tiers(monkeypatch):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)


def test_census(emul_lib):
    SP.check_census(emul_lib)


def test_tables_are_consistent():
    assert set(SP.EMUL_LOOP_CASES) <= set(SP.CASES) and SP.GUARDED_CASE in SP.CASES
    assert len(set(SP.CASES)) == len(SP.CASES)
    for key in list(SP.REPRESENTATIVES) + list(SP.CAPPED.values()):
        assert len(key) == len(SP.KEY_FIELDS)
    for _, test in SP.COVERED_ELSEWHERE.values():
        path, name = test.split('::')
        assert 'def %s(' % name in open(os.path.join(HERE, path)).read(), test
    for (cap, shape), key in SP.CAPPED_LOOP.items():
        assert SP.CAPPED_TRANSFORMS.get((cap, shape), key) == key


@pytest.mark.parametrize('shape', SP.CASES, ids=SP.case_id)
def test_transforms(emul_lib, shape):
    SP.check_transforms(shape, emul_lib)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
@pytest.mark.parametrize('shape', SP.EMUL_LOOP_CASES, ids=SP.case_id)
def test_loop_vs_oracle(emul_lib, shape, fused):
    SP.check_loop(shape, emul_lib, fused)


def test_no_access_past_buffer_ends(emul_lib):
    code = 'import sys; sys.path[:0] = [%r, %r]; import sht_plan_cases as SP; SP.run_guarded(%r)' % (HERE, os.path.dirname(HERE), emul_lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_EMUL_GUARD='1'), capture_output=True, text=True)
    assert r.returncode == 0 and 'SHT plan guarded ok' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
