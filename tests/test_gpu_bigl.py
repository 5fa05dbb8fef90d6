"""Band limits 64 <= L <= 128 on the MI355X (csrc/k_sht_big.h): the cases of tests/bigl_cases.py -- every transform operator against the
oracle at the shapes that reach a tail, a grid size or the limit, the generic kernels (MTIP_SHT_TIER=0) as the second implementation,
simulate_ccd beyond L = 63 against the same flow composed from the oracle, and what raises."""
import os
import subprocess
import sys

import pytest

import bigl_cases as BC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('shape', BC.SHAPES + (BC.SHAPE_WIDE, BC.ODD_SHAPE, BC.TALL_SHAPE), ids=str)
def test_operators_vs_oracle(monkeypatch, shape):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)
    BC.check_operators(shape)


def test_fallback_tier0():
    code = 'import sys; sys.path[:0] = [%r, %r]; import bigl_cases as BC; BC.run_fallback()' % (HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_SHT_TIER='0'), capture_output=True, text=True)
    assert r.returncode == 0 and 'BIGL fallback ok' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize('settings,through_extract', [(BC.FLOW64, True), (BC.FLOW128, False)], ids=['L64', 'L128'])
def test_flow(monkeypatch, settings, through_extract):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)
    BC.check_flow(settings, None, through_extract)


def test_raises():
    BC.check_raises()
