"""The Hankel tile kernel on the MI355X (csrc/k_hankel.hip) through the cases of tests/hankel_cases.py: the shapes of
tests/test_emul_hankel.py at every forced width CT in {1, 2, 3, 5}, plain and difference variant, and unforced 128 x L32 with 8
restarts (the benchmark's plan: the getter must say CT = 5) and 256 x L48 with 2 restarts (two row blocks, CT = 5) -- against a
longdouble contraction of a random weight table, every output element within its a-priori bound (hankel_cases).  The plan rule
is restated in Python and compared with the getter at the device's CU count.  DESIGN section 1 has the measured error / bound."""
import numpy as np
import pytest

import hankel_cases as HC
import parity_cases as PC

pytestmark = pytest.mark.gpu

RANDOM = HC.expand(HC.CASES)
REAL = HC.expand(HC.REAL_TABLE_CASES)


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize('N,L,B,mode,ct,mixed', RANDOM, ids=list(map(HC.case_id, RANDOM)))
def test_random_tables(monkeypatch, N, L, B, mode, ct, mixed):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    HC.check_random_tables(None, N, L, B, mode, ct, mixed)


@pytest.mark.parametrize('N,L,B,mixed', [(128, 32, 8, '10010110'), (256, 48, 2, None)])
def test_random_tables_unforced(monkeypatch, N, L, B, mixed):
    """the plan the device itself makes: at 256 CUs CT = 5 at both sizes, 231 workgroups at the benchmark's.  256 x L48 runs the
    plain transform only: the difference variant meets a second row block at (130, 5, 3) already, and the longdouble contraction
    of a second coefficient set at this size would double the test's host time"""
    monkeypatch.delenv('MTIP_HANKEL_CT', raising=False)
    n_cu = device_cus()
    if n_cu == 256:
        assert HC.plan_rule(N, L, B, n_cu)[0] == 5
    HC.check_random_tables(None, N, L, B, 'midpoint', None, mixed, n_cu=n_cu,
                           diff_masks=[None, np.array([ch == '1' for ch in mixed])] if mixed else [])


@pytest.mark.parametrize('N,L,B,mode,ct,mixed', REAL, ids=list(map(HC.case_id, REAL)))
def test_real_tables_vs_oracle(monkeypatch, N, L, B, mode, ct, mixed):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    HC.check_real_tables(None, N, L, B, mode, ct)


def test_difference_arguments():
    HC.check_difference_arguments(None)


@pytest.mark.parametrize('N,L,B,ct256', HC.PLAN_SHAPES)
def test_plan_rule(monkeypatch, N, L, B, ct256):
    monkeypatch.delenv('MTIP_HANKEL_CT', raising=False)
    HC.check_plan_rule_at_256_cus()
    n_cu = device_cus()
    HC.check_plan(None, N, L, B, n_cu, expect_ct=ct256 if n_cu == 256 else None)
