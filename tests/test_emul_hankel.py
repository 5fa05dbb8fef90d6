"""CPU pre-flight of the Hankel tile kernel (csrc/k_hankel.hip): the unchanged kernel source on the CPU emulator through the cases
of tests/hankel_cases.py -- every width CT in {1, 2, 3, 5} forced with MTIP_HANKEL_CT (the emulator's two "CUs" would plan CT = 5
almost everywhere), plain and difference variant, against a longdouble contraction of a random weight table within an a-priori
bound per output element.  The shapes are the smallest that leave each first tile (hankel_cases.CASES); 128 x L32 with 8 restarts
and 256 x L48 run on the MI355X only (tests/test_gpu_hankel.py): they reach no path that these do not."""
import os
import subprocess
import sys

import pytest

import hankel_cases as HC
import parity_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')
EMUL_N_CU = 2                                   # what the emulator's hipDeviceGetAttribute reports


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('N,L,B,mode,ct,mixed', HC.expand(HC.CASES), ids=list(map(HC.case_id, HC.expand(HC.CASES))))
def test_random_tables(emul_lib, monkeypatch, N, L, B, mode, ct, mixed):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    HC.check_random_tables(emul_lib, N, L, B, mode, ct, mixed)


@pytest.mark.parametrize('N,L,B,mode,ct,mixed', HC.expand(HC.REAL_TABLE_CASES), ids=list(map(HC.case_id, HC.expand(HC.REAL_TABLE_CASES))))
def test_real_tables_vs_oracle(emul_lib, monkeypatch, N, L, B, mode, ct, mixed):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    HC.check_real_tables(emul_lib, N, L, B, mode, ct)


def test_no_access_past_buffer_ends(emul_lib):
    """in a child process (a stray access ends it): the cases that touch the ends of the buffers, every device allocation of the
    emulator followed by an inaccessible page"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import hankel_cases as HC; HC.run_guarded(%r)' % (HERE, os.path.dirname(HERE), emul_lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_EMUL_GUARD='1'), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count('HANKEL') == sum(len(w) for _, w in HC.GUARDED), r.stdout


def test_difference_arguments(emul_lib):
    HC.check_difference_arguments(emul_lib)


def test_plan_rule_restated():
    HC.check_plan_rule_at_256_cus()


@pytest.mark.parametrize('N,L,B', [(16, 9, 5), (130, 5, 3), (10, 3, 2)])
def test_plan_unforced(emul_lib, monkeypatch, N, L, B):
    monkeypatch.delenv('MTIP_HANKEL_CT', raising=False)
    HC.check_plan(emul_lib, N, L, B, EMUL_N_CU)


# ---- the loop under every width: the fused single steps of the reference and the mixed per-restart ft_stab mask
@pytest.mark.parametrize('ct', [1, 2, 3, 5])
def test_single_steps_golden_hankel_width(emul_lib, golden_mtip16, monkeypatch, ct):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    PC.check_steps_golden(golden_mtip16, emul_lib, True, hankel_ct=ct)


@pytest.mark.parametrize('ct', [1, 2, 3, 5])
def test_ft_stab_disagreement_hankel_width(emul_lib, golden_mtip16, monkeypatch, ct):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    PC.check_ft_stab_disagreement(golden_mtip16, emul_lib, hankel_ct=ct)
