"""CPU pre-flight of the one-pass Hankel tile kernel (csrc/k_hankel.hip) through the cases of tests/hankel_onepass_cases.py: the
unchanged kernel source on the CPU emulator -- a second call of mtip_set_hankel_weights, Np at and just beyond the stage length of
every (CT, SUB) instantiation (once more in a child whose device buffers end at inaccessible pages), the same bits at every tile
width and the bits of the parent commit's kernel (tests/golden/hankel_bits.npz, keys emul_*)."""
import os
import subprocess
import sys

import pytest

import hankel_onepass_cases as OC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('N,L,B,mode', OC.STALE, ids=[c[3] for c in OC.STALE])
def test_second_table_replaces_the_first(emul_lib, monkeypatch, N, L, B, mode):
    monkeypatch.delenv('MTIP_HANKEL_CT', raising=False)
    OC.check_stale_copy(emul_lib, N, L, B, mode)


@pytest.mark.parametrize('N,B,ct', OC.EDGES, ids=list(map(OC.edge_id, OC.EDGES)))
def test_stage_and_pad_edges(emul_lib, monkeypatch, N, B, ct):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    OC.check_edge(emul_lib, N, B, ct)


def test_edges_no_access_past_buffer_ends(emul_lib):
    """in a child process (a stray access ends it): the edge list with every device allocation of the emulator followed by an
    inaccessible page"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import hankel_onepass_cases as OC; OC.run_guarded(%r)' % (
        HERE, os.path.dirname(HERE), emul_lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_EMUL_GUARD='1'), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count('HANKEL') == len(OC.EDGES), r.stdout


def test_same_bits_at_every_width_and_as_the_parent(emul_lib, monkeypatch):
    by_width = {}
    for ct in (1, 2, 3, 5):
        monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
        by_width[ct] = OC.bits_results(emul_lib, ct)
    OC.check_bits(by_width, 'emul')
