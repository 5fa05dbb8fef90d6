"""The one-pass Hankel tile kernel on the MI355X (csrc/k_hankel.hip) through the cases of tests/hankel_onepass_cases.py: a second
call of mtip_set_hankel_weights, Np at and just beyond the stage length of every (CT, SUB) instantiation, the same bits at every
tile width and the bits the parent commit's kernel gave on the MI355X (tests/golden/hankel_bits.npz, keys gpu_*)."""
import pytest

import hankel_onepass_cases as OC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('N,L,B,mode', OC.STALE, ids=[c[3] for c in OC.STALE])
def test_second_table_replaces_the_first(monkeypatch, N, L, B, mode):
    monkeypatch.delenv('MTIP_HANKEL_CT', raising=False)
    OC.check_stale_copy(None, N, L, B, mode)


@pytest.mark.parametrize('N,B,ct', OC.EDGES, ids=list(map(OC.edge_id, OC.EDGES)))
def test_stage_and_pad_edges(monkeypatch, N, B, ct):
    monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
    OC.check_edge(None, N, B, ct)


def test_same_bits_at_every_width_and_as_the_parent(monkeypatch):
    by_width = {}
    for ct in (1, 2, 3, 5):
        monkeypatch.setenv('MTIP_HANKEL_CT', str(ct))
        by_width[ct] = OC.bits_results(None, ct)
    OC.check_bits(by_width, 'gpu')
