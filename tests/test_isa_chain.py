"""Static check of the Legendre synthesis and the table staging of the three k_sht_chain instantiations the benchmark runs
(store + |.|^2, modulus, real-space update at 128 shells x L 32), on the gfx950 listing (scripts/isa_census.py).

The conditions are the description in xframe_amd/csrc/k_sht_legendre.h: between the staging barrier and the barrier in front of
the FFT passes the kernel touches no global memory, the double step of the recurrence is its 14 FP64 operations and 6 LDS reads
next to one running address, the loop control and counted waits, and every staging load of a thread is in flight before the
first is waited for.  They name what the loop should contain, not tuned numbers.  No GPU needed: hipcc cross-compiles.  One
compilation (about a minute) is shared by the tests of this file."""
import os
import shutil
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import isa_census  # noqa: E402

SRC = os.path.join(ROOT, 'xframe_amd', 'csrc', 'k_sht_chain.hip')
# k_sht_chain<EPI, PRE, 8, 16, 3, 16, false, 32, true>: EPI_STORE = 0 with the |.|^2 prologue, EPI_MODULUS = 1, EPI_REAL_UPDATE = 4
KINDS = {'store': 'k_sht_chain<0, 1, 8, 16, 3, 16, false, 32, true>',
         'modulus': 'k_sht_chain<1, 0, 8, 16, 3, 16, false, 32, true>',
         'real': 'k_sht_chain<4, 0, 8, 16, 3, 16, false, 32, true>'}
FP64_PER_DOUBLE_STEP = 14           # two recurrence values (3 each), eight accumulations
# 14 FP64 + 6 LDS reads + 3 address updates + 3 for counter and branch + at most 6 waits
MAX_PER_DOUBLE_STEP = 32
BEFORE_PER_DOUBLE_STEP = 50


def _hipcc():
    hipcc, _ = isa_census.makefile_flags()
    return hipcc if os.path.exists(hipcc) else shutil.which('hipcc')


@pytest.fixture(scope='module')
def kernels():
    if _hipcc() is None:
        pytest.skip('hipcc not found')
    found = isa_census.census(SRC)
    out = {}
    for kind, name in KINDS.items():
        ks = [k for k in found if name in k.name]
        assert len(ks) == 1, (kind, [k.name for k in found])
        out[kind] = ks[0]
    return out


def _synthesis_loop(kernel):
    """the innermost loop with 16-byte LDS reads whose FP64 count is a whole number of double steps and nothing but them"""
    loops = kernel.loops
    cands = []
    for lp in loops:
        inner = not any(o is not lp and o.first_line >= lp.first_line and o.last_line <= lp.last_line and
                        (o.first_line, o.last_line) != (lp.first_line, lp.last_line) for o in loops)
        fp64 = lp.counts.get('fp64', 0)
        reads = lp.detail.get('ds_read_b128', 0)
        if inner and reads > 0 and fp64 > 0 and fp64 % FP64_PER_DOUBLE_STEP == 0 and reads * FP64_PER_DOUBLE_STEP == 6 * fp64:
            cands.append(lp)
    assert len(cands) == 1, [(lp.label, lp.total, dict(lp.counts)) for lp in cands]
    return cands[0]


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_synthesis_loop_is_fp64_and_lds_work(kernels, kind):
    lp = _synthesis_loop(kernels[kind])
    c, d = lp.counts, lp.detail
    steps = c['fp64'] // FP64_PER_DOUBLE_STEP
    print('%s %s lines %d-%d: %d instructions for %d double steps %s %s' % (kind, lp.label, lp.first_line, lp.last_line, lp.total,
                                                                           steps, dict(c), dict(d)))
    assert c.get('memory', 0) == 0 and d.get('flat', 0) == 0 and d.get('global', 0) == 0, 'global or flat access in the loop'
    assert d.get('vmcnt', 0) == 0, 'a wait for global memory in the loop'
    assert c.get('saveexec', 0) == 0, 'EXEC-mask region in the loop'
    assert d.get('v_mov_b64', 0) == 0, 'register copies of the operand sets'
    assert d.get('scratch', 0) == 0
    assert c.get('waitcnt', 0) <= 6 * steps
    assert lp.total <= MAX_PER_DOUBLE_STEP * steps < BEFORE_PER_DOUBLE_STEP * steps


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_no_global_memory_around_the_synthesis(kernels, kind):
    """the loop over the wave's items (every loop that holds the synthesis loop) touches no global memory either: start values
    and cos(theta) were requested at kernel entry"""
    k = kernels[kind]
    syn = _synthesis_loop(k)
    outer = [lp for lp in k.loops if lp.first_line <= syn.first_line and lp.last_line >= syn.last_line and lp is not syn and
             not lp.detail.get('endpgm', 0)]                # (a span over the kernel's end is a block placed out of line, no loop)
    assert outer, 'no item loop around the synthesis loop'
    for lp in outer:
        print('%s item loop %s lines %d-%d: %s %s' % (kind, lp.label, lp.first_line, lp.last_line, dict(lp.counts), dict(lp.detail)))
        assert lp.counts.get('memory', 0) == 0 and lp.detail.get('vmcnt', 0) == 0


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_staging_is_not_a_loop_of_round_trips(kernels, kind):
    """no back-branch span up to the synthesis holds a global load, a full vmcnt wait and an LDS store together"""
    k = kernels[kind]
    syn = _synthesis_loop(k)
    for lp in k.loops:
        if lp.first_line <= syn.first_line and not lp.detail.get('endpgm', 0):      # (out-of-line blocks are no loops)
            d = lp.detail
            assert not (d.get('global_load', 0) and d.get('vmcnt0', 0) and d.get('lds_store', 0)), (lp.label, dict(d))
    assert 0 < k.vgprs <= 256 and k.scratch == 0
