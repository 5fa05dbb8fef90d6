"""Static check of the Jacobi round of k_rproj: what the compiler makes of rp_sweep_pad<NC, 16>, NC = 1..5.

The round is bound by the number of instructions a wave issues between two barriers, and DESIGN section 3
describes it as branch-free apart from the resident reload and the write-back, with every operand in registers or LDS.  The
conditions below are that description, checked on the gfx950 listing (scripts/isa_census.py); they are not tuned numbers.
No GPU needed: hipcc cross-compiles.  One compilation (about 20 s) is shared by the tests of this file."""
import os
import shutil
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import isa_census  # noqa: E402

SRC = os.path.join(ROOT, 'xframe_amd', 'csrc', 'k_projr.hip')
KERNEL = 'k_rproj<512, 2, 4, false, 16>'
FP64_OF_NC = {1: 55, 2: 66, 3: 77, 4: 88, 5: 99}          # 44 + 11 per row slot: 3 Gram FMAs, 8 operations of the rotations
ROUND_BEFORE_NC5 = 224                                    # instructions of the NC = 5 round before the round was cleared out


def _hipcc():
    hipcc, _ = isa_census.makefile_flags()
    return hipcc if os.path.exists(hipcc) else shutil.which('hipcc')


@pytest.fixture(scope='module')
def round_loops():
    """{NC: [Loop, ...]} of the production instance: every back-branch span with one barrier and the FP64 count of NC row
    slots (a round has two: with and without the write-back block behind the branch), the instance with timers left out."""
    if _hipcc() is None:
        pytest.skip('hipcc not found')
    kernels = [k for k in isa_census.census(SRC) if KERNEL in k.name]
    assert len(kernels) == 1, [k.name for k in isa_census.census(SRC)]
    out = {}
    for nc, fp64 in FP64_OF_NC.items():
        out[nc] = [lp for lp in kernels[0].loops
                   if lp.barriers == 1 and lp.counts.get('fp64', 0) == fp64 and lp.detail.get('clock', 0) == 0]
    return kernels[0], out


@pytest.mark.parametrize('nc', sorted(FP64_OF_NC))
def test_round_is_clear_of_compiler_leftovers(round_loops, nc):
    _, loops = round_loops
    assert loops[nc], 'no round loop with %d FP64 instructions and one barrier' % FP64_OF_NC[nc]
    labels = {lp.label for lp in loops[nc]}
    assert len(labels) == 1, 'more than one loop looks like the NC = %d round: %s' % (nc, sorted(labels))
    for lp in loops[nc]:
        c, d = lp.counts, lp.detail
        print('NC %d %s lines %d-%d: %d instructions %s %s' % (nc, lp.label, lp.first_line, lp.last_line, lp.total, dict(c), dict(d)))
        assert c.get('readlane', 0) == 0 and c.get('writelane', 0) == 0, 'SGPR spill traffic in the round'
        assert d.get('scratch', 0) == 0, 'scratch access in the round'
        assert d.get('flat', 0) == 0, 'flat access in the round: the operands are in LDS'
        assert c.get('saveexec', 0) <= 2, 'exec-mask regions beyond the resident reload and the write-back'
        assert d.get('v_mov_b64', 0) <= 1, 'loop-carried register copies'


def test_round_of_five_row_slots_is_shorter(round_loops):
    _, loops = round_loops
    longest = max(lp.total for lp in loops[5])
    print('NC 5 round: %d instructions on the path with the write-back (%d before)' % (longest, ROUND_BEFORE_NC5))
    assert longest < ROUND_BEFORE_NC5


def test_census_reads_the_kernel_figures(round_loops):
    kernel, _ = round_loops
    assert 0 < kernel.vgprs <= 256 and kernel.sgprs > 0 and kernel.scratch >= 0
