"""Static check of the FFT passes (the row-group loop) and of the Legendre sums behind them in the three k_sht_chain
instantiations the benchmark runs (store + |.|^2, modulus, real-space update at 128 shells x L 32), on the gfx950 listing
(scripts/isa_census.py), next to tests/test_isa_chain.py, which holds the synthesis in front of them.  No GPU needed: hipcc
cross-compiles.  One compilation (about a minute) is shared by the tests of this file.

The kernels are bound by the number of instructions a wave issues, so the tests name what the code should contain:

- The row-group loop (one iteration = the four FFT steps of one group of 4 rows; a wave runs 2) is the barrier-free loop with
  the largest FP64 count.  A loop has one header and, where the compiler places a block of the body behind the first
  back-branch, several back-branches: the WHOLE body is the widest span of the header, and that is what is counted here.  Its
  FP64 and LDS counts are those of the commit in front of this test (390 / 86, 627 / 101, 520 / 102 over the whole body; that
  commit's FIRST back-branch spans 386 / 85, 623 / 100, 516 / 101, four FP64 and one LDS store less, because its compiler put the
  tail of the last conditional panel store behind it): the arithmetic did not move.
- EXEC-mask regions (s_and_saveexec / s_andn2_saveexec) in that loop: 36 / 45 / 37 before.  The row guards, the conditional
  panel stores and (modulus) the conditional square root are gone; what is left is 31 in every variant, from two source
  constructs that are no guard and no conditional store:
    * half_fft (k_sht_common.h): the two halves of a 16-point transform are lanes 0-31 and 32-63 of the wave and do different
      arithmetic (a + b against (a - b) w), chosen per output by `if (half == 0)`.  The compiler merges neighbouring outputs
      into 4 regions in the inverse and 6 in the forward transform, each an s_and_saveexec and two s_andn2_saveexec: 30.
      Without the regions both halves would be computed by every lane, which is more FP64, not less.  (One if / else around
      the whole radix-2 stage leaves 4 of the 30 and takes ~95 instructions off a row group, but the compiler then contracts
      other products of the twiddle multiplications into FMAs and the MI355X results differ from the parent's in the last
      bits -- measured, tests/golden/chain_bits.npz -- so it is not in this kernel.)
    * step 1's read of spectrum entry k = k1 + 32, in the band for k1 = 0 alone: written as a clamped read and a select, compiled
      to a read under the lane mask (one s_and_saveexec, no branch).
  The count is pinned at 31.
- The block from the end of that loop to the closing barrier (the barrier behind the groups' partial sums) is the Legendre-sum
  phase: its 192 FMA and 32 16-byte LDS reads, at most 24 table loads of 16 bytes each, no 64-bit multiply-add, no integer
  division, no vector multiply, and at most 300 instructions in all (507 before).  The real-space variant reduces its error
  sums between the same two barriers: their 12 additions and at most 79 instructions come on top there (ERROR_SUM_* below).
- Behind that block there is no loop (before: three reduction loops, unrolled by four with remainder loops, for two groups)."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import isa_census  # noqa: E402

SRC = os.path.join(ROOT, 'xframe_amd', 'csrc', 'k_sht_chain.hip')
KINDS = {'store': 'k_sht_chain<0, 1, 8, 16, 3, 16, false, 32, true>',
         'modulus': 'k_sht_chain<1, 0, 8, 16, 3, 16, false, 32, true>',
         'real': 'k_sht_chain<4, 0, 8, 16, 3, 16, false, 32, true>'}
# whole body of the row-group loop in the commit in front of this test: (FP64, LDS) and its EXEC-mask regions
PARENT_FP64_LDS = {'store': (390, 86), 'modulus': (627, 101), 'real': (520, 102)}
PARENT_SAVEEXEC = {'store': 36, 'modulus': 45, 'real': 37}
SAVEEXEC_LEFT = 31                  # 10 regions of half_fft x 3 + the masked spectrum read of step 1 (see above)
SUMS_FP64, SUMS_READS, SUMS_LOADS, SUMS_MAX, SUMS_BEFORE = 192, 32, 24, 300, 507
# The real-space variant's error sums (two doubles through six butterfly steps of the wave, then lane 0 stores the pair) sit
# between the same two barriers and are no part of the Legendre sums.  By what they are: a step is the partner lane (xor, the
# width clamp's compare and select, the byte address), four 32-bit lane exchanges, two waits and two additions = 12 instructions;
# the store is compare, EXEC region with its branch and its end, a wait, the address and the write = 7.
ERROR_SUM_FP64, ERROR_SUM_MAX = 12, 6 * 12 + 7


def _hipcc():
    hipcc, _ = isa_census.makefile_flags()
    return hipcc if os.path.exists(hipcc) else shutil.which('hipcc')


@pytest.fixture(scope='module')
def listing():
    if _hipcc() is None:
        pytest.skip('hipcc not found')
    text = isa_census.compile_listing(SRC)
    found = isa_census.census_of_listing(text)
    out = {}
    for kind, name in KINDS.items():
        ks = [k for k in found if name in k.name]
        assert len(ks) == 1, (kind, [k.name for k in found])
        out[kind] = ks[0]
    return text.splitlines(), out


def _row_group_loop(kernel):
    """the barrier-free loop with the largest FP64 count: (header label, its widest span)"""
    free = [lp for lp in kernel.loops if lp.barriers == 0 and not lp.detail.get('endpgm', 0)]
    assert free
    top = max(free, key=lambda lp: lp.counts.get('fp64', 0))
    same = [lp for lp in free if lp.label == top.label]
    whole = max(same, key=lambda lp: lp.last_line)
    assert whole.first_line == top.first_line and whole.counts.get('fp64', 0) == top.counts.get('fp64', 0)
    return whole


def _instructions(lines, first, last):
    """(line number, mnemonic, operands) of the instructions in the listing's lines [first, last] (1-based, inclusive)"""
    out = []
    for ln in range(first, last + 1):
        m = isa_census._INSTR.match(lines[ln - 1])
        if m and not m.group(1).startswith('.') and isa_census.classify(m.group(1), m.group(2) or '') is not None:
            out.append((ln, m.group(1), m.group(2) or ''))
    return out


def _kernel_end(lines, start):
    ln = start
    while not lines[ln - 1].startswith('.Lfunc_end'):
        ln += 1
    return ln


def _sums_block(lines, kernel):
    """the instructions behind the row-group loop up to and including the closing barrier: the second s_barrier behind the loop
    (the first says the panel is complete, the second that the groups' partial sums are in LDS)"""
    lp = _row_group_loop(kernel)
    ins = _instructions(lines, lp.last_line + 1, _kernel_end(lines, lp.last_line))
    bars = [i for i, (_, mn, _o) in enumerate(ins) if mn == 's_barrier']
    assert len(bars) == 2, 'barriers behind the row-group loop: %d' % len(bars)
    return ins[:bars[1] + 1], ins[bars[1] + 1:]


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_row_group_loop_is_the_parents_arithmetic(listing, kind):
    lines, kernels = listing
    lp = _row_group_loop(kernels[kind])
    c, d = lp.counts, lp.detail
    print('%s row-group loop %s lines %d-%d: %d instructions %s %s' % (kind, lp.label, lp.first_line, lp.last_line, lp.total,
                                                                       dict(c), dict(d)))
    assert (c.get('fp64', 0), c.get('lds', 0)) == PARENT_FP64_LDS[kind]
    assert d.get('scratch', 0) == 0


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_row_group_loop_exec_regions(listing, kind):
    _, kernels = listing
    lp = _row_group_loop(kernels[kind])
    n = lp.counts.get('saveexec', 0)
    print('%s row-group loop: %d saveexec (before %d), %d branches' % (kind, n, PARENT_SAVEEXEC[kind], lp.detail.get('branch', 0)))
    assert n <= PARENT_SAVEEXEC[kind]
    assert n == SAVEEXEC_LEFT, 'EXEC-mask regions other than those of half_fft and the masked spectrum read (see the module docstring)'


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_legendre_sums_block(listing, kind):
    lines, kernels = listing
    block, _ = _sums_block(lines, kernels[kind])
    mns = [mn for _, mn, _o in block]
    cls = [isa_census.classify(mn, ops) for _, mn, ops in block]
    fp64 = cls.count('fp64')
    reads = sum(1 for mn in mns if mn.startswith('ds_read_b128'))
    loads = [mn for mn in mns if re.match(r'(global|flat|buffer)_load', mn)]
    print('%s sums block lines %d-%d: %d instructions, %d FP64, %d ds_read_b128, loads %s, %d waits, %d scalar'
          % (kind, block[0][0], block[-1][0], len(block), fp64, reads, sorted(set(loads)), cls.count('waitcnt'), cls.count('scalar')))
    # the real-space variant reduces its per-shell error sums in this block too (err_num, err_den: wave butterflies, lane 0 stores)
    fma = sum(1 for mn in mns if mn.startswith(('v_fma_f64', 'v_fmac_f64')))
    other = ERROR_SUM_FP64 if kind == 'real' else 0
    assert fma == SUMS_FP64 and fp64 == SUMS_FP64 + other and reads == SUMS_READS
    assert 0 < len(loads) <= SUMS_LOADS and all(mn.startswith('global_load_dwordx4') for mn in loads), loads
    for bad in ('v_mad_i64_i32', 'v_mad_u64_u32', 'v_rcp_iflag_f32', 'v_mul_lo_u32'):
        assert not any(mn.startswith(bad) for mn in mns), bad
    assert not any(mn.startswith('scratch_') for mn in mns)
    assert len(block) <= SUMS_MAX + (ERROR_SUM_MAX if kind == 'real' else 0) and SUMS_MAX < SUMS_BEFORE


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_no_loop_behind_the_sums(listing, kind):
    """the closing reduction is one add of the other group's partial sums, not a loop over groups"""
    lines, kernels = listing
    k = kernels[kind]
    block, rest = _sums_block(lines, k)
    first = block[0][0]
    behind = [lp for lp in k.loops if lp.last_line >= first and not lp.detail.get('endpgm', 0)]
    assert not behind, [(lp.label, lp.first_line, lp.last_line) for lp in behind]
    assert 0 < k.vgprs <= 256 and k.scratch == 0
