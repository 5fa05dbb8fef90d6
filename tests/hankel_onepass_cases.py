"""Cases of the one-pass Hankel tile kernel (csrc/k_hankel.hip) beyond tests/hankel_cases.py, shared by
tests/test_emul_hankel_onepass.py (CPU emulator) and tests/test_gpu_hankel_onepass.py (MI355X): what the fragment-ordered second
copy of the weights (d_Wf), the double-buffered stages of 32 or 64 input shells and the zero padding of both can get wrong.

- stale copy: mtip_set_hankel_weights called twice on one engine; the second transform must use the second table.
- stage and pad edges: Np equal to the stage length of every (CT, SUB) instantiation, one more than it, and 130.
- width independence: an output element's MFMA chain does not depend on the tile width, so the results at CT = 1, 2, 3, 5 are the
  same bits.
- equal to the parent: the same three results as tests/golden/hankel_bits.npz holds them, recorded by
  tests/golden/make_golden_hankel_bits.py with the library of the commit in front of the one-pass kernel.

Reference and bound of the first two are those of hankel_cases (longdouble contraction, a-priori bound per element)."""
import os

import numpy as np

import hankel_cases as HC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hankel_bits.npz')

# ---------------------------------------------------------------------------------------------- stale copy
STALE = [(18, 2, 2, 'midpoint'), (18, 2, 2, 'trapz')]          # Np = 18 and 17: multiples of neither 4 nor 16 (trapz), one tile


def check_stale_copy(lib_path, N, L, B, mode):
    """a random table, a transform, a DIFFERENT random table, a transform: the second result against the second table"""
    first, second = HC.Problem(N, L, B, mode, 31), HC.Problem(N, L, B, mode, 32)
    assert first.W.shape == second.W.shape and not np.array_equal(first.W, second.W)
    e = HC.random_table_engine(first, lib_path)
    try:
        worst = {'first': first.compare(e.hankel(first.x, False), False, None, 'first table')}
        e._ck(e.lib.mtip_set_hankel_weights(e.ctx, HC._lib.ptr(second.W), HC.FWD_SCALE, HC.INV_SCALE))
        for inverse in (False, True):
            d = 'inv' if inverse else 'fwd'
            worst[d] = second.compare(e.hankel(second.x, inverse), inverse, None, 'second table ' + d)
            got = e.hankel_difference(second.x, second.s, inverse, None)
            worst[d + '_diff'] = second.compare(got, inverse, np.ones(B, bool), 'second table diff ' + d)
    finally:
        e.close()
    HC.report('stale N%d L%d B%d %s' % (N, L, B, mode), **worst)


# ---------------------------------------------------------------------------------------------- stage and pad edges
def stage_length(ct, sub):
    """input shells per stage of k_hankel_tile<ct, sub>"""
    return 64 if ct == 1 else 32


def edge_sizes(ct):
    """N (= Np, midpoint) at the stage length of the plain and of the difference kernel of this width and one more than it, and
    130: beyond the padding of d_Wf (to 64 input shells), a last stage of two shells and a second row block with two valid rows"""
    sizes = {130}
    for sub in (False, True):
        st = stage_length(ct, sub)
        sizes |= {st, st + 1}
    return sorted(sizes)


EDGE_L = 2
EDGES = [(N, B, ct) for ct in (1, 2, 3, 5) for N in edge_sizes(ct) for B in (1, 3)]


def edge_id(c):
    return 'N%d-B%d-ct%d' % c


def edge_masks(B):
    """all-on, all-off and (from two restarts on) a mixed mask"""
    return [np.ones(B, bool), np.zeros(B, bool)] + ([np.arange(B) % 2 == 0] if B > 1 else [])


def check_edge(lib_path, N, B, ct):
    """plain and difference variant, both directions, at the forced width ct (the caller has set MTIP_HANKEL_CT)"""
    HC.check_random_tables(lib_path, N, EDGE_L, B, 'midpoint', ct, None, diff_masks=edge_masks(B))


def run_guarded(lib_path):
    """main of the child process of test_emul_hankel_onepass.test_edges_no_access_past_buffer_ends: the edge list on the emulator
    with MTIP_EMUL_GUARD=1, every device buffer followed by an inaccessible page.  A read past d_Wf or past the panel ends the
    process."""
    assert os.environ.get('MTIP_EMUL_GUARD') == '1'
    for N, B, ct in EDGES:
        os.environ['MTIP_HANKEL_CT'] = str(ct)
        check_edge(lib_path, N, B, ct)


# ---------------------------------------------------------------------------------------------- the same bits
BITS = (32, 4, 3, 'midpoint')                  # N, L, B, mode
BITS_SEED = 1618
BITS_MASK = (True, False, True)
BITS_KEYS = ('fwd', 'inv', 'diff')


def bits_results(lib_path, ct):
    """forward, inverse and (inverse, mixed mask) difference transform of the seeded problem at the width ct (the caller has set
    MTIP_HANKEL_CT), as a dict over BITS_KEYS"""
    p = HC.problem(*BITS, seed=BITS_SEED)
    e = HC.random_table_engine(p, lib_path)
    try:
        HC.assert_plan(e, ct)
        return {'fwd': e.hankel(p.x, False), 'inv': e.hankel(p.x, True),
                'diff': e.hankel_difference(p.x, p.s, True, np.array(BITS_MASK))}
    finally:
        e.close()


def check_bits_within_bound(res):
    """the three results are transforms at all (the bit comparisons alone would pass on equal garbage)"""
    p = HC.problem(*BITS, seed=BITS_SEED)
    return {'fwd': p.compare(res['fwd'], False, None, 'fwd'), 'inv': p.compare(res['inv'], True, None, 'inv'),
            'diff': p.compare(res['diff'], True, np.array(BITS_MASK), 'diff')}


def check_bits(results_by_width, prefix):
    """results_by_width: {ct: bits_results(...)} for ct = 1, 2, 3, 5.  All widths the same bits, and the bits of the parent commit's
    kernel as tests/golden/hankel_bits.npz holds them under prefix_* ('emul' or 'gpu': hardware MFMA rounding need not be the
    emulator's)"""
    assert sorted(results_by_width) == [1, 2, 3, 5]
    worst = check_bits_within_bound(results_by_width[1])
    g = np.load(GOLDEN)
    for key in BITS_KEYS:
        for ct in (2, 3, 5):
            assert np.array_equal(results_by_width[ct][key], results_by_width[1][key]), (key, ct)
        gold = g['%s_%s' % (prefix, key)]
        same = np.array_equal(results_by_width[1][key], gold)
        if not same:
            d = np.abs(results_by_width[1][key] - gold)
            raise AssertionError('%s differs from the parent commit %s in %d of %d elements, by at most %.3g' % (
                key, str(g['parent_commit']), int((d > 0).sum()), d.size, float(d.max())))
    HC.report('bits %s N%d L%d B%d' % ((prefix,) + BITS[:3]), **worst)
