"""Cases of the Hankel tile kernel (csrc/k_hankel.hip: k_hankel_tile<CT, SUB>, its launcher launch_hankel_mfma_sub and the plan of
build_hankel_tiles) at operator level, shared by tests/test_emul_hankel.py (CPU emulator) and tests/test_gpu_hankel.py (MI355X).

The width CT in {1, 2, 3, 5} is forced by the drivers with MTIP_HANKEL_CT before the engine is made; every case asserts through
mtip_debug_hankel_tiles that the width it means is the planned one (and the tile and row-block counts with it).

Inputs of the main cases: a seeded random weight table W ~ N(0, 1) of shape (L+1, Np, N), uploaded with mtip_set_hankel_weights in
place of the engine's Bessel table, with the scales FWD_SCALE / INV_SCALE; complex normal coefficients x and subtracted set s.  With
such a table every (l, p, k) term weighs the same: a dropped, doubled or shifted term is an error of order 1 / sqrt(Np) in its row,
where the Bessel weights j_l(q r) hide most single terms of the high orders below 1e-12.

Reference: a numpy.longdouble contraction of the very table handed to the device,
    H(x)[b, k, lm] = c_l sum_p W[l][p][k] x[b, p + poffs, lm],   c_l = scale (-/+ i)^l  (forward / inverse),
and for the difference variant (mtip_op_hankel_difference, SUB = true) of a restart whose mask byte is set
    out[b, k] = H(x)[b, k] - H(s)[b, k] above shell 0,  H(x)[b, 0] on shell 0;   out[b] = H(x)[b] for a restart whose byte is 0.
Bound, a priori (the dot-product bound of n terms holds for any summation order and for FMA), for EVERY output element, real and
imaginary part apart:
    |got - ref| <= (n + 4) 2^-52 |scale| sum_p |W[l][p][k]| (|x_p| + |s_p|)
with n = Np, s = 0 where nothing is subtracted, and n = 2 Np on output shell 0 of a subtracting restart (two MFMA chains: H(x - s)
and the row-0 correction H(s)).  The + 4 covers the rounding of x - s, the scale multiply and the reference's own rounding
(longdouble: eps < 1e-18 is asserted).  Nothing in the bound is measured.  Every case prints its worst error / bound on a line that
starts with 'HANKEL'; DESIGN section 1 has the table."""
import functools

import numpy as np

import parity_cases as PC
from helpers import rel_l2
from xframe_amd.fxs import _lib
from xframe_amd.fxs.engine import Engine

LD = np.longdouble
FWD_SCALE, INV_SCALE = 0.37, 2.9
WIDTHS = (5, 3, 2, 1)
ROWS = 128                                     # output shells per row block (HT_ROWS)

# (N, L, B, mode, widths, mixed mask): the smallest shapes that leave each first tile; all run the difference variant too
LADDER = [(N, 3, 2, 'midpoint', (1, 2, 3, 5), '10') for N in (10, 20, 40, 50, 70)]   # n_chunks = 1 .. 5, l mod 4 = 0 .. 3
ROW_BLOCK = (130, 5, 3, 'midpoint', (1, 5), '101')         # k_base = 128; 9 chunks, the last of 2 shells
TRAPZ = (34, 4, 2, 'trapz', (2, 3), '10')                  # Np = 33: the third chunk holds one shell; poffs = 1
FEW_COLUMNS = (16, 6, 1, 'midpoint', (1, 5), '1')          # l = 0 has 2 columns
STRADDLE = (16, 9, 5, 'midpoint', (1, 2, 3, 5), '10010')   # an 80-column tile of l = 0, 1, 2 spans restarts with different bytes
CASES = LADDER + [ROW_BLOCK, TRAPZ, FEW_COLUMNS, STRADDLE]
REAL_TABLE_CASES = [ROW_BLOCK, TRAPZ]
PLAN_SHAPES = [(128, 32, 2, 1), (128, 32, 3, 2), (128, 32, 5, 3), (128, 32, 8, 5), (256, 48, 1, 3), (256, 48, 2, 5)]   # (N, L, B, CT at 256 CUs)


def expand(cases):
    """(N, L, B, mode, ct, mixed) per width"""
    return [(N, L, B, mode, ct, mixed) for N, L, B, mode, widths, mixed in cases for ct in widths]


def case_id(c):
    return 'N%d-L%d-B%d-%s-ct%s' % tuple(c[:5])


def report(case, **figures):
    print('HANKEL %-34s %s' % (case, '  '.join('%s=%.3g' % kv for kv in figures.items())), flush=True)


# ---------------------------------------------------------------------------------------------- the plan rule, restated
def n_tiles(L, B, ct):
    """column tiles of width 16 ct, counted per order: a tile never spans two orders"""
    return sum(-(-B * (4 * l + 2) // (16 * ct)) for l in range(L + 1))


def n_row_blocks(N):
    return -(-N // ROWS)


def plan_rule(N, L, B, n_cu):
    """the widest of 5, 3, 2, 1 whose workgroup count x 5 reaches 4 n_cu, else 1"""
    for ct in WIDTHS:
        if n_tiles(L, B, ct) * n_row_blocks(N) * 5 >= 4 * n_cu:
            return ct, n_tiles(L, B, ct)
    return 1, n_tiles(L, B, 1)


def assert_plan(e, ct):
    plan = e.hankel_tiles()
    assert plan == (ct, n_tiles(e.L, e.B, ct), n_row_blocks(e.N)), (plan, ct)
    return plan


def check_plan_rule_at_256_cus():
    """the restated rule at the MI355X's 256 CUs: widths 1, 2, 3, 5 at 2, 3, 5, 8 restarts of 128 x L32 and 3, 5 at 1, 2 restarts of
    256 x L48; 231 workgroups at 8 restarts (the benchmark)"""
    for N, L, B, ct in PLAN_SHAPES:
        assert plan_rule(N, L, B, 256)[0] == ct, (N, L, B)
    assert plan_rule(128, 32, 8, 256) == (5, 231)


def check_plan(lib_path, N, L, B, n_cu, expect_ct=None):
    """the getter's plan of an unforced engine against the restated rule at the device's CU count"""
    e = Engine({'grid': {'n_radial_points': N, 'max_order': L}}, None, n_batch=B, lib_path=lib_path, max_q=1.0)
    plan = e.hankel_tiles()
    e.close()
    ct, nt = plan_rule(N, L, B, n_cu)
    report('plan N%d L%d B%d n_cu=%d' % (N, L, B, n_cu), ct=plan[0], n_tiles=plan[1], n_row_blocks=plan[2])
    assert plan == (ct, nt, n_row_blocks(N)), (plan, ct, nt)
    if expect_ct is not None:
        assert ct == expect_ct, (ct, expect_ct)


# ---------------------------------------------------------------------------------------------- inputs and reference
def _rot(re, im, r):
    """(re + i im) i^r"""
    return ((re, im), (-im, re), (-re, -im), (im, -re))[r]


class Problem:
    """seeded table, coefficients and subtracted set at (N, L, B, mode), and the longdouble contractions of both"""

    def __init__(self, N, L, B, mode, seed):
        assert np.finfo(LD).eps < 1e-18, 'the reference needs a longdouble wider than double'
        rng = np.random.default_rng(seed)
        self.N, self.L, self.B, self.mode = N, L, B, mode
        self.poffs = 1 if mode == 'trapz' else 0
        self.Np = N - self.poffs
        self.nlm = (L + 1) ** 2
        self.W = rng.normal(size=(L + 1, self.Np, N))
        self.x = PC.cplx(rng, (B, N, self.nlm))
        self.s = PC.cplx(rng, (B, N, self.nlm))
        self.Dx, self.Ax = self._contract(self.x)
        self._memo = {}
        for a in (self.W, self.x, self.s):
            a.setflags(write=False)

    @functools.cached_property
    def Ds(self):
        return self._sub[0]

    @functools.cached_property
    def As(self):
        return self._sub[1]

    @functools.cached_property
    def _sub(self):
        """the contractions of the subtracted set, on first use (the plain cases do without)"""
        return self._contract(self.s)

    def _contract(self, v):
        """D = sum_p W[l][p][k] v[b, p + poffs, lm] in longdouble and A >= sum_p |W| |v|, real and imaginary part apart, (B, N, nlm).
        A is a sum of non-negative terms evaluated in double: at least (1 - (Np + 1) 2^-53) of the exact sum whatever the order, so
        it is scaled up by (1 + (Np + 2) 2^-52) and the bound never falls below the one stated."""
        shape = (self.B, self.N, self.nlm)
        Dr, Di, Ar, Ai = (np.zeros(shape, LD) for _ in range(4))
        up = 1 + (self.Np + 2) * 2.0 ** -52
        for l in range(self.L + 1):
            sl = slice(l * l, (l + 1) ** 2)
            Wt = self.W[l].T                                                         # (N, Np): [k, p]
            part = v[:, self.poffs:self.poffs + self.Np, sl]
            Dr[:, :, sl], Di[:, :, sl] = np.matmul(Wt.astype(LD), part.real.astype(LD)), np.matmul(Wt.astype(LD), part.imag.astype(LD))
            Ar[:, :, sl], Ai[:, :, sl] = np.matmul(np.abs(Wt), np.abs(part.real)) * up, np.matmul(np.abs(Wt), np.abs(part.imag)) * up
        for a in (Dr, Di, Ar, Ai):
            a.setflags(write=False)
        return (Dr, Di), (Ar, Ai)

    def _prefactor(self, name, inverse):
        """c_l D per order for D = Dx / Ds, |c_l| A for the bound sums A = Ax / As (the rotation only swaps their parts); kept"""
        if (name, inverse) not in self._memo:
            D, absolute = getattr(self, name), name[0] == 'A'
            scale = LD(INV_SCALE if inverse else FWD_SCALE)
            re, im = np.empty_like(D[0]), np.empty_like(D[1])
            for l in range(self.L + 1):
                sl = slice(l * l, (l + 1) ** 2)
                r = (l & 3) if inverse else ((4 - (l & 3)) & 3)
                a, b = _rot(D[0][:, :, sl], D[1][:, :, sl], r)
                re[:, :, sl], im[:, :, sl] = (np.abs(a), np.abs(b)) if absolute else (a, b)
            out = (re * (abs(scale) if absolute else scale), im * (abs(scale) if absolute else scale))
            for a in out:
                a.setflags(write=False)
            self._memo[(name, inverse)] = out
        return self._memo[(name, inverse)]

    def reference(self, inverse, mask=None):
        """(ref_re, ref_im, bound_re, bound_im); mask: per-restart flags of the difference variant, None = the plain transform"""
        hx, ax = self._prefactor('Dx', inverse), self._prefactor('Ax', inverse)
        n = np.full((self.B, self.N, 1), self.Np + 4, LD)
        if mask is None or not np.any(mask):
            ref, A = hx, ax
        else:
            m = np.asarray(mask, bool).reshape(self.B, 1, 1)
            hs, as_ = self._prefactor('Ds', inverse), self._prefactor('As', inverse)
            above = np.arange(self.N).reshape(1, self.N, 1) > 0
            ref = tuple(np.where(m & above, a - b, a) for a, b in zip(hx, hs))
            A = tuple(np.where(m, a + b, a) for a, b in zip(ax, as_))
            n = np.where(m & ~above, LD(2 * self.Np + 4), n)
        eps = LD(2) ** -52
        return ref[0], ref[1], n * eps * A[0], n * eps * A[1]

    def compare(self, got, inverse, mask=None, what=''):
        """every element of the device's `got` against the reference within the a-priori bound; returns the worst error / bound"""
        assert got.shape == (self.B, self.N, self.nlm) and np.isfinite(got).all(), what
        rr, ri, br, bi = self.reference(inverse, mask)
        assert (br > 0).all() and (bi > 0).all()
        ratio = np.maximum(np.abs(got.real.astype(LD) - rr) / br, np.abs(got.imag.astype(LD) - ri) / bi)
        worst = float(ratio.max())
        if not worst <= 1.0:
            b, k, lm = np.unravel_index(np.argmax(ratio), ratio.shape)
            bad = np.argwhere(ratio > 1.0)
            raise AssertionError('%s: %d elements outside the bound, the worst (restart %d, shell %d, lm %d: order %d) at %.3g times it; '
                                 'restarts %s, shells %d..%d, orders %s' % (
                                     what, len(bad), b, k, lm, int(np.sqrt(lm)), worst, sorted(set(bad[:, 0].tolist())), bad[:, 1].min(),
                                     bad[:, 1].max(), sorted(set(np.sqrt(bad[:, 2]).astype(int).tolist()))))
        return worst


@functools.lru_cache(maxsize=2)
def problem(N, L, B, mode, seed=2718):
    return Problem(N, L, B, mode, seed)


def masks_of(B, mixed):
    """NULL, all zeros, all ones, the mixed pattern and its complement (in an order in which neighbours differ)"""
    m = np.array([ch == '1' for ch in mixed])
    assert m.shape == (B,)
    return [None, np.zeros(B, bool), np.ones(B, bool), m, ~m]


def random_table_engine(p, lib_path):
    e = Engine({'grid': {'n_radial_points': p.N, 'max_order': p.L}, 'fourier_transform': {'type': p.mode}}, None, n_batch=p.B,
               lib_path=lib_path, max_q=1.0)
    assert e.raw_weights.shape == p.W.shape, (e.raw_weights.shape, p.W.shape)
    e._ck(e.lib.mtip_set_hankel_weights(e.ctx, _lib.ptr(p.W), FWD_SCALE, INV_SCALE))
    return e


# ---------------------------------------------------------------------------------------------- the cases
def check_random_tables(lib_path, N, L, B, mode, ct, mixed, n_cu=None, diff_masks=None):
    """both directions of the plain transform and, under each mask, of the difference variant, on a random table at the width ct
    (None: the unforced plan at n_cu compute units), every output element within the a-priori bound"""
    p = problem(N, L, B, mode)
    e = random_table_engine(p, lib_path)
    try:
        plan = assert_plan(e, ct if ct is not None else plan_rule(N, L, B, n_cu)[0])
        worst = {}
        for inverse in (False, True):
            d = 'inv' if inverse else 'fwd'
            plain = e.hankel(p.x, inverse)
            worst[d] = p.compare(plain, inverse, None, d + ' plain')
            _, _, br, bi = p.reference(inverse, None)
            for mask in (masks_of(B, mixed) if diff_masks is None else diff_masks):
                tag = '%s diff mask %s' % (d, 'NULL' if mask is None else ''.join('01'[int(v)] for v in mask))
                got = e.hankel_difference(p.x, p.s, inverse, mask)
                eff = np.ones(B, bool) if mask is None else mask
                worst[d + '_diff'] = max(worst.get(d + '_diff', 0.0), p.compare(got, inverse, eff, tag))
                # the semantics, spelled out: a restart whose byte is 0 is the plain transform of x, and so is shell 0 of every
                # restart (each of the two device results is within its own bound of the same longdouble value)
                _, _, dr, di = p.reference(inverse, eff)
                same = np.broadcast_to((~eff).reshape(B, 1, 1) | (np.arange(N).reshape(1, N, 1) == 0), got.shape)
                assert (np.abs(got.real - plain.real)[same] <= (br + dr)[same]).all(), tag
                assert (np.abs(got.imag - plain.imag)[same] <= (bi + di)[same]).all(), tag
                if not eff.any():
                    assert np.array_equal(got, plain), tag            # nothing subtracted anywhere: the same chain, the same bits
    finally:
        e.close()
    report('N%d L%d B%d %s ct=%d' % (N, L, B, mode, plan[0]), n_tiles=plan[1], n_row_blocks=plan[2], **worst)
    return worst


def check_real_tables(lib_path, N, L, B, mode, ct):
    """the engine's own (Bessel) table against the oracle's Hankel pair at the bound of the operators, per (restart, order) block:
    ties scale, sign and poffs to the oracle at this width"""
    e, fp = PC.transforms_engine(N, L, lib_path, n_batch=B, mode=mode)
    try:
        assert_plan(e, ct)
        co = PC.cplx(np.random.default_rng(N + L), (B, N, e.nlm))
        worst = 0.0
        for inverse in (False, True):
            got, ref = e.hankel(co, inverse), (fp.ihankel if inverse else fp.hankel)(co)
            for b in range(B):
                for l in range(L + 1):
                    sl = slice(l * l, (l + 1) ** 2)
                    err = rel_l2(got[b][:, sl], ref[b][:, sl])
                    worst = max(worst, err)
                    assert err < PC.TOL_OP, (inverse, b, l, err)
    finally:
        e.close()
    report('N%d L%d B%d %s ct=%d oracle' % (N, L, B, mode, ct), worst_block_rel_l2=worst)


def check_difference_arguments(lib_path):
    """mtip_op_hankel_difference refuses null buffers with MTIP_EINVAL and leaves the context usable"""
    p = problem(*FEW_COLUMNS[:4])
    e = random_table_engine(p, lib_path)
    try:
        x, s, out = _lib.as_c128(p.x), _lib.as_c128(p.s), np.empty_like(p.x)
        for args in ((None, _lib.ptr(s), _lib.ptr(out)), (_lib.ptr(x), None, _lib.ptr(out)), (_lib.ptr(x), _lib.ptr(s), None)):
            assert e.lib.mtip_op_hankel_difference(e.ctx, *args, 0, None) == -1                  # MTIP_EINVAL
        assert e.lib.mtip_op_hankel_difference(None, _lib.ptr(x), _lib.ptr(s), _lib.ptr(out), 0, None) == -1
        p.compare(e.hankel_difference(p.x, p.s, False, None), False, np.ones(p.B, bool), 'after the refused calls')
    finally:
        e.close()


GUARDED = [(ROW_BLOCK, (1, 5)), (TRAPZ, (2, 3)), (FEW_COLUMNS, (1, 5)), (LADDER[0], (1, 5)), (LADDER[4], (3,))]


def run_guarded(lib_path):
    """main of the child process of test_emul_hankel.test_no_access_past_buffer_ends: the emulator with MTIP_EMUL_GUARD=1 (every
    device buffer ends at an inaccessible page) through the cases whose tiles, chunks or row blocks end at the end of W, of the
    coefficients or of the mask.  A load past a buffer's end that only feeds rows or columns which are never stored (the W column
    guard of a second row block, the row guard at p = Np) changes no result: here it ends the process."""
    import os
    assert os.environ.get('MTIP_EMUL_GUARD') == '1'
    for (N, L, B, mode, _, mixed), widths in GUARDED:
        for ct in widths:
            os.environ['MTIP_HANKEL_CT'] = str(ct)
            check_random_tables(lib_path, N, L, B, mode, ct, mixed, diff_masks=[np.array([ch == '1' for ch in mixed])])
