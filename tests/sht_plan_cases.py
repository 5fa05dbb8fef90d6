"""Cases that put every SHT plan the default grids reach below L = 64 (plan_sht, csrc/k_sht.hip) through the transforms and through a
phasing step, shared by tests/test_emul_sht_plan.py (CPU emulator) and tests/test_gpu_sht_plan.py (MI355X).

plan_sht picks another set of template instantiations for almost every band of L: k_sht_fwd_pair<MAXI, TH> or k_sht_fwd_reg<MAXI>,
k_sht_inv_wide (one or two workgroups per shell) or k_sht_inv_reg, k_sht_chain<MAXI, THG> with run-time tables, tables in registers
or the L = 32 form, the LDS Stockham pair, the generic kernels; each chained one three times over (store, modulus, real-space
update with the error sums).  Which one runs is read from the context (Engine.sht_plan, mtip_debug_sht_plan): the emulator's
launch log has names without template arguments, the GPU build has neither.

The plan key (KEY_FIELDS) is the tuple of plan fields that select an instantiation or a code path, with n_phi for the FFT radices;
the LDS byte counts and the rows per pass follow from them and the grid.  The census (check_census) takes the key of every
L = 1..63 on its default grid and asserts that their set is the set of keys of REPRESENTATIVES, so a change of the planner that
creates or retires a variant fails until a representative with a test of a step exists; COVERED_ELSEWHERE names the test that runs
a step at the keys this file does not run itself.  The same for CAPPED: MTIP_SHT_TIER caps at which the kernels differ from
their forms at 64 x L16, where tests/test_gpu_parity.py runs every cap.

Shapes: the smallest L of each class, and its neighbour where the class has both parities of L (an even L leaves the last order
without a partner in its wave); 4 .. 6 shells (below four the cubic regridding of the invariants has too few nodes); two restarts
for the chained plans (two slot tables, shell 0 and shells > 0 of either restart), one from L = 49 up.  Every shape's oracle run
was checked to have a non-zero error series (check_loop_vs_oracle asserts it).

Yardsticks, none of them set here: parity_cases.check_transforms (TOL_SHT = 1e-10 rel-L2 against the numpy oracle) and
bigl_loop_cases.check_loop_vs_oracle (2 HIO + SW + 2 ER against the oracle's loop: error series rtol 1e-8, densities 1e-9 rel-L2,
supports equal, oracle errors not all zero, density moved > 1e-3)."""
import contextlib
import os

import bigl_loop_cases as BL
import parity_cases as PC

KEY_FIELDS = ('n_phi', 'fwd', 'fwd_maxi', 'fwd_th', 'inv', 'inv_nsplit', 'real_update', 'chain', 'chain_gsz', 'chain_maxi')
CHAIN_FAMILIES = ('sht_chain', 'sht_chain_modulus', 'sht_chain_real')
FAMILIES = CHAIN_FAMILIES + ('sht_inv_real', 'sht_inv_modulus')

# plan key -> the shapes (N, L, n_theta, n_phi, restarts) this file runs at it, the representative first
K_LDS4 = (4, 'lds', 3, 0, 'lds', 1, False, 'off', 0, 0)
K_LDS8 = (8, 'lds', 3, 0, 'lds', 1, False, 'off', 0, 0)
K_RT128_64 = (64, 'pair', 3, 8, 'wide', 1, True, 'rt', 128, 3)
K_RT128_128 = (128, 'pair', 3, 8, 'wide', 1, True, 'rt', 128, 3)
K_REGTAB2 = (128, 'pair', 3, 8, 'wide', 1, True, 'regtab', 256, 2)
K_REGTAB3 = (128, 'pair', 3, 8, 'wide', 1, True, 'regtab', 256, 3)
K_RT512 = (128, 'pair', 5, 8, 'wide', 1, True, 'rt', 512, 3)
K_PAIR_REG = (256, 'pair', 5, 4, 'reg', 1, False, 'off', 0, 0)
K_REG9 = (256, 'reg', 9, 0, 'reg', 1, False, 'off', 0, 0)
K_LDS9 = (256, 'lds', 9, 0, 'lds', 1, False, 'off', 0, 0)
SHAPES = {
    K_LDS4: ((4, 1, 0, 0, 1),),                                # L = 1: Stockham pair at n_phi = 4
    K_LDS8: ((4, 2, 0, 0, 1),),                                # L = 2: n_phi = 8
    K_RT128_64: ((4, 19, 0, 0, 2), (6, 20, 0, 0, 2)),          # L = 19..21: n_phi 64, pair TH 8, chain RT, group 128, MAXI 3
    K_RT128_128: ((4, 22, 0, 0, 2), (4, 23, 0, 0, 2)),         # L = 22..26: the same chain at n_phi 128
    K_REGTAB2: ((4, 27, 0, 0, 2), (5, 28, 0, 0, 2)),           # L = 27..30: chain REGTAB MAXI 2
    K_REGTAB3: ((4, 31, 0, 0, 2),),                            # L = 31, 33..37: chain REGTAB MAXI 3 (L = 33: the bit fixture's neighbour)
    K_RT512: ((4, 38, 0, 0, 2), (4, 39, 0, 0, 2)),             # L = 38..42: forward pair MAXI 5, chain RT, group 512
    K_PAIR_REG: ((4, 49, 0, 0, 1),),                           # L = 49: pair MAXI 5 forward, register inverse, no real_update
    K_REG9: ((4, 50, 0, 0, 1), (4, 51, 0, 0, 1)),              # L = 50..59: k_sht_fwd_reg<9> / k_sht_inv_reg
    K_LDS9: ((4, 60, 0, 0, 1), (4, 61, 0, 0, 1)),              # L = 60..63: LDS Stockham, MAXI 9
}
# plan key -> (shape, the GPU test that runs a phasing step at it)
COVERED_ELSEWHERE = {
    (16, 'pair', 3, 2, 'wide', 1, True, 'rt', 128, 1): ((16, 4, 0, 0, 2), 'test_gpu_parity.py::test_short_trajectory_vs_oracle'),
    (32, 'pair', 3, 4, 'wide', 1, True, 'rt', 64, 1): ((32, 8, 0, 0, 1), 'test_gpu_parity.py::test_trajectory_golden_cfg1'),
    (32, 'pair', 3, 4, 'wide', 1, True, 'rt', 64, 3): ((24, 10, 0, 0, 5), 'test_gpu_parity.py::test_invariant_metrics_vs_oracle_synthetic'),
    (64, 'pair', 3, 8, 'wide', 1, True, 'rt', 64, 3): ((64, 16, 0, 0, 2), 'test_gpu_parity.py::test_config2_trajectory_vs_oracle'),
    (128, 'pair', 3, 8, 'wide', 1, True, 'l32', 256, 3): ((4, 32, 0, 0, 2), 'test_gpu_chain_latency.py::test_fused_steps_ft_stab'),
    (256, 'pair', 5, 4, 'wide', 2, True, 'off', 0, 0): ((12, 48, 0, 0, 2), 'test_gpu_parity.py::test_split_shell_steps_vs_oracle'),
}
REPRESENTATIVES = {**{k: v[0] for k, v in SHAPES.items()}, **{k: v[0] for k, v in COVERED_ELSEWHERE.items()}}
CASES = [s for shapes in SHAPES.values() for s in shapes]
KEY_OF = {s: k for k, shapes in SHAPES.items() for s in shapes}
EMUL_LOOP_CASES = [(6, 20, 0, 0, 2), (5, 28, 0, 0, 2), (4, 49, 0, 0, 1)]
GUARDED_CASE = (5, 28, 0, 0, 2)

# (cap, shape) -> plan key: MTIP_SHT_TIER caps whose kernels are not the MAXI 3 forms of 64 x L16; 4 shells, one restart
CAPPED_TRANSFORMS = {
    (1, (4, 44, 0, 0, 1)): (256, 'lds', 5, 0, 'lds', 1, False, 'off', 0, 0),       # k_sht_fwd_fused<5>
    (1, (4, 55, 0, 0, 1)): K_LDS9,                                                 # MAXI 9 where the default takes the register kernels
    (2, (4, 40, 0, 0, 1)): (128, 'reg', 5, 0, 'reg', 1, False, 'off', 0, 0),       # k_sht_fwd_reg<5>, register inverse at n_phi 128
    (3, (4, 40, 0, 0, 1)): (128, 'pair', 5, 8, 'wide', 1, False, 'off', 0, 0),     # pair MAXI 5, wide inverse without real_update
}
CAPPED_LOOP = {
    (4, (4, 28, 0, 0, 1)): (128, 'pair', 3, 8, 'wide', 1, True, 'off', 0, 0),      # wide real-update epilogue + coefficient difference at n_phi 128
    (1, (4, 44, 0, 0, 1)): (256, 'lds', 5, 0, 'lds', 1, False, 'off', 0, 0),
}
CAPPED = {**CAPPED_TRANSFORMS, **CAPPED_LOOP}


def case_id(shape):
    return '%dxL%d-B%d' % (shape[0], shape[1], shape[4])


# -------------------------------------------------------------------------------------------------------------------- the plan
def plan_key(e):
    p = e.sht_plan()
    return (e.n_phi,) + tuple(p[k] for k in KEY_FIELDS[1:])


@contextlib.contextmanager
def tier_cap(cap):
    """MTIP_SHT_TIER = cap (None: unset) while a context is created: plan_sht reads it when the angular grid is set"""
    old = os.environ.get('MTIP_SHT_TIER')
    if cap is None:
        os.environ.pop('MTIP_SHT_TIER', None)
    else:
        os.environ['MTIP_SHT_TIER'] = str(cap)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('MTIP_SHT_TIER', None)
        else:
            os.environ['MTIP_SHT_TIER'] = old


def key_of_geometry(shape, lib_path):
    """the plan key of a transforms-only context of this shape (under the MTIP_SHT_TIER of the caller); nothing is launched"""
    N, L, nt, nphi, B = shape
    e, _ = PC.transforms_engine(N, L, lib_path, n_batch=B, n_theta=nt, n_phi=nphi)
    try:
        p = e.sht_plan()
        assert set(p) == set(e.SHT_PLAN_FIELDS) and p['fwd'] in e.SHT_FWD_KINDS and p['inv'] in e.SHT_INV_KINDS, p
        return plan_key(e)
    finally:
        e.close()


def check_census(lib_path):
    """every L = 1..63 on its default grid with the default cap: the set of plan keys is the set of REPRESENTATIVES' keys, every
    representative (and every neighbour this file runs) has the key it stands for; the same for the capped entries"""
    with tier_cap(None):
        census = {}
        for L in range(1, 64):
            census.setdefault(key_of_geometry((2, L, 0, 0, 1), lib_path), []).append(L)
        for k, ls in census.items():
            print(dict(zip(KEY_FIELDS, k)), 'L =', ls)
        assert not set(SHAPES) & set(COVERED_ELSEWHERE)
        missing, retired = set(census) - set(REPRESENTATIVES), set(REPRESENTATIVES) - set(census)
        assert not missing, 'plans without a representative (add one with a GPU test of a step): %s' % {k: census[k] for k in missing}
        assert not retired, 'representatives of plans no default grid reaches any more: %s' % retired
        for key, shape in REPRESENTATIVES.items():
            assert shape[1] in census[key] and shape[2:4] == (0, 0), (key, shape)
            assert key_of_geometry(shape, lib_path) == key, (key, shape)
        for shape in CASES:
            assert key_of_geometry(shape, lib_path) == KEY_OF[shape], shape
    for (cap, shape), key in CAPPED.items():
        with tier_cap(cap):
            assert key_of_geometry(shape, lib_path) == key, (cap, shape)
        assert shape[1] not in census.get(key, ()), (cap, shape)                   # the cap moves this L onto other kernels


# ----------------------------------------------------------------------------------------------------------------------- (a)
def check_transforms(shape, lib_path, key=None):
    """parity_cases.check_transforms at a plan that is asserted first, expect_chain taken from it"""
    N, L, nt, nphi, B = shape
    key = KEY_OF[shape] if key is None else key
    assert key_of_geometry(shape, lib_path) == key, shape
    fig = {}
    PC.check_transforms(N, L, lib_path, seed=200 + N + L, expect_chain=key[7] != 'off', n_theta=nt, n_phi=nphi, n_batch=B, figures=fig)
    print('SHTPLAN transforms %s key %s: rel-L2 %.2e' % (case_id(shape), key, fig['transforms']))


# ------------------------------------------------------------------------------------------------------------------ (b), (c)
def check_loop(shape, lib_path, fused, key=None, tag=''):
    """bigl_loop_cases.check_loop_vs_oracle (2 HIO + SW + 2 ER, its bounds) in the default context at a plan that is asserted on the
    loop's own engine; for the fused step, the kernel families that ran (hipEvent brackets, profile_get) are those of the plan"""
    key = KEY_OF[shape] if key is None else key
    plan = dict(zip(KEY_FIELDS, key))
    ran, fig = {}, {}

    def before(e):
        assert plan_key(e) == key, (shape, plan_key(e))
        e.profile(True)

    def after(e):
        ran.update({f: e.profile_get(f)[1] for f in FAMILIES})
        e.profile(False)

    BL.check_loop_vs_oracle(shape, BL.SCHEDULE, lib_path, fused=fused, big_l=False, before_run=before, after_run=after, figures=fig,
                            tag=tag)
    print('SHTPLAN loop %s %s%s key %s: densities %.2e errors %.2e; launches %s'
          % (case_id(shape), tag, 'fused' if fused else 'reference order', key, fig['density'], fig['errors'], ran))
    if not fused:
        return
    if plan['chain'] != 'off':
        assert all(ran[f] > 0 for f in CHAIN_FAMILIES), ran
    else:
        assert all(ran[f] == 0 for f in CHAIN_FAMILIES), ran
        if plan['real_update']:
            assert ran['sht_inv_real'] > 0, ran
        else:
            assert ran['sht_inv_modulus'] > 0 and ran['sht_inv_real'] == 0, ran


# --------------------------------------------------------------------------------------------------- child processes: the caps
def run_capped_transforms(cap, shape, lib_path=None):
    assert os.environ.get('MTIP_SHT_TIER') == str(cap)
    check_transforms(tuple(shape), lib_path, CAPPED_TRANSFORMS[cap, tuple(shape)])
    print('SHT plan capped transforms ok')


def run_capped_loop(cap, shape, lib_path=None):
    assert os.environ.get('MTIP_SHT_TIER') == str(cap)
    for fused in (True, False):
        check_loop(tuple(shape), lib_path, fused, CAPPED_LOOP[cap, tuple(shape)], tag='cap %d ' % cap)
    print('SHT plan capped loop ok')


def run_guarded(lib_path):
    """child process with MTIP_EMUL_GUARD=1: every device allocation of the emulator ends at an inaccessible page"""
    assert os.environ.get('MTIP_EMUL_GUARD') == '1'
    check_loop(GUARDED_CASE, lib_path, True, tag='guarded ')
    print('SHT plan guarded ok')
