"""`schedule.walk` alone, on a scripted state that records the protocol calls: no library, no emulator.  The expected call lists are
written out by hand from the upstream loop (reconstruct.py:814-952) and the ramps of fxs_Projections.py:218-243, not produced by
the walker."""
import numpy as np

from xframe_amd.fxs import schedule

F, T = False, True
LINK = {'ft_stab': 'link_to_enforce_initial_support', 'link_to_enforce_initial_support': {'delay': 1}}
LIMIT = 0.05
DEFAULT_SIGMA = 7.0
BETA_A = [0.9, 0.5, -0.1, 10]
BETA_DEFAULT = [0.5, 0.5, -1 / 700, 1600]          # reconstruct.py:868, for a sub-loop beyond the end of HIO.beta


def beta(cfg, x):
    """ExponentialRamp of the reference (start, stop, exponent, stop argument), restated"""
    start, stop, exponent, stop_argument = cfg
    exponent = -abs(exponent) if stop < start else abs(exponent)
    a = (start - stop) / (1 - np.exp(exponent * stop_argument))
    v = a * np.exp(x * exponent) + (start - a)
    return max(v, stop) if start > stop else min(v, stop)


def settings(sub_loops, sigmas=(False,), thresholds=(0.1,), betas=(BETA_A,)):
    return {'main_loop': {'sub_loops': sub_loops},
            'projections': {'real': {'HIO': {'beta': list(betas)},
                                     'shrink_wrap': {'sigmas': list(sigmas), 'thresholds': list(thresholds)},
                                     'projections': {'support': {'enforce_initial_support': {'apply': True, 'if_error_bigger_than': LIMIT}}}}}}


class Scripted:
    """records every protocol call; `shrinkwrap` and `main_errors` answer from lists.  centre: what `before_sw_center` returns --
    None (the 3-D state) or the decisions of a 2-D state, in turn"""

    def __init__(self, enforce=(), errors=(), centre=None):
        self.calls = []
        self.enforce = [np.array(e) for e in enforce]
        self.errors = np.array(errors, dtype=float)
        self.centre = None if centre is None else [np.array(c) for c in centre]

    def check_method(self, key):
        self.calls.append(('check_method', key))

    def begin_sub_loop(self):
        self.calls.append(('begin_sub_loop',))

    def shrinkwrap(self, sigma, threshold, limit):
        self.calls.append(('shrinkwrap', sigma, threshold, limit))
        return self.enforce.pop(0)

    def before_sw_center(self, limit):
        self.calls.append(('before_sw_center', limit))
        return None if self.centre is None else self.centre.pop(0)

    def refresh_reciprocal_density(self):
        self.calls.append(('refresh_reciprocal_density',))

    def run(self, key, ft_stab, betas):
        assert isinstance(betas, np.ndarray) and betas.dtype == np.float64
        assert isinstance(ft_stab, bool) or (isinstance(ft_stab, np.ndarray) and ft_stab.dtype == bool)
        self.calls.append(('run', key, ft_stab if isinstance(ft_stab, bool) else ft_stab.tolist(), betas.tolist()))

    def main_errors(self, first, n):
        self.calls.append(('main_errors', first, n))
        return self.errors[first:first + n]

    def select_best(self, where):
        self.calls.append(('select_best', np.asarray(where).tolist()))


# Sub-loop a (index 0): its own beta ramp; sigma ramp 4 -> 2 over two updates, threshold ramp 0.125 -> 0.375 over two; reselects.
# Sub-loop b (index 1): beyond the end of HIO.beta (the default) and of the thresholds (0.1), sigma 10 - 2 x in the shrink-wrap
# updates of THIS sub-loop (8 after its first; counted on from sub-loop a's six it would be -4: the default sigma); no 'SW' in it and
# no reselection.
SUB_LOOPS = {
    'order': ['a', 'b'],
    'a': {'iterations': 2, 'order': ['HIO', 'HIO_non_FXS', 'SW', 'ER', 'SW_center'], 'best_density_not_in_first_n_iterations': 0,
          'methods': {'HIO': dict(iterations=2, **LINK), 'HIO_non_FXS': {'iterations': 0, 'ft_stab': True}, 'SW': 1,
                      'ER': {'iterations': 1, 'ft_stab': False}, 'SW_center': 2}},
    'b': {'iterations': 2, 'order': ['HIO', 'SW_center'], 'methods': {'HIO': dict(iterations=1, **LINK), 'SW_center': 1}}}
SIGMAS = [[4.0, [2.0, 2]], [10.0, False, -2.0]]
THRESHOLDS = [[0.125, [0.375, 2]]]
# the enforce decisions, in the order the shrink-wraps are issued (those marked * must not reach the ft_stab link)
ENFORCE = [[F, F],                  # a, iteration 1, SW
           [T, F], [F, F],          # a, iteration 1, SW_center: first update, second *
           [T, T],                  # a, iteration 2, SW
           [T, T], [F, F],          # a, iteration 2, SW_center: first, second *
           [F, F],                  # b, iteration 1, SW_center
           [F, F]]                  # b, iteration 2, SW_center
# main errors of the 8 steps (a: iterations 1, 1, 1, 2, 2, 2; b: 1, 2).  Restart 0 improves (a NaN in between never wins): its best
# iteration is >= 1 > 0; restart 1 never has an error below its starting inf (inf > inf is false, NaN compares false): iteration 0
ERRORS = [[5.0, np.inf], [np.nan, np.nan], [2.0, np.inf], [2.0, np.nan], [3.0, np.nan], [2.5, np.inf], [1.0, 1.0], [0.5, 0.5]]

EXPECTED = [
    # ---- sub-loop a
    ('check_method', 'HIO'), ('check_method', 'HIO_non_FXS'), ('check_method', 'SW'), ('check_method', 'ER'), ('check_method', 'SW_center'),
    ('begin_sub_loop',),
    # 'SW' is in the loop: ramps at 0 -> sigma 4, threshold 0.125, before anything runs
    # iteration 1
    ('run', 'HIO', F, [beta(BETA_A, 0), beta(BETA_A, 1)]),                      # no enforce decision yet: the link says no
    ('run', 'HIO_non_FXS', T, []),                                              # no steps, still issued, with its ft_stab
    ('shrinkwrap', 4.0, 0.125, LIMIT),                                          # -> [F, F]; then ramps at 1: 3, 0.25
    ('run', 'ER', F, [beta(BETA_A, 2)]),
    ('before_sw_center', LIMIT),
    ('shrinkwrap', 3.0, 0.25, LIMIT), ('refresh_reciprocal_density',),          # -> [T, F], the one decision kept; ramps at 2: 2, 0.375
    ('shrinkwrap', 2.0, 0.375, LIMIT), ('refresh_reciprocal_density',),         # -> [F, F] *; ramps at 3: clamped at 2, 0.375
    # iteration 2
    ('run', 'HIO', [F, T], [beta(BETA_A, 3), beta(BETA_A, 4)]),                 # last decision [T, F]: the restarts disagree
    ('run', 'HIO_non_FXS', T, []),
    ('shrinkwrap', 2.0, 0.375, LIMIT),                                          # -> [T, T]
    ('run', 'ER', F, [beta(BETA_A, 5)]),
    ('before_sw_center', LIMIT),
    ('shrinkwrap', 2.0, 0.375, LIMIT), ('refresh_reciprocal_density',),         # -> [T, T]
    ('shrinkwrap', 2.0, 0.375, LIMIT), ('refresh_reciprocal_density',),         # -> [F, F] *
    ('main_errors', 0, 6),
    ('select_best', [T, F]),
    # ---- sub-loop b: no 'SW' in it, so no ramp update at 0 -- sigma and threshold are what sub-loop a left
    ('check_method', 'HIO'), ('check_method', 'SW_center'),
    ('begin_sub_loop',),
    ('run', 'HIO', F, [beta(BETA_DEFAULT, 0)]),                                 # last decision [T, T]: both enforced, no ft_stab
    ('before_sw_center', LIMIT),
    ('shrinkwrap', 2.0, 0.375, LIMIT), ('refresh_reciprocal_density',),         # -> [F, F]; ramps of loop 1 at sw_step 1: 10 - 2, 0.1
    ('run', 'HIO', T, [beta(BETA_DEFAULT, 1)]),                                 # last decision [F, F]
    ('before_sw_center', LIMIT),
    ('shrinkwrap', 8.0, 0.1, LIMIT), ('refresh_reciprocal_density',),
    ('main_errors', 6, 2),                                                      # (followed to the end once some loop reselects; nobody flagged)
]


def run_main():
    opt = settings(SUB_LOOPS, SIGMAS, THRESHOLDS)
    state = Scripted(ENFORCE, ERRORS)
    ramps = schedule.ShrinkWrapRamps(opt, DEFAULT_SIGMA)
    assert (ramps.sigma, ramps.threshold) == (DEFAULT_SIGMA, 0.06)
    return state, schedule.walk(opt, state, ramps, 2)


def test_walk_call_list():
    state, (iterations, n_steps) = run_main()
    assert len(state.calls) == len(EXPECTED)
    for i, (got, want) in enumerate(zip(state.calls, EXPECTED)):
        assert got == want, (i, got, want)
    assert iterations == [2, 2] and n_steps == 8
    assert state.enforce == []


def test_walk_points_of_the_contract():
    calls = run_main()[0].calls
    runs = [c for c in calls if c[0] == 'run']
    # blocks of no steps are real calls with their own ft_stab; betas count the phasing steps within the sub-loop
    assert [c for c in runs if c[1] == 'HIO_non_FXS'] == [('run', 'HIO_non_FXS', T, [])] * 2
    assert [b for c in runs[:6] for b in c[3]] == [beta(BETA_A, i) for i in range(6)]
    assert [b for c in runs[6:] for b in c[3]] == [beta(BETA_DEFAULT, i) for i in range(2)]
    assert abs(beta(BETA_A, 0) - 0.9) < 1e-15 and 0.5 < beta(BETA_A, 5) < beta(BETA_A, 4) and beta(BETA_DEFAULT, 1) == 0.5
    # one ft_stab decision per block: False, an array, True all occur on the linked HIO
    assert [c[2] for c in runs if c[1] == 'HIO'] == [F, [F, T], F, T]
    # reselection: only the flagged restart, only in the loop that asks for it
    assert [c for c in calls if c[0] == 'select_best'] == [('select_best', [T, F])]
    # a sub-loop's keys are checked before it begins
    assert calls.index(('check_method', 'SW_center')) < calls.index(('begin_sub_loop',))


# What a sub-loop hands to the next one, and what it does not.  Sub-loop p: two iterations of 2 HIO + SW, never reselects.  Sub-loop q:
# one iteration of ER (linked), SW, 2 HIO, SW, its own beta ramp, reselects when the best iteration is past the first.
#   carried over: the enforce decisions (q's ER sees p's last, [F, F]: ft_stab), best error and best iteration (restart 0's best is
#   p's iteration 2, nothing in q beats it: 2 > 1, reselected; restart 1's is p's iteration 1: not)
#   restarting: the step count of the beta ramp (q's betas are its ramp at 0, 1, 2) and the shrink-wrap count (q's ramps at 0, then 1:
#   sigma 1 - 1 = 0 is no sigma -> the default; threshold 0.5 + 0.5 -> clamped to 1)
BETA_Q = [0.8, 0.2, -0.05, 20]
CARRY_LOOPS = {
    'order': ['p', 'q'],
    'p': {'iterations': 2, 'order': ['HIO', 'SW'], 'methods': {'HIO': dict(iterations=2, **LINK), 'SW': 1}},
    'q': {'iterations': 1, 'order': ['ER', 'SW', 'HIO', 'SW'], 'best_density_not_in_first_n_iterations': 1,
          'methods': {'ER': dict(iterations=1, **LINK), 'SW': 1, 'HIO': {'iterations': 2, 'ft_stab': False}}}}
CARRY_ENFORCE = [[T, T], [F, F], [T, F], [F, F]]
CARRY_ERRORS = [[5.0, 1.0], [4.0, 2.0], [3.0, 3.0], [2.0, 3.0], [2.5, 4.0], [2.2, 4.0], [2.1, 4.0]]
CARRY_EXPECTED = [
    ('check_method', 'HIO'), ('check_method', 'SW'),
    ('begin_sub_loop',),
    ('run', 'HIO', F, [beta(BETA_A, 0), beta(BETA_A, 1)]),
    ('shrinkwrap', 4.0, 0.125, LIMIT),                                          # -> [T, T]
    ('run', 'HIO', F, [beta(BETA_A, 2), beta(BETA_A, 3)]),
    ('shrinkwrap', 3.0, 0.25, LIMIT),                                           # -> [F, F]
    ('main_errors', 0, 4),
    ('check_method', 'ER'), ('check_method', 'SW'), ('check_method', 'HIO'), ('check_method', 'SW'),      # the order, entry by entry
    ('begin_sub_loop',),
    ('run', 'ER', T, [beta(BETA_Q, 0)]),                                        # p's last decision, p's step count gone
    ('shrinkwrap', 1.0, 0.5, LIMIT),                                            # q's ramps at 0; -> [T, F]
    ('run', 'HIO', F, [beta(BETA_Q, 1), beta(BETA_Q, 2)]),
    ('shrinkwrap', DEFAULT_SIGMA, 1, LIMIT),                                    # q's ramps at 1, not at 3
    ('main_errors', 4, 3),
    ('select_best', [T, F]),
]


def test_what_sub_loops_hand_on():
    opt = settings(CARRY_LOOPS, [SIGMAS[0], [1.0, False, -1.0]], [THRESHOLDS[0], [0.5, False, 0.5]], [BETA_A, BETA_Q])
    state = Scripted(CARRY_ENFORCE, CARRY_ERRORS)
    iterations, n_steps = schedule.walk(opt, state, schedule.ShrinkWrapRamps(opt, DEFAULT_SIGMA), 2)
    assert len(state.calls) == len(CARRY_EXPECTED)
    for i, (got, want) in enumerate(zip(state.calls, CARRY_EXPECTED)):
        assert got == want, (i, got, want)
    assert (iterations, n_steps) == ([2, 1], 7)
    betas = [beta(BETA_Q, i) for i in range(3)] + [beta(BETA_A, i) for i in range(4)]
    assert len(set(betas)) == 7                                     # every beta of this case tells its ramp and its step


def test_unknown_key_before_unreadable_one():
    """the keys of a sub-loop are read and checked in the order's sequence: what the first bad entry raises is what comes out"""
    class Refusing(Scripted):
        def check_method(self, key):
            if key == 'RAAR':
                raise NotImplementedError(key)

    def raised(order):
        opt = settings({'order': ['main'], 'main': {'iterations': 1, 'order': order, 'methods': {'HIO': 1, 'RAAR': 1}}})
        try:
            schedule.walk(opt, Refusing(), schedule.ShrinkWrapRamps(opt, DEFAULT_SIGMA), 1)
        except (NotImplementedError, KeyError) as err:
            return type(err)
    assert raised(['HIO', 'RAAR', 'missing']) is NotImplementedError
    assert raised(['HIO', 'missing', 'RAAR']) is KeyError


def test_no_reselection_no_reads():
    """no sub-loop with a finite best_density_not_in_first_n_iterations: the main errors are never read (a read waits for the device)"""
    loops = {'order': ['main'], 'main': {'iterations': 3, 'order': ['HIO', 'SW', 'ER'], 'methods': {'HIO': 2, 'SW': 1, 'ER': {'iterations': 1}}}}
    opt = settings(loops)
    state = Scripted([[F]] * 3)
    iterations, n_steps = schedule.walk(opt, state, schedule.ShrinkWrapRamps(opt, DEFAULT_SIGMA), 1)
    assert (iterations, n_steps) == ([3], 9)
    assert {c[0] for c in state.calls} == {'check_method', 'begin_sub_loop', 'run', 'shrinkwrap'}
    # sigma undefined (False): the default stays; thresholds[0] = 0.1 is constant
    assert [c for c in state.calls if c[0] == 'shrinkwrap'] == [('shrinkwrap', DEFAULT_SIGMA, 0.1, LIMIT)] * 3
    assert [c[2] for c in state.calls if c[0] == 'run'] == [F] * 6                 # bare counts and option-less methods: no ft_stab


def centre_loops(n_center):
    return {'order': ['main'], 'main': {'iterations': 1, 'order': ['HIO', 'SW_center', 'ER'], 'methods': {
        'HIO': 1, 'SW_center': {'iterations': n_center}, 'ER': dict(iterations=1, **LINK)}}}


def test_sw_center_decision_of_the_state():
    """a state that answers `before_sw_center` with a decision (the 2-D ones: from the last main error) has that ONE decision linked,
    also with no support update at all; a state that answers None (3-D) has the first update's, and none without an update"""
    def er_flag(n_center, centre, enforce):
        opt = settings(centre_loops(n_center))
        state = Scripted(enforce, centre=centre)
        schedule.walk(opt, state, schedule.ShrinkWrapRamps(opt, DEFAULT_SIGMA), 2)
        assert [c[0] for c in state.calls].count('shrinkwrap') == n_center == [c[0] for c in state.calls].count('refresh_reciprocal_density')
        # 'SW_center' alone never moves the ramps to their start: the first update runs on the initial pair
        assert n_center == 0 or [c for c in state.calls if c[0] == 'shrinkwrap'][0] == ('shrinkwrap', DEFAULT_SIGMA, 0.06, LIMIT)
        return [c for c in state.calls if c[0] == 'run'][-1][2]
    assert er_flag(2, [[T, T]], [[F, F], [F, F]]) is F              # the state's decision, not the updates'
    assert er_flag(0, [[T, F]], []) == [F, T]                       # no update: still linked
    assert er_flag(2, None, [[T, T], [F, F]]) is F                  # the first update's, not the second's
    assert er_flag(2, None, [[F, F], [T, T]]) is T
    assert er_flag(0, None, []) is F                                # nothing decided, nothing linked


def test_change_to_ft_stab_contract():
    f = schedule.change_to_ft_stab
    two = {'ft_stab': 'link_to_enforce_initial_support', 'link_to_enforce_initial_support': {'delay': 2}}
    e = [np.array(x) for x in ([T, F], [F, F], [F, T])]
    assert f({}, 'HIO', e) is F and f({'ft_stab': T}, 'HIO', e) is T and f({'ft_stab': T}, 'HIO_ft_stab', e) is F
    assert f(two, 'HIO', e[:1]) is F                                # fewer decisions than the delay
    assert f(two, 'HIO', e[:2]).tolist() == [F, T]                  # enforced within the last two: restart 0 only
    assert f(two, 'HIO', e).tolist() == [T, F]
    assert f(two, 'HIO', e[1:2] * 2) is T and f(two, 'HIO', [np.array([T, T])] * 2) is F
    assert f(dict(two, link_to_enforce_initial_support={'delay': 0}), 'HIO', e).tolist() == [T, F]      # a delay below 1 is 1


def test_parse_methods():
    lo = {'order': ['HIO', 'SW', 'ER'], 'methods': {'HIO': {'iterations': 3, 'ft_stab': T}, 'SW': 1, 'ER': {'ft_stab': F}, 'unused': 9}}
    assert schedule.parse_methods(lo) == {'HIO': {'iterations': 3, 'options': {'iterations': 3, 'ft_stab': T}},
                                          'SW': {'iterations': 1, 'options': {}}, 'ER': {'iterations': 0, 'options': {'ft_stab': F}}}
