"""The sub-loop state machine of ``xframe/projects/fxs/reconstruct.py`` (814-952), once, for every phasing loop of this package:
the only place that reads ``main_loop.sub_loops``.  `walk` goes through the sub-loops, their iterations and method blocks, keeps
what upstream decides on the host (beta and shrink-wrap ramps, the `ft_stab` link to the enforce decisions, the best iteration and
the end-of-loop reselection) and talks to the loop's state through eight calls:

    check_method(key)                       for every key of a sub-loop, at its top; raises what that loop cannot run
    begin_sub_loop()                        859 / 866: stale history := history, no non-FXS intensity
    shrinkwrap(sigma, threshold, limit)     new support from the latest real density -> the enforce decision, (B,) bool
    before_sw_center(limit)                 887: the decision from the last main error (IndexError before any step), or None where
                                            the first support update's own decision stands for it
    refresh_reciprocal_density()            'SW_center' tail, 891-894
    run(key, ft_stab, betas)                len(betas) steps of one method; a block of no steps is still a call (it takes / drops the
                                            non-FXS intensity)
    main_errors(first, n) -> (n, B)         read only
    select_best(where)                      945-949 for the flagged restarts

The states: `reconstruct._EngineState` (3-D, resident `Engine`), `reconstruct2d._ResidentState` (`Engine2D.run`) and
`reconstruct2d._OperatorState` (one `Engine2D.step` per step, histories on the host).  Host Python only, nothing shared between
calls: every engine group of the worker walks its own schedule on its own thread."""
import numpy as np

from . import hostsetup as hs

DEFAULT_BETA = (0.5, 0.5, -1 / 700, 1600)


class ShrinkWrapRamps:
    """the sigma / threshold ramps of every sub-loop (reconstruct.py:1212-1258) and the current pair `sigma`, `threshold`"""

    def __init__(self, opt, default_sigma):
        sw_opt = opt['projections']['real']['shrink_wrap']
        self.default_sigma = default_sigma
        self._sigmas, self._thresholds = [], []
        for lid in range(len(opt['main_loop']['sub_loops']['order'])):
            s = sw_opt['sigmas'][lid] if len(sw_opt['sigmas']) - 1 >= lid else False
            s = s if isinstance(s, (list, tuple)) else [s]
            self._sigmas.append(hs.LinearRamp(*s, default_start=default_sigma, default_stop=default_sigma))
            t = sw_opt['thresholds'][lid] if len(sw_opt['thresholds']) - 1 >= lid else 0.1
            t = t if isinstance(t, (list, tuple)) else [t]
            self._thresholds.append(hs.LinearRamp(*t))
        self.sigma, self.threshold = default_sigma, 0.06

    def update(self, iteration, loop_number):
        r = self._sigmas[loop_number]
        if not r.undefined:
            v = r(iteration)
            ok = np.issubdtype(np.array(v).dtype, np.number) and not isinstance(v, bool) and v > 0
            self.sigma = v if ok else self.default_sigma                     # fxs_Projections.py:233-243
        t = self._thresholds[loop_number]
        if not t.undefined:
            v = t(iteration)
            self.threshold = 0 if v < 0 else (1 if v >= 1 else v)            # 218-227


def change_to_ft_stab(popt, name, eis_list):
    """reconstruct.py:836-850: the reference decides per reconstruction process -- a bool when the restarts agree, else one per
    restart (`Engine.run` / `Engine2D.run` / `MTIP2D._step` take it)"""
    if name[-8:] == '_ft_stab' or 'ft_stab' not in popt:
        return False
    v = popt['ft_stab']
    if isinstance(v, bool):
        return v
    if v == 'link_to_enforce_initial_support':
        delay = max(int(popt['link_to_enforce_initial_support']['delay']), 1)
        if len(eis_list) >= delay:
            recent = np.array(eis_list[-delay:])            # (delay, B)
            flags = ~(recent == True).any(axis=0)          # noqa: E712
            if flags.all() != flags.any():
                return flags
            return bool(flags.all())
    return False


def parse_methods(lo, check=None):
    """key -> {'iterations', 'options'} of a sub-loop's method table (a bare number is the iteration count); `check(key)` follows
    every entry of the order as it is read, so the first entry that cannot be read or run is the one that raises"""
    methods = {}
    for key in lo['order']:
        mo = lo['methods'][key]
        methods[key] = ({'iterations': mo.get('iterations', 0), 'options': mo} if isinstance(mo, dict)
                        else {'iterations': mo, 'options': {}})
        if check is not None:
            check(key)
    return methods


def walk(opt, state, ramps, B):
    """the sub-loops of `opt` on `state` (the protocol above) for B restarts -> (last iteration number of every sub-loop, steps)"""
    loops = opt['main_loop']['sub_loops']
    beta_opt = opt['projections']['real']['HIO']['beta']
    eis_opt = opt['projections']['real']['projections']['support']['enforce_initial_support']
    limit = eis_opt['if_error_bigger_than'] if eis_opt['apply'] else np.inf
    # best_error / best_iteration per restart (934-938) are only followed when some loop reselects the best density at its end
    # (945-949): reading the main errors waits for the device
    track_best = any(np.isfinite(loops[name].get('best_density_not_in_first_n_iterations', np.inf)) for name in loops['order'])
    best_err, best_iter = np.full(B, np.inf), np.zeros(B, int)
    eis_list, iterations, n_steps = [], [], 0
    for loop_number, loop_name in enumerate(loops['order']):
        lo = loops[loop_name]
        methods = parse_methods(lo, state.check_method)
        state.begin_sub_loop()
        ramp = hs.ExponentialRamp(*(beta_opt[loop_number] if len(beta_opt) - 1 >= loop_number else DEFAULT_BETA))
        if 'SW' in methods:
            ramps.update(0, loop_number)
        loop_first_step, step_iteration = n_steps, []
        step = sw_step = iteration = 0
        for iteration in range(1, lo['iterations'] + 1):
            for key in lo['order']:
                if key == 'SW':                                               # 877-885
                    eis_list.append(state.shrinkwrap(ramps.sigma, ramps.threshold, limit))
                    sw_step += 1
                    ramps.update(sw_step, loop_number)
                    continue
                if key == 'SW_center':
                    # 886-897: one enforce decision, then `iterations` support updates, each replacing the last pair (the sketch,
                    # 606-613, shifts nothing and hands its outputs back in swapped order)
                    enforced = state.before_sw_center(limit)
                    if enforced is not None:
                        eis_list.append(enforced)
                    for i in range(methods[key]['iterations']):
                        first = state.shrinkwrap(ramps.sigma, ramps.threshold, limit)
                        if i == 0 and enforced is None:
                            eis_list.append(first)
                        state.refresh_reciprocal_density()
                        sw_step += 1
                        ramps.update(sw_step, loop_number)
                    continue
                repeats = methods[key]['iterations']
                ft_stab = change_to_ft_stab(methods[key]['options'], key, eis_list)
                state.run(key, ft_stab, np.array([ramp.eval(step + i) for i in range(repeats)], dtype=float))
                step += repeats
                n_steps += repeats
                step_iteration += [iteration] * repeats
        if track_best and n_steps > loop_first_step:
            errs = state.main_errors(loop_first_step, n_steps - loop_first_step)
            for err, it in zip(errs, step_iteration):
                better = best_err > err
                best_err = np.where(better, err, best_err)
                best_iter = np.where(better, it, best_iter)
        reselect = best_iter > lo.get('best_density_not_in_first_n_iterations', np.inf)
        if reselect.any():
            state.select_best(reselect)
        iterations.append(iteration)
    return iterations, n_steps
