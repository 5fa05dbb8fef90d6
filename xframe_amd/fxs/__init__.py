"""Host-side mirror of ``xframe.projects.fxs`` for the reconstruct (MTIP phasing) path."""
from . import simulate_ccd                                              # noqa: E402,F401  (the worker `fxs simulate_ccd`)
from .simulate_ccd import (deg2_invariant_to_cc, deg2_invariant_to_cc_2d, density_to_deg2_invariants,  # noqa: E402,F401
                           shape_density)
