"""The cases of tests/test_hip_q8_spec_model_tree.py: trees from a draft model over the (target <- draft) pairs, fixtures
and shapes of tests/spec_model_cases.py.  No GPU, nothing of rama_amd imported."""
from tests.spec_model_cases import PAIRS, SAMPLERS  # noqa: F401  (the pairs and samplers are that file's)

# (K, B, R): a one-level tree; the header's example; three choices per trunk node; R cuts the sides short; R cuts the trunk short
GRID = [(1, 2, 16), (4, 2, 16), (3, 3, 16), (7, 2, 8), (7, 4, 2)]

# the linear chain again: B = 1, R = K + 1 against rama_q8_spec_begin_model on the same inputs
LINE = [(1, "untied<-untied"), (7, "untied<-untied"), (7, "synth15m<-near"), (2, "untied<-tied")]

# THE COVERAGE CONDITION.  Between them the recorded cases' replays must show a step with a == 0, one with a == cap, one with 0 < a < cap, a
# catch-up row, and a step that accepts a node off the trunk.  A model drafting for itself accepts its trunk whole (a == cap, catch-up rows);
# two unrelated models accept next to nothing (a == 0).  Off the trunk: the near-copy pair agrees greedy, and at temperature 1 its 32 000
# logits are too flat for the target's pick ever to be the draft's next choice, so OFF_TRUNK samples at a low temperature, where now and
# then the running sum crosses u * total between the first and the second token for one model and not for the other.  Its context seed and
# sampler were chosen on the CPU with tests/q8_ref.py as both models' logits (8 seeds x 4 samplers searched); the counts are that replay's:
# (steps, accepted, off_trunk_accepted) per (K, B, R) of the grid.  test_every_outcome_occurs replays the cases and fails if an input drifts.
COVERAGE = ("zero", "full", "partial", "catch_up", "off_trunk")
OFF_TRUNK = dict(pair="synth15m<-near", context_seed=1, sampler=(0.08, 0.9, 0.6),
                 counts={(1, 2, 16): (12, 12, 1), (4, 2, 16): (5, 19, 0), (3, 3, 16): (6, 18, 3), (7, 2, 8): (4, 20, 0), (7, 4, 2): (13, 11, 0)})
