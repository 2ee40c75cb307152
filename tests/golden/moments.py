"""Deterministic AdamW moments shared by the fixture generator (dev container, live reference) and the parity tests
(GPU box), the way weights.fill_state shares the weights: the same (seed, name) always gives the same pair, so no
optimiser state is stored in a fixture.

The protocol fixtures take their ONE AdamW step from this state at step count STEPS_BEFORE, not from a fresh optimiser.
A first step from zero moments is lr * g / (|g| + eps): where a gradient is analytically zero (a bias in front of the
head's training-mode BatchNorm(256); a head column whose four rows are all kept and all past the ReLU, whose gradient is
the batch sum that BatchNorm's backward makes zero) its rounding noise, a few 1e-8 after the clip coefficient and of
either sign, is of the size of eps, and the reference's parameter after the step is anywhere in [-lr, +lr] around the one
before -- a figure of the reference's rounding, which nothing reproduces.  With second moments of the gradients' own
scale the step is smooth in g (d step / d g ~ 1e-4 here), so the parameters after it are a property of the model and the
AdamW tolerance applies to every element."""
import zlib

import numpy as np

STEPS_BEFORE = 10


def fill_moments(name, shape, seed):
    """(exp_avg, exp_avg_sq) of parameter `name`, fp32: first moments of the clipped gradients' size, second moments
    around 1e-4 (gradients around 1e-2)."""
    rng = np.random.default_rng([seed, zlib.crc32(name.encode()), STEPS_BEFORE])
    exp_avg = 5e-3 * rng.standard_normal(shape)
    exp_avg_sq = rng.uniform(0.5e-4, 1.5e-4, shape)
    return exp_avg.astype(np.float32), exp_avg_sq.astype(np.float32)
