"""Learning-rate schedules of the reference's utils/general_utils.py, restated.

`get_expon_lr_func` is what scene/gaussian_model.py:625-661 builds its xyz / grid / deformation / posenet schedules from
and what update_learning_rate(iteration) evaluates every iteration (train.py:312-313).  Host arithmetic in float64 with
numpy's exp / log / sin, statement by statement as the reference forms it: mobgs_amd.optim.DeviceAdam tabulates these
values once and the device indexes the table, so the rate a step runs with is the rate the eager loop would have set.
"""
from __future__ import annotations

import numpy as np


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """-> rate(step): lr_init at step 0, lr_final from max_steps on, interpolated linearly in the logarithm between
    them (an exponential decay).  step < 0, or both rates zero: 0.0 (the group is switched off).  lr_delay_steps > 0: the
    rate is scaled by lr_delay_mult + (1 - lr_delay_mult) sin(pi / 2 clip(step / lr_delay_steps, 0, 1)), i.e. it starts
    at lr_init * lr_delay_mult and is eased back to the plain decay over the first lr_delay_steps steps."""

    def rate(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            ease = np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
            delay = lr_delay_mult + (1 - lr_delay_mult) * ease
        else:
            delay = 1.0
        t = np.clip(step / max_steps, 0, 1)
        return delay * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)

    return rate
