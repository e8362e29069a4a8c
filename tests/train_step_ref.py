"""Float64 / plain-numpy restatements that the train-step tests hold the device code against (learner.adam_step: hh_adam_step,
learner.minibatch_stage: hh_minibatch_stage), written from the formulas of include/hh_learner.h and from nothing in the learner package."""
import math

import numpy as np


def adam_ref(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """one step of Adam (amsgrad = False, weight_decay = 0) in float64: arrays in, NEW arrays out; t = the steps taken so far
    -> (p, m, v).  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t')) m / (sqrt(v) / sqrt(1 - b2^t') + eps), t' = t + 1"""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    step = int(t) + 1
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
    return p, m, v


def stage_ref(col, cap, row):
    """one column [S, ...] (numpy, any dtype) staged by the schedule row (first chunk, last chunk + 1, n_valid, 0): -> [cap, ...], the
    chunks first, zero bytes behind them"""
    s0, s1 = int(row[0]), int(row[1])
    col = np.asarray(col)
    out = np.zeros((int(cap),) + col.shape[1:], dtype=col.dtype)
    out[:s1 - s0] = col[s0:s1]
    return out


def adam_inputs(sizes, seed, offset_of=None):
    """gradients for the Adam tests: |g| in {0} u [1e-6, 1e3] (log-uniform), mixed signs, about one element in eight exactly 0;
    parameters of order 0.1.  -> per size (p, list of five g) as float32 arrays"""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        p = (0.1 * rng.standard_normal(n)).astype(np.float32)
        gs = []
        for _ in range(5):
            mag = 10.0 ** rng.uniform(-6.0, 3.0, n)
            g = mag * rng.choice([-1.0, 1.0], n) * (rng.random(n) >= 0.125)
            gs.append(g.astype(np.float32))
        out.append((p, gs))
    return out
