"""Sequential float64 restatement of gradient clipping by global norm (learner.grad_norm: hh_grad_norm; learner.adam_step(clip=...):
hh_adam_step_clipped), written from the formulas of include/hh_learner.h and from nothing in the learner package, and the tests' gradient lists.
No test in here."""
import numpy as np

U = 2.0 ** -53      # float64's unit roundoff


def norm_coef(grads, max_norm):
    """-> (norm, coef) as Python floats: norm = sqrt(sum of float64(g)^2 over every element of every array, added one after the other in
    list order), coef = min(1, max_norm / (norm + 1e-6))"""
    total = np.float64(0.0)
    for g in grads:
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        if g.size:
            total = np.cumsum(np.concatenate(([total], g * g)))[-1]      # cumsum adds sequentially: ((total + g0^2) + g1^2) + ...
    norm = float(np.sqrt(total))
    return norm, min(1.0, float(max_norm) / (norm + 1e-6))


def bound(grads):
    """the relative bound on a float64 sum of n non-negative terms in any order (and so on the norm): n x 2^-53, n at least 1"""
    return max(1, sum(int(np.asarray(g).size) for g in grads)) * U


def scaled(grads, coef):
    """what hh_adam_step_clipped reads: float32(float64(g) * coef), one rounding"""
    return [(np.asarray(g, dtype=np.float32).astype(np.float64) * float(coef)).astype(np.float32) for g in grads]


HEAD_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193, 0)      # around the float4 group and the 4096-element tile, and an empty tensor


def grad_list(n_small, seed, last_scale=1e3):
    """float32 gradients: HEAD_SIZES, then n_small tensors of 1..40 elements; standard normal, the LAST tensor scaled by last_scale so
    that the largest gradients sit at the end of the list (a norm taken per launch, or without the last launch, misses them)"""
    rng = np.random.default_rng(seed)
    sizes = HEAD_SIZES + tuple(1 + (7 * i) % 40 for i in range(n_small))
    out = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    out[-1] = (out[-1] * np.float32(last_scale)).astype(np.float32)
    return out
