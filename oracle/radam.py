"""Oracle restatement of RAdam.step (ZEGGS/optimizers.py:31-99) in numpy, in the dtype of the arrays it is given.

float32 arrays: every scalar is rounded to float32 where the reference's float32 kernels round it (the restatement the fixtures
pin).  float64 arrays: the betas, their complements, eps and the step scalars stay Python doubles -- the yardstick.

TEST INFRASTRUCTURE -- see oracle/__init__.py.
"""
import math

import numpy as np


def radam_scalars(step, lr, beta1=0.9, beta2=0.999, degenerated_to_sgd=True):
    """Host scalars of optimizers.py:64-84 for a given (1-based) step count.
    Returns (rectified: bool, step_scale) where the update is
      rectified : p -= step_scale * m / (sqrt(v) + eps)
      otherwise : p -= step_scale * m          (degenerated_to_sgd=True)
      otherwise : no update at all, step_scale None (degenerated_to_sgd=False: optimizers.py:82-83, step_size = -1)"""
    beta2_t = beta2 ** step
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n_sma = n_max - 2.0 * step * beta2_t / (1.0 - beta2_t)
    if n_sma >= 5:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma
                              * n_max / (n_max - 2)) / (1 - beta1 ** step)
        return True, step_size * lr
    if not degenerated_to_sgd:
        return False, None
    return False, lr / (1 - beta1 ** step)


def radam_step(p, g, m, v, step, lr, eps, beta1=0.9, beta2=0.999, weight_decay=0.0, degenerated_to_sgd=True):
    """In-place update of arrays p, m, v (all float32 or all float64) with gradient g (step is 1-based).  weight_decay:
    optimizers.py:88-95 (p += -weight_decay * lr * p before the update, in the branches that apply one;
    degenerated_to_sgd=True applies a step in both branches, False none before the rectified one).
    float64 torch tensors (on any device) are taken as well: the whole flat buffer of an engine is 25 M elements."""
    if isinstance(p, np.ndarray):
        f, sqrt = p.dtype.type, np.sqrt
        assert p.dtype == m.dtype == v.dtype and p.dtype in (np.float32, np.float64)
        g = g.astype(p.dtype, copy=False)
    else:
        import torch
        f, sqrt = float, torch.sqrt
        assert p.dtype == m.dtype == v.dtype == g.dtype == torch.float64
    v *= f(beta2)
    v += f(1 - beta2) * g * g                       # addcmul_(grad, grad, value=1-beta2)
    m *= f(beta1)
    m += f(1 - beta1) * g                           # add_(grad, alpha=1-beta1)
    rect, scale = radam_scalars(step, lr, beta1, beta2, degenerated_to_sgd)
    if scale is None:
        return p, m, v
    if weight_decay != 0:
        p += f(-weight_decay * lr) * p                # add_(p, alpha=-weight_decay * lr)
    if rect:
        p += f(-scale) * (m / (sqrt(v) + f(eps)))  # addcdiv_(m, sqrt(v)+eps, value=-step*lr)
    else:
        p += f(-scale) * m
    return p, m, v


# ---- the input recipe of tests/golden/radam_steps.npz (oracle/make_golden.py: gold_radam_steps) and of the kernel tests at other
# sizes: gradients whose magnitudes span what training meets (every element has a magnitude of its own, log-uniform over
# 1e-9 ... 10, and its draws stay within a factor of 10 -- so sqrt(v) ~ 0.08 |g| lies below eps = 1e-5 for half of the elements and
# above it for the other half at the rectified steps), elements that never see a gradient and elements that miss one step.
def recipe(n, steps, seed, n_never=8, n_once=8):
    """-> p0 [n] float32, grads [steps, n] float32, never (indices whose gradient is zero at every step), once ((index, step))"""
    rng = np.random.default_rng(seed)
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(np.float32)
    mag = 10.0 ** (rng.uniform(-8.5, 0.5, n)[None, :] + rng.uniform(-0.5, 0.5, (steps, n)))
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)[None, :] * np.where(rng.random((steps, n)) < 0.25, -1.0, 1.0)
    g = (mag * sign).astype(np.float32)
    n_never, n_once = min(n_never, n // 4), min(n_once, n // 4)
    pick = rng.permutation(n)[:n_never + n_once]
    never, once_i = np.sort(pick[:n_never]), pick[n_never:]
    once = [(int(i), int(rng.integers(0, steps))) for i in once_i]
    g[:, never] = 0
    for i, t in once:
        g[t, i] = 0
    return p0, g, never, once
