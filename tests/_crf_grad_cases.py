"""The data of the trainable-CRF tests (tests/test_crf_grad_cpu.py and tests/test_gpu_crf_grad.py): ``_crf_cases.bounded_cases`` -- every K
and radius, C in {2, 3, 8}, T in {1, 2, 5}, Potts and the non-symmetric mu, binary and two-plane input, every frame -- with an output and a
seeded gradient of the output per case.  A case's reference and bound are computed once and shared (``reference``, ``bound``)."""
import functools

import numpy as np

import _crf_cases as K

OUTPUTS = ("logit", "prob")


def grad_cases():
    """``_crf_cases.bounded_cases`` with an output each, drawn so that binary and two-plane input, Potts and mu meet both outputs:
    ``(name, case, output)``."""
    out = []
    for i, case in enumerate(K.bounded_cases()):
        output = OUTPUTS[(i + i // 3 + i // 12) % 2]
        out.append((f"{case[0]}-{output}", case, output))
    return out


def case_inputs(gcase):
    """``(unary, guide, grad_output in the output's (= the unaries') shape, the keyword arguments of crf_backward_reference)``."""
    name, case, output = gcase
    unary, guide, kw = K.case_inputs(case)
    g = np.random.RandomState(900 + sum(map(ord, name))).randn(*unary.shape).astype(np.float32)
    return unary, guide, g, dict(output=output, **kw)


@functools.lru_cache(maxsize=None)
def _by_name(name):
    return next(c for c in grad_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    from hyperpri_amd import crf
    unary, guide, g, kw = case_inputs(_by_name(name))
    return crf.crf_backward_reference(unary, guide, g, **kw)


@functools.lru_cache(maxsize=None)
def bound(name):
    from hyperpri_amd import crf
    unary, guide, g, kw = case_inputs(_by_name(name))
    return crf.crf_grad_bound(unary, guide, g, **kw)


def fp64_grad_tolerance(n, C, T, w_total, mu_sum, u_max, g_max):
    """What two fp64 evaluations of the backward may differ by, u = 2^-53: ``(per element of dU, per pixel of a parameter's sum)``.  One
    iteration maps gL^t to gL^(t-1) with a gain of at most ``2 w_total mu_sum`` (the gather's weights sum to at most ``4 w_total`` -- a
    corner neighbour's n_i - 1 is a quarter of n - 1 --, ``mu^T``'s absolute column sums to ``mu_sum``, ``|Q (x - <Q, x>)| <= max|x| / 2``)
    and adds ``(n + 2 C + 16) u`` of that magnitude plus three times what the two forwards' Q differ by (``fp64_tolerance``)."""
    u = 2.0 ** -53
    dq = K.fp64_tolerance(n, C, T, w_total, max(mu_sum, 1.0), u_max)
    gain = max(2.0 * w_total * mu_sum, 1.0)
    rel = (n + 2 * C + 16) * u + 3 * dq
    mag, err, sum_mag, sum_err, per_pixel = g_max, rel * g_max, g_max, rel * g_max, 0.0
    for _ in range(T):
        per_pixel += 4 * mu_sum * max(1.0, w_total) * (err + rel * mag)
        err = gain * (err + rel * mag)
        mag = gain * mag
        sum_mag += mag
        sum_err += err
    return sum_err + (T + 1) * u * sum_mag, per_pixel
