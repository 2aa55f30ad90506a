"""Per-exit temperature scaling: the host restatements, the deterministic search and the loader-level fit.

Temperature scaling is the one-scalar-per-classifier post-hoc calibration (Guo et al. 2017; the subject of the Mix-n-Match code the
reference's ECE evaluator comes from, SA/train/results_analyzer.py:53): exit e's probabilities become ``softmax(logits / tau_e)``.  With
Monte-Carlo sampling the prediction is the T-mean of the per-sample softmax, which is NOT a function of the untempered mean — the
temperature has to act where the per-sample softmax exists, inside the fused exit head (``MCDEngine.set_temperature``) — and the objective
of the fit is the NLL of that mean,

    nll(tau) = sum_b -log( (1/T) sum_t softmax(l_tb / tau)[y_b] ),

evaluated on the device for a grid of candidates per exit in one launch (``MCDEngine.nll_grid``, bmi_nll_temperature_grid).  The reference
has no temperature scaling; it saves the validation predictions (``save_validation``) this step is fitted on.

* ``nll_grid_numpy``  — float64 restatement of the device objective (what host users and the tests call).
* ``temper_logits``   — mean / var of the tempered per-sample softmax, the restatement of what the head computes under a temperature.
* ``zoom_search``     — the deterministic per-exit search, all exits evaluated in the same launch.
* ``TemperatureScaling`` — walks a labelled loader once, keeps the split's raw logits on the device, searches, applies, saves.

Members calibrated one by one do not give a calibrated mean.  The exit ensemble (``predict_ensemble``: per sample the mean of exits
0..e) is formed from the tempered members, and the JOINT fit minimises the ensemble's own NLL,

    nll_e(tau) = sum_b -log( 1 / (T (e + 1)) sum_{i <= e} sum_t softmax(l_tib / tau_i)[y_b] ),

evaluated on the device for a grid of candidates of one coordinate (or of one shared temperature) in one launch
(``MCDEngine.ensemble_nll_grid``, bmi_nll_ensemble_temperature_grid).

* ``ensemble_nll_grid_numpy`` — float64 restatement of that objective.
* ``coordinate_search``  — coordinate descent (``zoom_search`` per coordinate) or one shared temperature, on row ``target``.
* ``EnsembleTemperatureScaling`` — the loader-level joint fit, on the same walk as ``TemperatureScaling``.

Equal weights are the wrong prior where the early exits are much weaker than the late ones.  The WEIGHTED exit ensemble is
q_te = sum_{i<=e} W[e][i] p_ti (``MCDEngine.set_ensemble_weights``); its T-mean is sum_i W[e][i] mean_i, so the likelihood of a weight row
depends only on the table A[i][n] = mean_t p_{t,i,n}(y_n) — the label's entry of the T-mean softmax ``predict`` already returns — and

    nll_e(w) = sum_n -log( sum_{i<=e} w_i A[i][n] )

is convex in w: EM on the [E, N] table is exact and monotone, runs on the host, and keeps no per-sample logits (no ``max_logit_bytes``).

* ``mixture_weights_em`` — the EM iteration for one row.
* ``EnsembleWeights``    — the loader-level fit: the walk of ``TemperatureScaling``, the table gathered on the device, EM per row.

One scalar per exit cannot correct class-wise miscalibration.  VECTOR SCALING (Guo et al. 2017) gives every exit a per-class scale and
bias, z_c = a_c * l_c + b_c (``MCDEngine.set_vector_scaling``: two rounded fp32 operations inside the fused head, in place of the
temperature's product; never both), fitted on the same objective with z in place of l / tau,

    nll_e(a, b) = sum_n -log( (1/T) sum_t softmax(a * l_tn + b)[y_n] ),

whose value and gradient come from the device in one call for all exits (``MCDEngine.nll_vector_grad``, bmi_nll_vector_scaling_grad).

* ``scale_logits``     — mean / var of the scaled per-sample softmax, the restatement of what the head computes under a vector scaling.
* ``nll_vector_numpy`` — float64 restatement of the device objective, value and both gradients.
* ``lbfgs_minimize``   — a small deterministic L-BFGS with Armijo backtracking, the exits as independent problems in the same evaluations.
* ``VectorScaling``    — the loader-level fit, on the same walk as ``TemperatureScaling``, started at the scalar fit.

Neither map can move probability mass BETWEEN classes: a model that systematically confuses class i with class j — what the early exits
of a multi-exit network do — needs MATRIX SCALING (Guo et al. 2017), z = M l + b with a full [C, C] matrix per exit
(``MCDEngine.set_matrix_scaling``: inside the fused head, per class the products in ascending j, each rounded to fp32, added one by one;
never beside the other two maps, which are its special cases).  Its C^2 + C parameters per exit overfit a small split, so the
fit carries the off-diagonal and bias regulariser of Kull et al. 2019 (ODIR); the same bias term is ``VectorScaling.fit``'s ``bias_l2``.

* ``matrix_z`` / ``matrix_logits`` — the fp32 z of the matrix-scaled head, exactly, and mean / var of its softmax.
* ``nll_matrix_numpy`` — float64 restatement of the device objective (``MCDEngine.nll_matrix_grad``, bmi_nll_matrix_scaling_grad).
* ``odir_penalty``     — the regulariser, value and gradients, host float64.
* ``MatrixScaling``    — the loader-level fit, started at the vector fit; ``select`` picks the regulariser on a hold-out loader.

THE ORDER: fit the temperatures (``TemperatureScaling`` or ``EnsembleTemperatureScaling``) OR the vector scaling (``VectorScaling``) OR the
matrix scaling (``MatrixScaling``) first,
``apply()``, then fit the weights AT those members — they are then fixed and the problem is convex (``EnsembleWeights`` reads ``predict``'s
means, so it needs no change: weights fitted after ``VectorScaling.apply()`` are fitted at the scaled members).  The joint temperature
fit's objective stays the equal-weight ensemble's; a joint fit of weights and temperatures, or of weights and a vector scaling, is not built.
"""
import numpy as np
import torch

from .results_analyzer import get_device


def _inv32(tau):
    """float32(1 / float64(float32 tau)): the factor the exit heads multiply by."""
    return (1.0 / np.asarray(tau, dtype=np.float32).astype(np.float64)).astype(np.float32)


def nll_grid_numpy(logits, labels, tau_grid):
    """float64 [E, G]: sum_b -log mean_t softmax(l_tb / tau_eg)[y_b] for ``logits`` [T, E, B, C], ``labels`` [B], ``tau_grid`` [E, G] (taken
    as float32, like the device's).  bmi_nll_temperature_grid's arithmetic step by step, in log-sum-exp form (no clip; finite for any
    finite logits):  z = float64(l) * (1.0 / float64(tau));  a_t = (z_y - max_c z) - log sum_c exp(z_c - max_c z);
    term_b = -(logsumexp_t a_t - log T)."""
    logits = np.asarray(logits)
    T, E, B, C = logits.shape
    labels = np.asarray(labels).astype(np.int64).reshape(B)
    if labels.min() < 0 or labels.max() >= C:
        raise ValueError(f"labels must lie in [0, {C})")
    inv = 1.0 / np.asarray(tau_grid, dtype=np.float32).astype(np.float64)
    if inv.ndim != 2 or inv.shape[0] != E:
        raise ValueError(f"tau_grid must be [E, G] with E = {E}")
    out = np.zeros(inv.shape)
    idx = np.arange(B)
    for e in range(E):
        l = logits[:, e].astype(np.float64)                      # [T, B, C]
        for g in range(inv.shape[1]):
            z = l * inv[e, g]
            zmax = z.max(-1)
            a = (z[:, idx, labels] - zmax) - np.log(np.exp(z - zmax[..., None]).sum(-1))       # [T, B]
            am = a.max(0)
            lse = am + np.log(np.exp(a - am).sum(0))
            out[e, g] = np.sum(-(lse - np.log(float(T))))
    return out


def _vary_list(vary, n_exits):
    idx = [] if vary is None else [int(vary)] if np.ndim(vary) == 0 else [int(i) for i in vary]
    if any(i < 0 or i >= n_exits for i in idx):
        raise ValueError(f"vary: exit indices must lie in [0, {n_exits}), got {idx}")
    return idx


def ensemble_nll_grid_numpy(logits, labels, tau, vary, cand):
    """float64 [E, G]: row e is sum_b -log of the mean over exits 0..e and the T samples of softmax(l / tau_i(g))[y_b], for ``logits``
    [T, E, B, C], ``labels`` [B], ``tau`` [E] (or a scalar), ``vary`` (an exit index, an iterable of indices, or None) and ``cand`` [G],
    temperatures taken as float32 like the device's: tau_i(g) = cand[g] for the exits in ``vary``, tau[i] for the others.
    bmi_nll_ensemble_temperature_grid's arithmetic step by step (no clip; finite for any finite logits):
    z = float64(l) * (1.0 / float64(tau_i(g)));  a_ti = (z_y - max_c z) - log sum_c exp(z_c - max_c z);  L_i = logsumexp_t a_ti;
    R_0 = L_0, R_e = m + log(exp(R_{e-1} - m) + exp(L_e - m)) with m = max(R_{e-1}, L_e);  term_e = -(R_e - log(T (e + 1)))."""
    logits = np.asarray(logits)
    T, E, B, C = logits.shape
    labels = np.asarray(labels).astype(np.int64).reshape(B)
    if labels.min() < 0 or labels.max() >= C:
        raise ValueError(f"labels must lie in [0, {C})")
    tau = np.asarray(tau, dtype=np.float32).reshape(-1)
    tau = np.repeat(tau, E) if tau.size == 1 else tau
    if tau.size != E:
        raise ValueError(f"tau must hold one value per exit ({E})")
    cand = np.asarray(cand, dtype=np.float32).reshape(-1)
    varied = set(_vary_list(vary, E))
    inv_tau, inv_cand = 1.0 / tau.astype(np.float64), 1.0 / cand.astype(np.float64)
    idx = np.arange(B)

    def lse_samples(l, inv):                                     # L [B] of one exit at one temperature
        z = l * inv
        zmax = z.max(-1)
        a = (z[:, idx, labels] - zmax) - np.log(np.exp(z - zmax[..., None]).sum(-1))       # [T, B]
        am = a.max(0)
        return am + np.log(np.exp(a - am).sum(0))

    ls = [logits[:, i].astype(np.float64) for i in range(E)]
    fixed = {i: lse_samples(ls[i], inv_tau[i]) for i in range(E) if i not in varied}
    out = np.zeros((E, cand.size))
    for g in range(cand.size):
        R = None
        for e in range(E):
            L = lse_samples(ls[e], inv_cand[g]) if e in varied else fixed[e]
            if R is None:
                R = L
            else:
                m = np.maximum(R, L)
                R = m + np.log(np.exp(R - m) + np.exp(L - m))
            out[e, g] = np.sum(-(R - np.log(float(T) * float(e + 1))))
    return out


def temper_logits(logits, tau):
    """(mean, var), float64 [E, B, C]: over the T samples of ``logits`` [T, E, B, C], the mean and the variance (ddof = 0) of
    softmax(float32(l * inv_e)), inv_e = float32(1 / tau_e) — the fp32 product the exit head forms, the softmax in float64.  ``tau``: one
    value per exit or a scalar."""
    logits = np.asarray(logits)
    E = logits.shape[1]
    inv = np.broadcast_to(_inv32(tau).reshape(-1), (E,))
    z = (logits.astype(np.float32) * inv.reshape(1, E, 1, 1)).astype(np.float64)
    z -= z.max(-1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(-1, keepdims=True)
    return p.mean(0), p.var(0)


def scale_logits(logits, scale, bias=None):
    """(mean, var), float64 [E, B, C]: over the T samples of ``logits`` [T, E, B, C], the mean and the variance (ddof = 0) of
    softmax(float32(float32(l * scale) + bias)) — the two rounded fp32 operations the exit head forms under a vector scaling, the softmax in
    float64 like ``temper_logits``.  ``scale`` / ``bias``: [E, C], or [C] for every exit; ``bias`` None = zeros."""
    from ..engine import check_vector_scaling
    logits = np.asarray(logits)
    E, C = logits.shape[1], logits.shape[3]
    a, b = check_vector_scaling(scale, bias, E, C)
    z = (logits.astype(np.float32) * a[None, :, None, :]).astype(np.float32)
    z = (z + b[None, :, None, :]).astype(np.float32).astype(np.float64)
    z -= z.max(-1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(-1, keepdims=True)
    return p.mean(0), p.var(0)


def nll_vector_numpy(logits, labels, scale, bias):
    """(nll [E], g_scale [E, C], g_bias [E, C]), float64: value and gradient of sum_b -log mean_t softmax(l_tb * scale_e + bias_e)[y_b] for
    ``logits`` [T, E, B, C], ``labels`` [B], ``scale`` / ``bias`` [E, C] taken as float64.  bmi_nll_vector_scaling_grad's arithmetic in
    log-sum-exp form:  z = float64(l) * a + b;  A_t = (z_y - max_c z) - log sum_c exp(z_c - max_c z);  term_b = -(logsumexp_t A_t - log T);
    r_t = exp(A_t) / sum_t' exp(A_t'),  p_t = softmax(z_t):  d term / d b_c = sum_t r_t (p_tc - [c == y]),  d term / d a_c the same with a
    factor l_tc.  sum_c g_bias = 0 identically."""
    logits = np.asarray(logits)
    T, E, B, C = logits.shape
    labels = np.asarray(labels).astype(np.int64).reshape(B)
    if labels.min() < 0 or labels.max() >= C:
        raise ValueError(f"labels must lie in [0, {C})")
    a = np.asarray(scale, dtype=np.float64)
    b = np.asarray(bias, dtype=np.float64)
    if a.shape != (E, C) or b.shape != (E, C):
        raise ValueError(f"scale and bias must be [E, C] = [{E}, {C}]")
    idx = np.arange(B)
    hot = np.zeros((B, C))
    hot[idx, labels] = 1.0
    nll, ga, gb = np.zeros(E), np.zeros((E, C)), np.zeros((E, C))
    for e in range(E):
        l = logits[:, e].astype(np.float64)                      # [T, B, C]
        z = l * a[e] + b[e]
        zmax = z.max(-1)
        ex = np.exp(z - zmax[..., None])
        s = ex.sum(-1)
        A = (z[:, idx, labels] - zmax) - np.log(s)               # [T, B]
        am = A.max(0)
        w = np.exp(A - am)
        S = w.sum(0)
        nll[e] = np.sum(-((am + np.log(S)) - np.log(float(T))))
        d = (w / S)[..., None] * (ex / s[..., None] - hot)        # [T, B, C]
        gb[e] = d.sum((0, 1))
        ga[e] = (d * l).sum((0, 1))
    return nll, ga, gb


def matrix_z(logits, matrix, bias=None):
    """float32 [T, E, B, C]: the logits of ``logits`` [T, E, B, C] under a matrix scaling, bit for bit what the exit head forms
    (csrc/head_fused_body.h, TEMP == 3): per output class c, acc = fl32(M[c][0] * l_0), then acc = fl32(acc + fl32(M[c][j] * l_j)) for j
    ascending, then fl32(acc + b[c]) — a loop over j on float32 arrays (numpy rounds every elementwise operation, nothing is fused), not
    ``@``, whose summation order is not this one.  ``matrix`` / ``bias`` as ``engine.check_matrix_scaling`` takes them."""
    from ..engine import check_matrix_scaling
    l = np.asarray(logits, dtype=np.float32)
    if l.ndim != 4:
        raise ValueError("logits must be [T, E, B, C]")
    E, C = l.shape[1], l.shape[3]
    M, b = check_matrix_scaling(matrix, bias, E, C)
    if M is None:
        return l
    z = np.empty_like(l)
    for e in range(E):
        le = l[:, e]                                             # [T, B, C]
        acc = (M[e][:, 0] * le[..., 0:1]).astype(np.float32)     # [T, B, C]: entry c = M[c][0] * l_0
        for j in range(1, C):
            acc = (acc + (M[e][:, j] * le[..., j:j + 1]).astype(np.float32)).astype(np.float32)
        z[:, e] = (acc + b[e]).astype(np.float32)
    return z


def matrix_logits(logits, matrix, bias=None):
    """(mean, var), float64 [E, B, C]: over the T samples of ``logits`` [T, E, B, C], the mean and the variance (ddof = 0) of
    softmax(``matrix_z``) — the head's fp32 z exactly, the softmax in float64 like ``scale_logits``.  A diagonal matrix gives
    ``scale_logits``' result bit for bit."""
    z = matrix_z(logits, matrix, bias).astype(np.float64)
    z -= z.max(-1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(-1, keepdims=True)
    return p.mean(0), p.var(0)


def nll_matrix_numpy(logits, labels, matrix, bias):
    """(nll [E], g_matrix [E, C, C], g_bias [E, C]), float64: value and gradient of sum_b -log mean_t softmax(M_e l_tb + bias_e)[y_b] for
    ``logits`` [T, E, B, C], ``labels`` [B], ``matrix`` [E, C, C] (row = output class) and ``bias`` [E, C] taken as float64.
    bmi_nll_matrix_scaling_grad's arithmetic:  z_c = ((0.0 + float64(l_0) * M[c][0]) + float64(l_1) * M[c][1] + ...) + b[c], a loop over j
    ascending (not ``@``), so z is the kernel's;  A_t, term_b, r_t and p_t as in ``nll_vector_numpy``;  d_tc = r_t (p_tc - [c == y]):
    d term / d b_c = sum_t d_tc,  d term / d M[c][j] = sum_t d_tc l_tj.  On a diagonal matrix the value, g_bias and the diagonal of g_matrix
    are ``nll_vector_numpy``'s, exactly.  sum_c g_bias = 0 and sum_c g_matrix[c][j] = 0 identically (the softmax gauge)."""
    logits = np.asarray(logits)
    T, E, B, C = logits.shape
    labels = np.asarray(labels).astype(np.int64).reshape(B)
    if labels.min() < 0 or labels.max() >= C:
        raise ValueError(f"labels must lie in [0, {C})")
    M = np.asarray(matrix, dtype=np.float64)
    b = np.asarray(bias, dtype=np.float64)
    if M.shape != (E, C, C) or b.shape != (E, C):
        raise ValueError(f"matrix must be [E, C, C] = [{E}, {C}, {C}] and bias [E, C] = [{E}, {C}]")
    idx = np.arange(B)
    hot = np.zeros((B, C))
    hot[idx, labels] = 1.0
    nll, gM, gb = np.zeros(E), np.zeros((E, C, C)), np.zeros((E, C))
    for e in range(E):
        l = logits[:, e].astype(np.float64)                      # [T, B, C]
        z = np.zeros((T, B, C))
        for j in range(C):
            z = z + l[..., j:j + 1] * M[e][:, j]
        z = z + b[e]
        zmax = z.max(-1)
        ex = np.exp(z - zmax[..., None])
        s = ex.sum(-1)
        A = (z[:, idx, labels] - zmax) - np.log(s)               # [T, B]
        am = A.max(0)
        w = np.exp(A - am)
        S = w.sum(0)
        nll[e] = np.sum(-((am + np.log(S)) - np.log(float(T))))
        d = (w / S)[..., None] * (ex / s[..., None] - hot)        # [T, B, C]
        gb[e] = d.sum((0, 1))
        for j in range(C):                                       # (column j: the reduction nll_vector_numpy runs for its g_scale)
            gM[e][:, j] = (d * l[..., j:j + 1]).sum((0, 1))
    return nll, gM, gb


def odir_penalty(matrix, bias, n, off_diag_l2=0.0, bias_l2=0.0):
    """(value [E], grad_matrix [E, C, C], grad_bias [E, C]), host float64: the off-diagonal and bias regulariser of Kull et al. 2019 (ODIR)
    on the MEAN NLL, times ``n`` because the device objective is a sum over the n images,
        value_e = n ( off_diag_l2 / (C (C - 1)) sum_{c != j} M[e][c][j]^2  +  bias_l2 / C sum_c b[e][c]^2 ).
    It depends on the parameters only.  ``matrix`` None (``VectorScaling``'s bias term): no matrix term, grad_matrix None.  Zero on a
    diagonal matrix with ``bias_l2 = 0``."""
    b = np.asarray(bias, dtype=np.float64)
    E, C = b.shape
    n = float(n)
    value = n * (float(bias_l2) / C) * np.sum(b * b, axis=1)
    gb = (2.0 * n * float(bias_l2) / C) * b
    if matrix is None:
        return value, None, gb
    M = np.asarray(matrix, dtype=np.float64)
    if M.shape != (E, C, C):
        raise ValueError(f"matrix must be [E, C, C] = [{E}, {C}, {C}]")
    off = M * (1.0 - np.eye(C))
    lam = float(off_diag_l2) / (C * (C - 1)) if C > 1 else 0.0
    value = value + n * lam * np.sum(off * off, axis=(1, 2))
    return value, (2.0 * n * lam) * off, gb


def lbfgs_minimize(fun, x0, max_iter=100, gtol=1e-6, history=10, c1=1e-4, max_backtracks=30):
    """A small deterministic L-BFGS for P independent problems evaluated together: ``fun(x [P, D] float64) -> (f [P], g [P, D])``, every
    call evaluates all P problems (a problem that is not moving is evaluated where it stands).  Per problem: the two-loop recursion over
    the last ``history`` pairs (pairs with s.y <= 0 are skipped; a direction that is not a descent direction restarts from -g), then Armijo
    backtracking from step 1 (first iteration: 1 / max(1, |g|_inf)) by halving — a step is accepted only when f_new <= f + c1 t g.d, so
    every accepted iterate lowers the objective; non-finite values count as rejected.  A problem stops when |g|_inf <= ``gtol``
    (``converged``) or when ``max_backtracks`` halvings find no decrease (the step is below what float64 resolves: not ``converged``
    unless the gradient test holds); the run after ``max_iter`` iterations.

    Returns dict(x [P, D], f [P], g [P, D], iterations [P], converged bool [P], trace (list of f [P] after each iteration, trace[0] the
    start), n_eval)."""
    x = np.array(x0, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x0 must be [P, D]")
    P = x.shape[0]
    f, g = fun(x)
    f, g = np.array(f, dtype=np.float64).reshape(P), np.array(g, dtype=np.float64).reshape(x.shape)
    n_eval = 1
    S, Y = [[] for _ in range(P)], [[] for _ in range(P)]
    active = np.array([np.isfinite(f[p]) and np.max(np.abs(g[p])) > gtol for p in range(P)])
    converged = np.array([np.isfinite(f[p]) and np.max(np.abs(g[p])) <= gtol for p in range(P)])
    iterations = np.zeros(P, dtype=np.int64)
    trace = [f.copy()]
    for it in range(int(max_iter)):
        if not active.any():
            break
        d, gd, t = np.zeros_like(x), np.zeros(P), np.zeros(P)
        for p in np.flatnonzero(active):
            q = g[p].copy()
            alphas = []
            for s_, y_ in zip(reversed(S[p]), reversed(Y[p])):
                al = s_.dot(q) / y_.dot(s_)
                alphas.append(al)
                q -= al * y_
            if S[p]:
                q *= S[p][-1].dot(Y[p][-1]) / Y[p][-1].dot(Y[p][-1])
            for (s_, y_), al in zip(zip(S[p], Y[p]), reversed(alphas)):
                q += (al - y_.dot(q) / y_.dot(s_)) * s_
            d[p], gd[p] = -q, -q.dot(g[p])
            if not gd[p] < 0:
                S[p], Y[p] = [], []
                d[p], gd[p] = -g[p], -g[p].dot(g[p])
            t[p] = 1.0 if S[p] else 1.0 / max(1.0, float(np.max(np.abs(g[p]))))
        searching = active.copy()
        x_new, f_new, g_new = x.copy(), f.copy(), g.copy()
        for _ in range(int(max_backtracks)):
            trial = x.copy()
            for p in np.flatnonzero(searching):
                trial[p] = x[p] + t[p] * d[p]
            ft, gt = fun(trial)
            ft, gt = np.asarray(ft, dtype=np.float64).reshape(P), np.asarray(gt, dtype=np.float64).reshape(x.shape)
            n_eval += 1
            for p in np.flatnonzero(searching):
                if np.isfinite(ft[p]) and np.all(np.isfinite(gt[p])) and ft[p] <= f[p] + c1 * t[p] * gd[p]:
                    x_new[p], f_new[p], g_new[p] = trial[p], ft[p], gt[p]
                    searching[p] = False
                else:
                    t[p] *= 0.5
            if not searching.any():
                break
        for p in np.flatnonzero(active):
            if searching[p]:                                     # no decrease found: this problem ends where it stands
                active[p] = False
                continue
            s_, y_ = x_new[p] - x[p], g_new[p] - g[p]
            if s_.dot(y_) > 1e-12 * np.sqrt(s_.dot(s_) * y_.dot(y_)):
                S[p].append(s_)
                Y[p].append(y_)
                if len(S[p]) > history:
                    S[p].pop(0)
                    Y[p].pop(0)
            iterations[p] += 1
        x, f, g = x_new, f_new, g_new
        trace.append(f.copy())
        for p in range(P):
            if np.max(np.abs(g[p])) <= gtol:
                converged[p] = True
                active[p] = False
    return dict(x=x, f=f, g=g, iterations=iterations, converged=converged, trace=trace, n_eval=n_eval)


def _log_grid(lo, hi, n):
    """n log-spaced float32-representable points on [lo, hi] whose first and last are lo and hi THEMSELVES (exp(log(20)) is
    19.999999999999996, and at_bound compares for equality)."""
    if n < 2 or hi <= lo:
        return np.full(max(n, 1), lo)
    g = np.exp(np.linspace(np.log(lo), np.log(hi), n)).astype(np.float32).astype(np.float64)
    g[0], g[-1] = lo, hi
    return np.clip(g, lo, hi)


def zoom_search(eval_fn, n_exits, bracket=(0.05, 20.0), grid=33, rtol=1e-4, max_rounds=8, include=None):
    """Deterministic one-dimensional search per exit, every exit evaluated in the same call: ``eval_fn(tau [E, G] float64) -> nll [E, G]``.

    Round one evaluates a log-spaced grid of ``grid`` points over the bracket plus tau = 1 exactly; each later round puts a log-spaced
    grid on [left neighbour, right neighbour] of the best point so far (neighbours among everything evaluated for that exit, clamped at the
    bracket).  An exit stops when hi / lo - 1 <= rtol, the search when every exit has or after ``max_rounds``.  Returned is the argmin over
    EVERYTHING evaluated, so nll_after <= nll_before (the value at tau = 1) holds by construction.  Candidates are float32-representable
    (what the device evaluates and what an engine stores), the bracket's ends included: the ends are rounded to float32 once, and
    ``at_bound[e]`` says the returned point is one of them — the optimum lies outside the bracket, or the split does not determine it.

    ``include`` ([E] or a scalar, None: off) is appended to the candidates of EVERY round, as given (the caller's current point: the
    argmin is then never worse than it) — it is not clamped to the bracket, and ``nll_before`` stays the value at tau = 1.

    The search finds the basin of the coarse grid's minimum; the objective is NOT guaranteed unimodal in tau (a mixture over samples),
    and a narrower basin between two coarse points is not seen.  Non-finite objective values count as +inf.

    Returns dict(tau [E], nll_after [E], nll_before [E], at_bound bool [E], rounds)."""
    E, G = int(n_exits), int(grid)
    if G < 3:
        raise ValueError("grid must have at least 3 points")
    b_lo, b_hi = float(np.float32(bracket[0])), float(np.float32(bracket[1]))
    if not (0 < b_lo < b_hi and np.isfinite(b_hi)):
        raise ValueError(f"bracket must be 0 < lo < hi, got {bracket}")
    taus = [np.empty(0) for _ in range(E)]
    nlls = [np.empty(0) for _ in range(E)]
    lo, hi = np.full(E, b_lo), np.full(E, b_hi)
    nll_before = None
    rounds = 0
    extra = None if include is None else np.broadcast_to(np.asarray(include, dtype=np.float64).reshape(-1, 1), (E, 1))
    while rounds < max_rounds:
        cand = np.stack([_log_grid(lo[e], hi[e], G) for e in range(E)])
        if extra is not None:
            cand = np.concatenate([cand, extra], axis=1)
        if rounds == 0:
            cand = np.concatenate([cand, np.ones((E, 1))], axis=1)
        val = np.asarray(eval_fn(cand), dtype=np.float64).reshape(cand.shape)
        val = np.where(np.isfinite(val), val, np.inf)
        rounds += 1
        if nll_before is None:
            nll_before = val[:, -1].copy()
        done = True
        for e in range(E):
            t, v = np.concatenate([taus[e], cand[e]]), np.concatenate([nlls[e], val[e]])
            order = np.argsort(t, kind="stable")
            t, v = t[order], v[order]
            keep = np.concatenate([[True], t[1:] != t[:-1]])      # a tau evaluated twice gave the same value twice
            taus[e], nlls[e] = t[keep], v[keep]
            i = int(np.argmin(nlls[e]))
            lo[e] = min(max(taus[e][max(i - 1, 0)], b_lo), b_hi)
            hi[e] = max(min(taus[e][min(i + 1, len(taus[e]) - 1)], b_hi), b_lo)
            done = done and (hi[e] / lo[e] - 1.0 <= rtol)
        if done:
            break
    best = [int(np.argmin(nlls[e])) for e in range(E)]
    tau = np.array([taus[e][best[e]] for e in range(E)])
    return dict(tau=tau, nll_after=np.array([nlls[e][best[e]] for e in range(E)]), nll_before=nll_before,
                at_bound=np.array([t == b_lo or t == b_hi for t in tau]), rounds=rounds)


def coordinate_search(eval_fn, n_exits, target, init, mode="vector", sweep_rtol=1e-7, max_sweeps=50, **zoom):
    """Deterministic search of the temperatures of exits 0..``target`` on row ``target`` of the ensemble objective:
    ``eval_fn(tau [E] float64, vary, cand [G] float64) -> nll [E, G]`` (``ensemble_nll_grid_numpy``'s signature behind the logits).

    ``mode="vector"``: sweeps over the coordinates 0..target, each step a ``zoom_search`` (keyword arguments ``zoom``) over that one
    exit's temperature with the others held; the coordinate's current value is among the candidates of every round
    (``zoom_search(include=)``), so no step increases the objective.  The search stops when a whole sweep improves row ``target`` by at
    most ``sweep_rtol`` relative (``stopped_by_rule``), or after ``max_sweeps``.  ``mode="shared"``: ONE ``zoom_search`` with every exit
    0..target in the mask — one temperature for the ensemble's members (``sweeps`` = 1, ``stopped_by_rule`` = True; the members' common ``init`` value is
    the included candidate, and where they differ in ``init`` nothing is, so only a uniform start bounds the result by ``nll_init``).  Exits above
    ``target`` are not members of row ``target``: they keep their ``init`` value.  ``init``: [E] or a scalar, float32-representable
    values are kept as they are (others are rounded to float32 once).

    Returns dict(tau [E], nll_init [E], nll_after [E] (every row at ``init`` / at ``tau``), trace (row ``target`` after each sweep),
    sweeps, at_bound bool [E] (a searched coordinate ended on an end of the bracket), stopped_by_rule)."""
    E = int(n_exits)
    target = int(target) + (E if int(target) < 0 else 0)
    if not 0 <= target < E:
        raise ValueError(f"target must be an exit index of {E} exits, got {target}")
    if mode not in ("vector", "shared"):
        raise ValueError(f'mode must be "vector" or "shared", got {mode!r}')
    tau = np.asarray(init, dtype=np.float64).reshape(-1).astype(np.float32).astype(np.float64)
    tau = np.repeat(tau, E) if tau.size == 1 else tau.copy()
    if tau.size != E or not (np.all(np.isfinite(tau)) and np.all(tau > 0)):
        raise ValueError(f"init must hold one finite temperature > 0 per exit ({E}), got {tau.tolist()}")
    at_bound = np.zeros(E, dtype=bool)

    def rows(t):
        return np.asarray(eval_fn(t, None, t[:1]), dtype=np.float64).reshape(E, 1)[:, 0]

    def step(vary, current):
        z = zoom_search(lambda c: np.asarray(eval_fn(tau, vary, c[0]), dtype=np.float64)[target][None], 1, include=current, **zoom)
        return z["tau"][0], z["nll_after"][0], bool(z["at_bound"][0])

    nll_init = rows(tau)
    trace, sweeps, stopped = [], 0, False
    if mode == "shared":
        members = list(range(target + 1))
        same = bool(np.all(tau[members] == tau[0]))
        t, v, b = step(members, tau[0] if same else None)
        tau[members], at_bound[members] = t, b
        trace, sweeps, stopped = [float(v)], 1, True
    else:
        prev = float(nll_init[target])
        while sweeps < int(max_sweeps):
            for i in range(target + 1):
                tau[i], v, at_bound[i] = step(i, tau[i])
            sweeps += 1
            trace.append(float(v))
            if prev - v <= sweep_rtol * abs(prev):
                stopped = True
                break
            prev = float(v)
    return dict(tau=tau, nll_init=nll_init, nll_after=rows(tau), trace=np.array(trace), sweeps=sweeps, at_bound=at_bound, stopped_by_rule=stopped)


# apply(): what a fit sets on the model, kind -> (the model's setter, the entries of the result it takes, the attribute it fills)
_MODEL_SETTERS = {"temperature": ("set_exit_temperature", ("tau",), "exit_temperature"),
                  "vector": ("set_exit_vector_scaling", ("scale", "bias"), "exit_vector_scaling"),
                  "matrix": ("set_exit_matrix_scaling", ("matrix", "bias"), "exit_matrix_scaling"),
                  "weights": ("set_exit_ensemble_weights", ("weights",), "exit_ensemble_weights")}


class _Fit:
    """What the loader-level fits below share: ``result`` (None before ``fit()``), ``apply()`` and ``save()``.  A subclass names its
    ``_kind`` (a key of the table above), the kinds ``apply()`` clears first (``_clears``: one calibration map per model) and its file
    prefix (``_file``)."""
    result = None
    _kind = _file = None
    _clears = ()

    def _require_fit(self):
        if self.result is None:
            raise RuntimeError("fit() first")
        return self.result

    def _save(self, prefix, experiment_id):
        name = f"{prefix}_{experiment_id}.npz"
        np.savez(name, **{k: np.asarray(v) for k, v in self._require_fit().items()})
        return name

    def apply(self):
        """Sets the fitted values on the model — after clearing the maps they cannot stand beside (``VectorScaling`` and ``MatrixScaling``
        clear the other two; a temperature clears nothing) — and returns the model's attribute: ``exit_temperature``, ``exit_vector_scaling``,
        ``exit_matrix_scaling`` or ``exit_ensemble_weights``."""
        r = self._require_fit()
        for kind in self._clears:
            getattr(self.model, _MODEL_SETTERS[kind][0])(None)
        setter, keys, attr = _MODEL_SETTERS[self._kind]
        getattr(self.model, setter)(*(r[k] for k in keys))
        return getattr(self.model, attr)

    def save(self, experiment_id):
        """Writes ``<prefix>_<id>.npz`` — every entry of the result; the prefix is temperature, vector_scaling, matrix_scaling,
        ensemble_temperature or ensemble_weights — and returns its name."""
        return self._save(self._file, experiment_id)


class TemperatureScaling(_Fit):
    """Fits one temperature per exit on a labelled (validation) loader.

        ts = TemperatureScaling(model, val_loader, gpu=0, mc_passes=10)
        ts.fit()            # dict(tau, nll_before, nll_after, at_bound, rounds, n)
        ts.apply()          # model.set_exit_temperature(tau): every engine built from the model from now on runs under it

    ``fit`` walks the loader ONCE — batch k under the Philox seed ``seed + k`` and the Masksembles counter FullAnalysis' walk would use
    (the layers' current ``cnt``, advanced by ``mc_passes`` per batch; the model's own state is left where it was) — and keeps the RAW
    per-sample logits of the whole split on the device: N x T x E x C x 4 bytes (160 MB for the paper's 10 000 x 10 x 4 x 100).  Beyond
    ``max_logit_bytes`` it raises ValueError (recomputing the logits per search round is out of scope).  The search is ``zoom_search``
    with one ``MCDEngine.nll_grid`` launch per batch and round.  Raw logits do not depend on a temperature already set on the model, so a
    fit can be repeated."""

    def __init__(self, model, val_loader, gpu=0, mc_passes=10, seed=0, max_logit_bytes=1 << 30):
        self.model, self.loader, self.gpu = model, val_loader, gpu
        self.mc_passes, self.seed, self.max_logit_bytes = int(mc_passes), int(seed), int(max_logit_bytes)
        self.device = get_device(gpu)

    _kind, _file = "temperature", "temperature"

    def _n_images(self):
        loader = self.loader
        if getattr(loader, "sampler", None) is not None and hasattr(loader.sampler, "__len__"):
            return len(loader.sampler)
        if hasattr(loader, "dataset"):
            return len(loader.dataset)
        return sum(len(b[1]) for b in loader)

    def collect(self):
        """The walk: [(logits fp32 [T, E, B, C], labels int32 [B])] per loader batch, on the device."""
        from ..engine import model_exits
        model, T = self.model, self.mc_passes
        model.eval()
        E, C = model_exits(model), int(model.out_dim)
        need = self._n_images() * T * E * C * 4
        if need > self.max_logit_bytes:
            raise ValueError(f"the split's per-sample logits take {need} bytes (N x T x E x C x 4 = {self._n_images()} x {T} x {E} x {C} x 4), "
                             f"more than max_logit_bytes = {self.max_logit_bytes}")
        ml = model.mask_layers()
        cnt, held, batches = (ml[0].cnt if ml else 0), 0, []
        for k, (x, y) in enumerate(self.loader):
            y = torch.as_tensor(y).reshape(-1).to("cpu", torch.int64)
            if y.numel() != x.shape[0] or int(y.min()) < 0 or int(y.max()) >= C:
                raise ValueError(f"batch {k}: labels must be one per image and lie in [0, {C})")
            held += x.shape[0] * T * E * C * 4
            if held > self.max_logit_bytes:            # (a loader that yields more than it announced)
                raise ValueError(f"the split's per-sample logits exceed max_logit_bytes = {self.max_logit_bytes} ({held} bytes after batch {k})")
            x = x.to(self.device, non_blocking=True)
            eng = model.engine(self.device, max_batch=x.shape[0], calib=x)
            cnt0 = (cnt + k * T) % ml[0].n if ml else 0
            batches.append((eng.forward_samples(x, T, seed=self.seed + k, cnt0=cnt0), y.to(self.device, torch.int32)))
        if not batches:
            raise ValueError("the loader yielded no batch")
        self._engine = eng
        return batches

    def fit(self, **search):
        """Walk + search (keyword arguments go to ``zoom_search``).  Returns — and keeps in ``self.result`` — dict(tau, nll_before, nll_after,
        at_bound [E] each, rounds, n)."""
        from ..engine import model_exits
        batches = self.collect()
        r = zoom_search(lambda tau: self._eval_tau(batches, tau), model_exits(self.model), **search)
        r["n"] = int(sum(y.numel() for _, y in batches))
        self.result = r
        return r

    def _eval_tau(self, batches, tau):
        """nll [E, G] of the candidate temperatures ``tau`` [E, G] over ``batches``, on the device (``MCDEngine.nll_grid``)."""
        out = None
        grid = torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float32)).to(self.device)
        for logits, y in batches:
            out = self._engine.nll_grid(logits, y, grid, out=out)
        return out.cpu().numpy()

    def _eval_vector(self, batches, x, C):
        """Unpenalised (nll [E], grad [E, 2 C]) of the point x [E, 2 C] = (scale, bias) over ``batches``, on the device."""
        a = torch.from_numpy(np.ascontiguousarray(x[:, :C])).to(self.device)
        b = torch.from_numpy(np.ascontiguousarray(x[:, C:])).to(self.device)
        out = None
        for logits, y in batches:
            out = self._engine.nll_vector_grad(logits, y, a, b, out=out)
        return out[0].cpu().numpy(), np.concatenate([out[1].cpu().numpy(), out[2].cpu().numpy()], axis=1)

    def _eval_matrix(self, batches, x, C):
        """Unpenalised (nll [E], grad [E, C * C + C]) of the point x [E, C * C + C] = (matrix rows, bias) over ``batches``, on the device."""
        E = x.shape[0]
        M = torch.from_numpy(np.ascontiguousarray(x[:, :C * C]).reshape(E, C, C)).to(self.device)
        b = torch.from_numpy(np.ascontiguousarray(x[:, C * C:])).to(self.device)
        out = None
        for logits, y in batches:
            out = self._engine.nll_matrix_grad(logits, y, M, b, out=out)
        return out[0].cpu().numpy(), np.concatenate([out[1].cpu().numpy().reshape(E, C * C), out[2].cpu().numpy()], axis=1)

    @staticmethod
    def _round_and_keep(evaluate, penalty, x, x0):
        """The tail of the vector and the matrix fit: the optimiser's point ``x`` and its start ``x0`` [E, D] rounded to float32 once — what
        the head will run — and the objective (``evaluate(x)[0]``, plus ``penalty(x)`` [E] where one is given) evaluated once more at both;
        per exit the rounded start is kept where rounding lost ground against it (a fit that moved: never).  Returns (x float32 [E, D],
        the unpenalised nll [E], the penalty [E] — zeros without one)."""
        x32, x032 = (v.astype(np.float32).astype(np.float64) for v in (x, x0))
        nll, nll0 = evaluate(x32)[0], evaluate(x032)[0]
        pen, pen0 = (penalty(x32), penalty(x032)) if penalty else (np.zeros_like(nll), np.zeros_like(nll0))
        keep = nll + pen <= nll0 + pen0
        return np.where(keep[:, None], x32, x032).astype(np.float32), np.where(keep, nll, nll0), np.where(keep, pen, pen0)


class VectorScaling(TemperatureScaling):
    """Fits a per-class scale and bias per exit (vector scaling) on a labelled (validation) loader.

        vs = VectorScaling(model, val_loader, gpu=0, mc_passes=10)
        vs.fit()            # dict(scale, bias, nll_start, nll_after, grad_norm, iterations, converged, n)
        vs.apply()          # model.set_exit_temperature(None); model.set_exit_vector_scaling(scale, bias)

    The walk and the ``max_logit_bytes`` rule are ``TemperatureScaling``'s.  The search starts at the scalar fit of the same logits — a =
    1 / tau_e for every class, b = 0, tau from ``zoom_search`` — and runs ``lbfgs_minimize`` on the 2C parameters of every exit, all exits
    in the same ``MCDEngine.nll_vector_grad`` launches (one per batch and evaluation), in float64.  The result is rounded to float32 once
    and ``nll_after`` is evaluated once more at the ROUNDED parameters — what the head will run; should that rounding not keep the
    start's value (a fit that did not move), the rounded start is returned.  sum_c of the bias gradient is 0, so the bias stays in the
    zero-sum gauge it starts in.  Raw logits depend on neither a temperature nor a vector scaling set on the model: a fit can be repeated."""

    def fit(self, max_iter=50, gtol=1e-5, history=10, bias_l2=0.0, **search):
        """Walk + scalar search (keyword arguments ``search`` go to ``zoom_search``) + L-BFGS.  Returns — and keeps in ``self.result`` —
        dict(scale, bias float32 [E, C]; nll_start (the scalar fit's NLL), nll_after, grad_norm (|g|_inf at the optimiser's last point),
        iterations, converged [E] each; tau [E] (the scalar fit); n).  ``bias_l2`` > 0: the optimiser's objective gains ``odir_penalty``'s
        bias term, n bias_l2 / C sum_c b_c^2, added on the host; ``nll_after`` stays the unpenalised NLL, the result gains ``penalty``
        [E], and the rounded start is kept when rounding lost ground on the PENALISED objective.  0.0: the fit as it was, the penalty is
        never evaluated."""
        from ..engine import model_exits
        batches = self.collect()
        E, C = model_exits(self.model), int(self.model.out_dim)
        n = int(sum(y.numel() for _, y in batches))
        bias_l2 = float(bias_l2)
        if bias_l2 < 0 or not np.isfinite(bias_l2):
            raise ValueError("bias_l2 must be finite and >= 0")

        def eval_vec(x):
            return self._eval_vector(batches, x, C)

        def pen_of(x):                                           # (bias_l2 > 0 only)
            return odir_penalty(None, x[:, C:], n, 0.0, bias_l2)

        def eval_pen(x):
            f, g = eval_vec(x)
            pv, _, pg = pen_of(x)
            g[:, C:] += pg
            return f + pv, g

        z = zoom_search(lambda tau: self._eval_tau(batches, tau), E, **search)
        inv = 1.0 / np.asarray(z["tau"], dtype=np.float32).astype(np.float64)
        x0 = np.concatenate([np.repeat(inv[:, None], C, axis=1), np.zeros((E, C))], axis=1)
        r = lbfgs_minimize(eval_pen if bias_l2 else eval_vec, x0, max_iter=max_iter, gtol=gtol, history=history)
        x32, nll_after, pen = self._round_and_keep(eval_vec, (lambda x: pen_of(x)[0]) if bias_l2 else None, r["x"], x0)
        extra = dict(penalty=pen) if bias_l2 else {}
        self.result = dict(**extra, scale=np.ascontiguousarray(x32[:, :C]), bias=np.ascontiguousarray(x32[:, C:]), nll_start=z["nll_after"], nll_after=nll_after,
                           grad_norm=np.max(np.abs(r["g"]), axis=1), iterations=r["iterations"], converged=r["converged"],
                           tau=np.asarray(z["tau"]), n=n)
        return self.result

    _kind, _file, _clears = "vector", "vector_scaling", ("temperature", "matrix")


class MatrixScaling(VectorScaling):
    """Fits a full [C, C] matrix and a bias per exit (matrix scaling) on a labelled (validation) loader.

        ms = MatrixScaling(model, val_loader, gpu=0, mc_passes=10)
        ms.fit(off_diag_l2=1.0)       # dict(matrix, bias, nll_start, nll_after, penalty, grad_norm, iterations, converged, scale0, bias0, tau, n)
        ms.select(holdout_loader)     # ... or let a hold-out split choose off_diag_l2
        ms.apply()                    # clears temperature and vector scaling; model.set_exit_matrix_scaling(matrix, bias)

    AN UNREGULARISED MATRIX FIT ON A SMALL SPLIT OVERFITS.  It has C^2 + C parameters per exit (10 100 at C = 100) and will drive the
    training NLL towards 0 with off-diagonal entries of any size.  A CPU trial — C = 10, 48 images, T = 10, teacher labels from a banded
    confusion matrix, two exits: training NLL 97.1 / 38.2 under the vector fit; the unpenalised matrix fit took it to 39.0 / 0.32 with an
    off-diagonal rms of 47 and 11; off_diag_l2 = 1.0 gives 54.9 / 5.7 with rms 0.30; off_diag_l2 = 100 gives 86.3 / 30.9 with rms 0.03.
    Use ``off_diag_l2`` > 0 (``odir_penalty``: Kull et al. 2019) and choose it with ``select`` on data the fit has not seen.

    The walk and the ``max_logit_bytes`` rule are ``TemperatureScaling``'s.  ``fit`` runs the vector fit first, unregularised, exactly as
    ``VectorScaling.fit`` does, starts at M = diag(scale), b = bias and runs ``lbfgs_minimize`` on the C^2 + C parameters of every exit, all
    exits in the same ``MCDEngine.nll_matrix_grad`` launches (one per batch and evaluation), in float64; the penalty is added on the host.
    The result is rounded to float32 once, ``nll_after`` is the UNPENALISED NLL at the rounded parameters, and the rounded start is kept
    where rounding lost ground on the penalised objective.  With ``bias_l2 = 0`` the start has zero penalty and every accepted step lowers
    the penalised objective, so ``nll_after <= nll_start`` for every ``off_diag_l2 >= 0``."""

    _held = None          # (select) the collected batches, kept across the candidates' fits
    _held_vec = None      # (select) the vector fit of those batches

    def collect(self):
        return self._held if self._held is not None else super().collect()

    def fit(self, off_diag_l2=0.0, bias_l2=0.0, max_iter=50, gtol=1e-5, history=10, **search):
        """Walk + vector fit (``VectorScaling.fit(max_iter, gtol, history, **search)``, unregularised) + L-BFGS on the matrix.  Returns — and
        keeps in ``self.result`` — dict(matrix float32 [E, C, C], bias float32 [E, C]; nll_start (the vector fit's NLL), nll_after (unpenalised,
        at the returned parameters), penalty, grad_norm (|g|_inf of the penalised objective at the optimiser's last point), iterations,
        converged [E] each; scale0, bias0 (the vector fit), tau (the scalar fit); n)."""
        from ..engine import model_exits
        off_diag_l2, bias_l2 = float(off_diag_l2), float(bias_l2)
        if not (np.isfinite(off_diag_l2) and np.isfinite(bias_l2)) or off_diag_l2 < 0 or bias_l2 < 0:
            raise ValueError("off_diag_l2 and bias_l2 must be finite and >= 0")
        own = self._held is None
        if own:
            self._held = TemperatureScaling.collect(self)
        try:
            batches = self._held
            v = self._held_vec if self._held_vec is not None else VectorScaling.fit(self, max_iter=max_iter, gtol=gtol, history=history, **search)
            if not own:
                self._held_vec = v
            E, C, n = model_exits(self.model), int(self.model.out_dim), int(v["n"])
            penalised = off_diag_l2 != 0.0 or bias_l2 != 0.0

            def pen_of(x):
                return odir_penalty(x[:, :C * C].reshape(E, C, C), x[:, C * C:], n, off_diag_l2, bias_l2)

            def objective(x):
                f, g = self._eval_matrix(batches, x, C)
                if penalised:
                    pv, pm, pb = pen_of(x)
                    f, g = f + pv, g + np.concatenate([pm.reshape(E, C * C), pb], axis=1)
                return f, g

            a0, b0 = v["scale"].astype(np.float64), v["bias"].astype(np.float64)
            M0 = np.zeros((E, C, C))
            M0[:, np.arange(C), np.arange(C)] = a0
            x0 = np.concatenate([M0.reshape(E, C * C), b0], axis=1)          # (float32 values: the vector fit's rounded result)
            r = lbfgs_minimize(objective, x0, max_iter=max_iter, gtol=gtol, history=history)
            x32, nll_after, pen = self._round_and_keep(lambda x: self._eval_matrix(batches, x, C), lambda x: pen_of(x)[0], r["x"], x0)
            self.result = dict(matrix=np.ascontiguousarray(x32[:, :C * C].reshape(E, C, C)), bias=np.ascontiguousarray(x32[:, C * C:]),
                               nll_start=np.asarray(v["nll_after"]), nll_after=nll_after, penalty=pen,
                               grad_norm=np.max(np.abs(r["g"]), axis=1), iterations=r["iterations"], converged=r["converged"],
                               scale0=v["scale"], bias0=v["bias"], tau=np.asarray(v["tau"]), n=n)
        finally:
            if own:
                self._held = None
        return self.result

    def select(self, holdout_loader, off_diag_l2=(0.01, 0.1, 1.0, 10.0), bias_l2=0.0, **fit):
        """Chooses ``off_diag_l2`` on data the fit has not seen: one ``fit`` per candidate on the validation loader (walked once: the
        collected logits and the vector fit are reused), the UNPENALISED NLL of each result on ``holdout_loader`` (walked once, the same
        ``MCDEngine.nll_matrix_grad`` call), and the candidate with the lowest hold-out NLL summed over the exits is kept in ``self.result``
        (ties: the first).  Returns the table: one dict per candidate, in order — off_diag_l2, bias_l2, nll_after [E] (validation),
        nll_holdout [E], total_holdout, penalty [E], selected (bool)."""
        cands = [float(c) for c in np.atleast_1d(np.asarray(off_diag_l2, dtype=np.float64))]
        if not cands:
            raise ValueError("select: no candidate")
        C = int(self.model.out_dim)
        self._held = TemperatureScaling.collect(self)
        self._held_vec = None
        try:
            hold = TemperatureScaling(self.model, holdout_loader, self.gpu, self.mc_passes, self.seed, self.max_logit_bytes).collect()
            table, results = [], []
            for c in cands:
                r = self.fit(off_diag_l2=c, bias_l2=bias_l2, **fit)
                E = r["matrix"].shape[0]
                x = np.concatenate([r["matrix"].reshape(E, C * C), r["bias"]], axis=1).astype(np.float64)
                nll_h = self._eval_matrix(hold, x, C)[0]
                results.append(r)
                table.append(dict(off_diag_l2=c, bias_l2=float(bias_l2), nll_after=r["nll_after"], nll_holdout=nll_h,
                                  total_holdout=float(np.sum(nll_h)), penalty=r["penalty"], selected=False))
        finally:
            self._held = self._held_vec = None
        best = int(np.argmin([row["total_holdout"] for row in table]))       # (argmin: the first of equals)
        table[best]["selected"] = True
        self.result = results[best]
        self.selected = best
        return table

    _kind, _file, _clears = "matrix", "matrix_scaling", ("temperature", "vector")


class EnsembleTemperatureScaling(TemperatureScaling):
    """Fits the exits' temperatures JOINTLY, to the NLL of the exit ensemble they end up in (row ``target``: the mean of exits 0..target).

        ets = EnsembleTemperatureScaling(model, val_loader, gpu=0, mc_passes=10)
        ets.fit()           # dict(tau, nll_init, nll_after, trace, sweeps, at_bound, stopped_by_rule, tau_init, nll_ones, nll_per_exit, n)
        ets.apply()         # model.set_exit_temperature(tau): predict_ensemble and the adaptive / staged read-outs follow

    The walk (``collect``), its seeds, the Masksembles counter and the ``max_logit_bytes`` budget are ``TemperatureScaling``'s; the search
    is ``coordinate_search`` with one ``MCDEngine.ensemble_nll_grid`` launch per batch and round."""

    def fit(self, target=-1, mode="vector", init="per_exit", **search):
        """Walk + search (keyword arguments go to ``coordinate_search`` and on to ``zoom_search``).  ``init``: "per_exit" (the parent's fit
        of every exit to its own NLL, on the same logits), "ones", or an array [E].  Returns — and keeps in ``self.result`` —
        ``coordinate_search``'s dict plus ``tau_init`` (the start of the search), ``nll_ones`` [E] (the ensemble rows at tau = 1), ``nll_per_exit`` [E] (the ensemble rows at the
        per-exit fit, where that fit was run) and ``n``."""
        from ..engine import model_exits
        batches = self.collect()
        eng, E = self._engine, model_exits(self.model)

        def eval_fn(tau, vary, cand):
            out = None
            cand = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.float32)).to(self.device)
            for logits, y in batches:
                out = eng.ensemble_nll_grid(logits, y, tau, vary, cand, out=out)
            return out.cpu().numpy()

        extra = {}
        if isinstance(init, str):
            if init == "per_exit":
                init = zoom_search(lambda tau: self._eval_tau(batches, tau), E)["tau"]
                extra["nll_per_exit"] = eval_fn(init, None, np.ones(1))[:, 0]
            elif init == "ones":
                init = np.ones(E)
            else:
                raise ValueError(f'init must be "per_exit", "ones" or an array, got {init!r}')
        r = coordinate_search(eval_fn, E, target, init, mode=mode, **search)
        r["tau_init"] = np.asarray(init, dtype=np.float64).reshape(-1)
        r["nll_ones"] = eval_fn(np.ones(E), None, np.ones(1))[:, 0]
        r.update(extra)
        r["n"] = int(sum(y.numel() for _, y in batches))
        self.result = r
        return r

    _file = "ensemble_temperature"


# ---- the weights of the exit ensembles -----------------------------------------------------------------------------------------------
_MIX_FLOOR = 1e-300      # a sample whose label has probability 0 under every member: its mixture is floored here, the NLL stays finite


def _mixture(A, w):
    """max(sum_i w_i A_i, 1e-300) [N], the members added in order (no BLAS: the same bits for the same table wherever it lies in memory)."""
    mix = np.zeros(A.shape[1], dtype=np.float64)
    for i in range(A.shape[0]):
        mix = mix + w[i] * A[i]
    return np.maximum(mix, _MIX_FLOOR)


def mixture_nll(A, w):
    """sum_n -log(max(w @ A, 1e-300)) for a table ``A`` [k, N] of member likelihoods and weights ``w`` [k], float64."""
    return float(-np.log(_mixture(np.asarray(A, dtype=np.float64), np.asarray(w, dtype=np.float64))).sum())


def mixture_weights_em(A, rtol=1e-12, max_iter=100000):
    """The maximum-likelihood weights of a mixture with FIXED members: ``A`` [k, N], A[i][n] >= 0 the likelihood of sample n under member
    i.  Starts uniform and iterates  w <- w * mean_n(A / (w @ A))  (the EM step; the NLL is convex in w, every step lowers it and keeps
    sum(w) = 1 — renormalised by the exactly rounded sum against drift) until a step gains <= rtol * |NLL|; a step that would RAISE the
    NLL (rounding, at the optimum) is not taken.  Returns dict(w [k], nll, nll_uniform, trace — the NLL after every accepted step, first
    entry the uniform start: non-increasing —, iterations, converged).  One member returns w = [1.]."""
    import math
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("A must be [k, N] with k >= 1 members and N >= 1 samples")
    if not np.all(np.isfinite(A)) or np.any(A < 0):
        raise ValueError("A: every likelihood must be finite and >= 0")
    k = A.shape[0]
    w = np.full(k, 1.0 / k)
    mix = _mixture(A, w)
    nll = float(-np.log(mix).sum())
    trace, converged, it = [nll], False, 0
    for it in range(1, int(max_iter) + 1):
        w_new = w * (A / mix).mean(axis=1)
        w_new = w_new / math.fsum(w_new)
        mix_new = _mixture(A, w_new)
        nll_new = float(-np.log(mix_new).sum())
        gain = nll - nll_new
        if gain >= 0:
            w, mix, nll = w_new, mix_new, nll_new
            trace.append(nll)
        if gain <= rtol * abs(nll):
            converged = True
            break
    return dict(w=w, nll=nll, nll_uniform=trace[0], trace=np.array(trace), iterations=it, converged=converged)


class EnsembleWeights(_Fit):
    """Fits the weights of the exit ensembles on a labelled (validation) loader, by maximum likelihood per row.

        ew = EnsembleWeights(model, val_loader, gpu=0, mc_passes=10)
        ew.fit()            # dict(weights [E, E], nll_uniform, nll_after, nll_per_exit [E] each, iterations, converged, n)
        ew.apply()          # model.set_exit_ensemble_weights(W): predict_ensemble, the adaptive / staged read-outs and decisions follow

    The walk is ``TemperatureScaling``'s — batch k under the Philox seed ``seed + k`` and the Masksembles counter FullAnalysis' walk would
    use, the model's own state left where it was — but it keeps only A[e][n] = mean[e, n, y_n], the label's entry of ``predict``'s T-mean
    softmax, gathered on the device: E x N float64, no per-sample logits and no ``max_logit_bytes``.  The members are as tempered by the
    temperature currently set on the model: fit and ``apply()`` the temperatures FIRST, then the weights at those temperatures.  Row e
    of the result is ``mixture_weights_em`` on rows 0..e of the table (row 0 is [1.])."""

    def __init__(self, model, val_loader, gpu=0, mc_passes=10, seed=0):
        self.model, self.loader, self.gpu = model, val_loader, gpu
        self.mc_passes, self.seed = int(mc_passes), int(seed)
        self.device = get_device(gpu)

    _kind, _file = "weights", "ensemble_weights"

    def _engine_for(self, x):
        return self.model.engine(self.device, max_batch=x.shape[0], calib=x)

    def collect(self):
        """The walk: the table A [E, N] float64 (host) of the label's T-mean probability per exit and image."""
        model, T = self.model, self.mc_passes
        model.eval()
        C = int(model.out_dim)
        ml = model.mask_layers()
        cnt, cols = (ml[0].cnt if ml else 0), []
        for k, (x, y) in enumerate(self.loader):
            y = torch.as_tensor(y).reshape(-1).to("cpu", torch.int64)
            if y.numel() != x.shape[0] or int(y.min()) < 0 or int(y.max()) >= C:
                raise ValueError(f"batch {k}: labels must be one per image and lie in [0, {C})")
            x = x.to(self.device, non_blocking=True)
            eng = self._engine_for(x)
            cnt0 = (cnt + k * T) % ml[0].n if ml else 0
            mean = eng.predict(x, T, seed=self.seed + k, cnt0=cnt0)["mean"]              # [E, B, C] float64
            idx = y.to(mean.device).view(1, -1, 1).expand(mean.shape[0], -1, 1)
            cols.append(mean.gather(2, idx).squeeze(2).cpu().numpy())
            eng.check_finite()
        if not cols:
            raise ValueError("the loader yielded no batch")
        return np.concatenate(cols, axis=1)

    def fit(self, **em):
        """Walk + EM per row (keyword arguments go to ``mixture_weights_em``).  Returns — and keeps in ``self.result`` — dict(weights [E, E],
        nll_uniform / nll_after [E]: the ensemble rows' NLL at equal weights and at the fit, nll_per_exit [E]: every exit alone,
        iterations, converged [E], n)."""
        A = self.table = self.collect()
        E = A.shape[0]
        W = np.zeros((E, E), dtype=np.float64)
        rows = [mixture_weights_em(A[:e + 1], **em) for e in range(E)]
        for e, r in enumerate(rows):
            W[e, :e + 1] = r["w"]
        self.result = dict(weights=W, nll_uniform=np.array([r["nll_uniform"] for r in rows]), nll_after=np.array([r["nll"] for r in rows]),
                           nll_per_exit=np.array([mixture_nll(A[e:e + 1], [1.0]) for e in range(E)]),
                           iterations=np.array([r["iterations"] for r in rows]), converged=np.array([r["converged"] for r in rows]),
                           n=int(A.shape[1]))
        return self.result
