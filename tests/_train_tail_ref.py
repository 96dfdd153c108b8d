"""Restatement of the loss-head and Adam rules of include/sgx.h ("the loss head", "the optimiser") in numpy float64, the
dropout mask in exact integer arithmetic, and the error bounds of the fp32 kernels derived from their operation counts.

u = 2^-24 is fp32's unit roundoff; gamma(n) = n u / (1 - n u) bounds n successive roundings (Higham, Accuracy and
Stability, lemma 3.1).  expf / logf are taken at OpenCL's conformance limit of 3 ulp = 6 u (the device library is
tighter).  Nothing here is tuned to what the kernels return."""
import numpy as np

from _sampler_ref import mix64

U = 2.0 ** -24
K_EXP = K_LOG = 6.0          # in units of u: 3 ulp
HEAD_GRID = 256              # slices of sgx_head_loss (include/sgx.h)
M64 = (1 << 64) - 1


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the dropout mask --------------------------------------------------------------------------------------------------
def _mix64_np(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keep_mask(G, P, p, seed, step):
    """keep[g][j] of the rule: exact integers.  p is taken as the float32 the call receives."""
    key = mix64(mix64(seed & M64) ^ (step & M64))
    thr = int(np.floor(float(np.float32(p)) * 2.0 ** 24))
    idx = np.arange(G * P, dtype=np.uint64)
    k = _mix64_np(np.uint64(key) ^ idx)
    return ((k >> np.uint64(40)) >= np.uint64(thr)).reshape(G, P)


def keep_mask_scalar(G, P, p, seed, step):
    """The same on Python integers through _sampler_ref.mix64 only (slow; the CPU test holds the two together)."""
    key = mix64(mix64(seed) ^ (step & M64))
    thr = int(np.floor(float(np.float32(p)) * 2.0 ** 24))
    return np.array([[(mix64(key ^ (g * P + j)) >> 40) >= thr for j in range(P)] for g in range(G)])


def dropped(pooled, p, seed, step):
    """x of the rule, in float32 exactly as the kernel forms it (two fp32 operations for the scale, one product), the
    mask and the scale."""
    pooled = np.asarray(pooled, np.float32)
    keep = keep_mask(pooled.shape[0], pooled.shape[1], p, seed, step)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    x = np.where(keep, pooled * scale, np.float32(0.0)).astype(np.float32)
    return x, keep, scale


# ---- the loss head in float64 ------------------------------------------------------------------------------------------
def head_f64(pooled, W, bias, target, p=0.0, seed=0, step=0, grad_scale=1.0):
    """loss, logits, grad_pooled, grad_W, grad_bias (None without a bias) in float64 from the fp32 inputs, plus what the
    bounds need."""
    x32, keep, scale = dropped(pooled, p, seed, step)
    x, W = x32.astype(np.float64), np.asarray(W, np.float64)
    G, P = x.shape
    C = W.shape[0]
    b = np.zeros(C) if bias is None else np.asarray(bias, np.float64)
    t = np.asarray(target, np.int64)
    live = (t >= 0) & (t < C)
    z = x @ W.T + b
    m = z.max(1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
    onehot = np.zeros((G, C))
    onehot[np.nonzero(live)[0], t[live]] = 1.0
    loss_g = np.where(live, lse - (z * onehot).sum(1), 0.0)
    prob = np.exp(z - lse[:, None])
    gs = float(np.float32(grad_scale)) / G
    dz = np.where(live[:, None], (prob - onehot) * gs, 0.0)
    grad_pooled = np.where(keep, float(scale) * (dz @ W), 0.0)
    grad_W = dz.T @ x
    grad_b = None if bias is None else dz.sum(0)
    aux = dict(x=x, keep=keep, scale=float(scale), z=z, lse=lse, prob=prob, onehot=onehot, live=live, dz=dz, gs=gs, loss_g=loss_g,
               W=W, b=b)
    return loss_g.sum() / G, z, grad_pooled, grad_W, grad_b, aux


def head_bounds(aux):
    """Absolute error bounds of sgx_head_loss against head_f64, per output, from the operation counts:
      logits   a dot product of P products and the bias, any order: gamma(P + 1) (|W| |x| + |b|)
      lse      1-Lipschitz in the logits' error (max norm); evaluated: z - m (u each, weighted by exp <= 1), expf (K_EXP u),
               C additions, logf (K_LOG u |log s|, log s <= log C), m + log s (u |lse|)
      loss_g   lse - z_t: both errors and one rounding; loss: G additions over the slices and the division
      dz       the argument z_c - lse carries both errors and one rounding; expf of it; the subtraction; gs carries two
               roundings (grad_scale / G, the product)
      grad_pooled  C products and additions and the scale: gamma(C + 1), plus |W|^T E_dz, times scale
      grad_W / grad_bias  every term passes at most ceil(G / S) + S additions and one product: gamma(that + 1)"""
    x, z, lse, prob, onehot, dz, gs, W, b = (aux[k] for k in ("x", "z", "lse", "prob", "onehot", "dz", "gs", "W", "b"))
    G, P = x.shape
    C = W.shape[0]
    e_z = gamma(P + 1) * (np.abs(x) @ np.abs(W).T + np.abs(b))
    # t_c = z_c - m <= 0 rounds by u |t_c|, which exp turns into a relative u |t_c| of a term of weight e^t_c / s:
    # |t| e^t <= 1 / e, s >= 1, so all C of them give at most u C / e; then expf, the C additions, logf, the last sum
    e_lse = e_z.max(1) + (U * C / np.e + K_EXP * U + gamma(C)) * (1 + gamma(C)) + K_LOG * U * np.log(C) + U * np.abs(lse)
    e_loss_g = np.where(aux["live"], e_lse + (e_z * onehot).sum(1) + U * np.abs(aux["loss_g"]), 0.0)
    S = min(G, HEAD_GRID)
    n_sum = -(-G // S) + S
    loss_abs = np.abs(aux["loss_g"]).sum() / G
    e_loss = e_loss_g.sum() / G + gamma(n_sum + 1) * loss_abs
    d_arg = e_z + e_lse[:, None] + U * np.abs(z - lse[:, None])
    e_prob = prob * (np.expm1(d_arg) + K_EXP * U * np.exp(d_arg))
    e_dz = np.where(aux["live"][:, None], gs * (e_prob + U * np.abs(prob - onehot)) * (1 + 3 * U) + 3 * U * np.abs(dz), 0.0)
    scale = aux["scale"]
    e_gp = np.where(aux["keep"], scale * (e_dz @ np.abs(W) + gamma(C + 1) * (np.abs(dz) @ np.abs(W))) * (1 + U), 0.0)
    e_gw = e_dz.T @ np.abs(x) + gamma(n_sum + 1) * (np.abs(dz).T @ np.abs(x))
    e_gb = e_dz.sum(0) + gamma(n_sum + 1) * np.abs(dz).sum(0)
    tiny = np.finfo(np.float32).tiny                      # below fp32's normal range a result is off by an absolute 2^-149
    return dict(logits=e_z + tiny, loss=e_loss + tiny, grad_pooled=e_gp + tiny, grad_W=e_gw + tiny, grad_bias=e_gb + tiny)


# ---- Adam in float64 ---------------------------------------------------------------------------------------------------
def adam_constants(lr, beta1, beta2, eps, weight_decay, t):
    """The constants as the rule rounds them (float32 values, held as float64)."""
    f = lambda v: float(np.float32(v))
    return dict(lr=f(lr), b1=f(beta1), ob1=f(1.0 - beta1), b2=f(beta2), ob2=f(1.0 - beta2), eps=f(eps), wd=f(weight_decay),
                bc1=f(1.0 - beta1 ** t), sbc2=f(np.sqrt(1.0 - beta2 ** t)))


def adam_f64(param, grad, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, rounded_constants=True):
    """One step of the rule in float64 (t = the step's number, from 1).  rounded_constants=False: the constants as the
    doubles torch.optim.Adam uses (the comparison against torch on float64 tensors)."""
    if rounded_constants:
        c = adam_constants(lr, beta1, beta2, eps, weight_decay, t)
    else:
        c = dict(lr=lr, b1=beta1, ob1=1.0 - beta1, b2=beta2, ob2=1.0 - beta2, eps=eps, wd=weight_decay, bc1=1.0 - beta1 ** t,
                 sbc2=np.sqrt(1.0 - beta2 ** t))
    p, g, m, v = (np.asarray(a, np.float64) for a in (param, grad, m, v))
    if c["wd"] != 0:
        g = g + c["wd"] * p
    m = c["b1"] * m + c["ob1"] * g
    v = c["b2"] * v + c["ob2"] * (g * g)
    denom = np.sqrt(v) / c["sbc2"] + c["eps"]
    p = p - (c["lr"] / c["bc1"]) * (m / denom)
    return p, m, v


def adam_bound_step(param, grad, m, v, t, e_p=0.0, e_m=0.0, e_v=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """Bounds (e_param, e_m, e_v) on the fp32 kernel's state after step t against adam_f64's, given the float64 state
    BEFORE the step (param, m, v) and bounds e_* on the kernel's state before it (0 at the start: both begin on the same
    fp32 values).  The constants are the same rounded values on both sides, so only the per-element operations err:
      g   = grad + wd * param        2 roundings on the product's term, one on the sum; the incoming e_p times wd
      m   = b1 m + ob1 g             each term one product, then the sum: 2 u on each; incoming errors times b1 / ob1
      v   = b2 v + ob2 g g           b2 v: 2 u; ob2 g g: 3 u; g's error enters as 2 |g| e_g + e_g^2
      s   = sqrt(v): |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b), and one rounding; / sqrt_bc2: one more
      d   = s + eps: one rounding;  q = m / d: (e_m + |q| e_d) / (d - e_d), one rounding
      p   = p - step_size q: step_size one rounding (the division), the product one, the difference one"""
    c = adam_constants(lr, beta1, beta2, eps, weight_decay, t)
    p, g0, m, v = (np.asarray(a, np.float64) for a in (param, grad, m, v))
    g = g0 + c["wd"] * p if c["wd"] != 0 else g0
    e_g = (c["wd"] * e_p + 2 * U * np.abs(c["wd"] * p) + U * np.abs(g)) if c["wd"] != 0 else np.zeros_like(g)
    m1 = c["b1"] * m + c["ob1"] * g
    e_m1 = (c["b1"] * e_m + c["ob1"] * e_g) * (1 + 2 * U) + 2 * U * (np.abs(c["b1"] * m) + np.abs(c["ob1"] * g))
    v1 = c["b2"] * v + c["ob2"] * g * g
    e_gg = 2 * np.abs(g) * e_g + e_g * e_g
    e_v1 = (c["b2"] * e_v + c["ob2"] * e_gg) * (1 + 3 * U) + 2 * U * c["b2"] * np.abs(v) + 3 * U * c["ob2"] * g * g
    s = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(v1 > 0, e_v1 / np.where(v1 > 0, s, 1.0), np.sqrt(e_v1)) + U * s
    sd = s / c["sbc2"]
    e_sd = e_s / c["sbc2"] * (1 + U) + U * sd
    d = sd + c["eps"]
    e_d = e_sd + U * (d + e_sd)
    q = m1 / d
    d_low = d - e_d
    assert (d_low > 0).all(), "the bound needs a denominator that stays positive"
    e_q = (e_m1 + np.abs(q) * e_d) / d_low
    e_q = e_q + U * (np.abs(q) + e_q)
    ss = c["lr"] / c["bc1"]
    e_u = ss * (1 + U) * e_q + 2 * U * ss * np.abs(q) * (1 + U)
    p1 = p - ss * q
    e_p1 = e_p + e_u + U * (np.abs(p1) + e_p + e_u)
    tiny = np.finfo(np.float32).tiny
    return e_p1 + tiny, e_m1 + tiny, e_v1 + tiny
