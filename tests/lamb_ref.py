"""Host reference of the fused LAMB step (csrc/lamb.hip; the definition in include/zsg.h, "Fused LAMB"), written from that definition
with numpy alone.  Every fp32 operation is one numpy operation, so it rounds on its own as the kernels' do (they are compiled without
contraction); the two norms are fp64 sums rounded to fp32.  For one parameter tensor w with gradient g, moments m, v, at its step t:

    m <- b1 m + (1 - b1) g                v <- b2 v + (1 - b2) g g
    u  = (m / bc1) / (sqrt(v / bc2) + eps) + wd w          bc = 1 - beta^t, formed in fp64, rounded once to fp32
    Nw = sqrt(sum w^2)   Nu = sqrt(sum u^2)
    r  = Nw / Nu if adapt and Nw > 0 and Nu > 0 else 1     (adapt and a NaN norm: r = NaN)
    w <- w - (lr r) u
"""
import numpy as np

F = np.float32


def bias_correction(beta, t):
    """1 - beta^t with beta as the fp32 value the kernel receives: formed in fp64, rounded once to fp32"""
    return F(1.0 - float(F(beta)) ** int(t))


def trust_ratio(nw, nu, adapt=True):
    nw, nu = F(nw), F(nu)
    if not adapt:
        return F(1.0)
    if np.isnan(nw) or np.isnan(nu):
        return F(np.nan)
    if nw > 0 and nu > 0:
        return F(nw / nu)
    return F(1.0)


def lamb_step(w, g, m, v, t, lr, beta1, beta2, eps, wd, adapt=True, grad_scale=1.0):
    """One step of one tensor (any shape; numpy arrays or anything np.asarray takes).  t = the tensor's own step count + 1.
    Returns (w, m, v, info) as new fp32 arrays; info = dict(ratio, norm_w, norm_u, u)."""
    w, g, m, v = (np.asarray(x, dtype=F) for x in (w, g, m, v))
    b1, b2, one = F(beta1), F(beta2), F(1.0)
    with np.errstate(all="ignore"):
        g = g * F(grad_scale)
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * (g * g)
        u = (m / bias_correction(beta1, t)) / (np.sqrt(v / bias_correction(beta2, t)) + F(eps)) + F(wd) * w
        nw = F(np.sqrt(np.sum(w.astype(np.float64) ** 2)))
        nu = F(np.sqrt(np.sum(u.astype(np.float64) ** 2)))
        r = trust_ratio(nw, nu, adapt)
        w = w - (F(lr) * r) * u
    return w, m, v, dict(ratio=r, norm_w=nw, norm_u=nu, u=u)
