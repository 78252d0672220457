"""Float64 models of gmz_opt_step and gmz_grad_add_t(_cols) (csrc/gmz_train.hip; include/gmz.h), in plain numpy.
Nothing here imports the package under test; tests/test_opt_ref.py pins them to torch.optim.Adam,
torch.nn.utils.clip_grad_norm_, the GradScaler's skip rule and the soft target update, all in float64.

The optimiser step over a flat bucket (p, t, g, m, v: float64 arrays of the bucket's length holding the f32 values
as stored; has_t: which elements have a target twin).  The C float arguments enter as their float32 values (f32()).
  scale     the GradScaler's scale; None = 1.  The bucket holds the SCALED gradient
  norm      sqrt(sum g^2) / scale: the norm of the unscaled gradient
  clip      min(max_norm / (norm + 1e-6), 1)            (torch.nn.utils.clip_grad_norm_)
  skip      skip_on_inf and some g is not finite
  coef      {1 if skip else 0, clip / scale}; on a skipped step coef[1] is written but carries no meaning
  step      += 1 unless skipped
  unless skipped, per element, with the advanced step s:
            g' = g coef[1] + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
            bc1 = 1 - b1^s, bc2 = 1 - b2^s;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)      (torch.optim.Adam)
  always    t = (1 - tau) t + tau p with the p just updated (or left, when skipped), where there is a twin; g = 0
"""
import numpy as np


def f32(v):
    return float(np.float32(v))


def opt_step(p, t, has_t, g, m, v, step, scale, skip_on_inf, max_norm, lr, beta1, beta2, eps, wd, tau):
    max_norm, lr, beta1, beta2, eps, wd, tau = (f32(a) for a in (max_norm, lr, beta1, beta2, eps, wd, tau))
    sc = 1.0 if scale is None else float(scale)
    finite = bool(np.isfinite(g).all())
    skip = bool(skip_on_inf) and not finite
    with np.errstate(all="ignore"):
        sumsq = float(np.sum(g * g))
        norm = np.sqrt(sumsq) / sc
        clip = min(max_norm / (norm + 1e-6), 1.0) if finite else float("nan")
    out = dict(finite=finite, skip=skip, sumsq=sumsq, norm=norm, clip=clip, coef=(1.0 if skip else 0.0, clip / sc),
               step=step if skip else step + 1.0, g=np.zeros_like(g))
    p2, m2, v2 = p.copy(), m.copy(), v.copy()
    if not skip:
        s = out["step"]
        with np.errstate(all="ignore"):
            gs = g * out["coef"][1]
            g2 = gs + wd * p
            m2 = beta1 * m + (1 - beta1) * g2
            v2 = beta2 * v + (1 - beta2) * g2 * g2
            bc1, bc2 = 1 - beta1 ** s, 1 - beta2 ** s
            denom = np.sqrt(v2) / np.sqrt(bc2) + eps
            upd = (lr / bc1) * m2 / denom
            p2 = p - upd
        out.update(gs=gs, g2=g2, bc1=bc1, bc2=bc2, denom=denom, upd=upd)
    t2 = np.where(has_t, (1 - tau) * t + tau * p2, t)
    out.update(p=p2, m=m2, v=v2, t=t2)
    return out


def grad_add_t_cols(dst, src, P, C, O, ldo, col0):
    """dst [O][C][P] (float64, what the destination held) + src[(p C + c) ldo + col0 + o]: one add per element."""
    s = np.asarray(src, np.float64).reshape(P, C, ldo)[:, :, col0:col0 + O]
    return np.asarray(dst, np.float64).reshape(O, C, P) + s.transpose(2, 1, 0)
