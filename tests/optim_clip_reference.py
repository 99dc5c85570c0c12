"""fp64 reference of gradient clipping and learning-rate decay in the device optimizer (include/clvae.h:
clv_grad_norm_scale, clv_adam_wn_step_clipped), on top of tests/optim_reference.py, which is imported and left as it is.

  norm   = sqrt(sum g^2) over the elements of the table's tensors (never the padding between them)
  scale  = clipnorm / norm where norm >= clipnorm, else 1                      (Keras: K.switch(n >= c, g * c / n, g))
  g_eff  = clampv(fl32(g * scale)), clampv the clamp to [-clipvalue, clipvalue] for clipvalue > 0, the identity at 0
  gdot_eff = fl32(gdot * scale)                                                (the known-sums form's sum g.V)
  lr     = fl32(lr0 / (1 + decay * it)) evaluated in fp64, it = t - 1          (Keras: lr *= 1 / (1 + decay * iterations))

Bounds.  The norm's, built the way optim_reference.true_sums builds b_A: the gradients are given (no operand variance); the
n terms g^2 are rounded once each, U^2 sum g^4; fp32 accumulation of n terms in any order, (U S)^2 (n / 3 + 1) with S the
sum; the square root, var_S / (4 S) + (U norm)^2; times KAPPA.  (A device that sums its partials in fp64 lies well inside:
the bound does not assume it.)  The scale's follows with one more division: (c / norm^2)^2 var_norm + (U scale)^2; where
nothing is clipped the scale is an exact 1 and its bound 0.  A clipnorm within the norm's bound of the norm would make
the branch itself uncertain: norm_ref refuses it (the tests use 0.25 and 4 times the norm, and inf).  Nothing here is fitted
to a GPU run.

g_eff and gdot_eff are evaluated in numpy float32 FROM A GIVEN fp32 scale (the device's own, already held to its bound):
one exactly rounded product and one clamp are the contract bit for bit, so the clipped step's outputs are held to
optim_reference.ref_step on g_eff with ref_step's own bounds and nothing added.  The decayed rate is likewise one
correctly rounded fp64 division rounded to fp32 once: the value a conforming device holds bit for bit.
"""
import numpy as np

import optim_reference as R
from vae_reference import U, KAPPA

F = np.float32


def owned(table, n):
    """mask over the flat buffer: the elements of the table's tensors"""
    own = np.zeros(n, bool)
    for d in table:
        own[d.offset:d.offset + d.rows * d.cols] = True
    return own


def norm64(grads, table):
    g = np.asarray(grads, np.float64)
    return float(np.sqrt(sum(float(np.square(g[d.offset:d.offset + d.rows * d.cols]).sum()) for d in table)))


def norm_ref(grads, table, clipnorm):
    """dict(norm, s_norm, b_norm, scale, s_scale, b_scale) for the fp32 clipnorm the device is handed (inf allowed)"""
    g = np.asarray(grads, np.float64)
    x = np.concatenate([np.square(g[d.offset:d.offset + d.rows * d.cols]) for d in table])
    norm = norm64(grads, table)
    n, S = x.size, norm * norm
    vS = U * U * float(np.square(x).sum()) + (U * S) ** 2 * (n / 3.0 + 1)
    v_norm = (vS / (4 * S) + (U * norm) ** 2) if S > 0 else 0.0
    out = dict(norm=norm, s_norm=float(np.sqrt(v_norm)), b_norm=KAPPA * float(np.sqrt(v_norm)))
    c = float(F(clipnorm))
    if not c > 0:
        raise ValueError("clipnorm must be > 0")
    if np.isfinite(c) and abs(norm - c) <= out['b_norm']:
        raise ValueError("clipnorm within the norm's bound of the norm: the branch is not determined")
    if np.isfinite(c) and norm >= c:
        scale = c / norm
        v_scale = (c / (norm * norm)) ** 2 * v_norm + (U * scale) ** 2
    else:
        scale, v_scale = 1.0, 0.0
    out.update(scale=scale, s_scale=float(np.sqrt(v_scale)), b_scale=KAPPA * float(np.sqrt(v_scale)))
    return out


def g_eff(grads, table, scale32, clipvalue=0.0):
    """the gradient every kernel reads in the place of g, in fp32 as the contract states it; what the table does not own
    (the padding) is returned as it is"""
    g = np.asarray(grads, F).copy()
    own = owned(table, g.size)
    x = g[own] * F(scale32)
    assert x.dtype == F
    if clipvalue > 0:
        cv = F(clipvalue)
        x = np.where(x < -cv, -cv, np.where(x > cv, cv, x)).astype(F)          # (a NaN stays a NaN)
    g[own] = x
    return g


def gdot_eff(gdot, scale32):
    out = np.asarray(gdot, F) * F(scale32)
    assert out.dtype == F
    return out


def median_abs(grads, table):
    """the clipvalue of the tests: the median |g| over the table's elements (about half of them are clamped).  Where more than
    half of them are zero (pair_first_145x2: column 1 of its 145 x 2 matrix and the zero rows) that median is 0, which means
    "off": there, the median of the non-zero ones"""
    g = np.asarray(grads, np.float64)
    a = np.abs(g[owned(table, g.size)])
    med = np.median(a)
    return float(F(med if med > 0 else np.median(a[a > 0])))


def decayed_lr(lr, decay, t):
    """fl32(lr / (1 + decay * it)), it = t - 1, with lr and decay the fp32 values the device is handed; fp64 inside"""
    return float(F(float(F(lr)) / (1.0 + float(F(decay)) * float(t - 1))))


def decayed_hyper(hyp, decay, t):
    return dict(hyp, lr=decayed_lr(hyp['lr'], decay, t)) if decay > 0 else dict(hyp)


def differing_share(clipped, other, mask):
    """share of the masked elements of params' at which `other` lies beyond the clipped reference's bounds: where a device
    that left the clip out (and returned `other`) would be reported by optim_reference.violations against `clipped`"""
    far = np.abs(clipped['params'] - other['params']) > clipped['b_params']
    return float(far[mask].sum()) / max(int(mask.sum()), 1)


# ------------------------------------------------------------------------------------------------------------ cases --
BY_NAME = {c['name']: c for c in R.GPU_CASES}
CASE_ROUTES = [(c, r) for c in R.GPU_CASES for r in c['routes']]
IDS = ["%s-%s" % (c['name'], r) for c, r in CASE_ROUTES]
VARIANTS = ('clipnorm', 'clipvalue', 'both')
CLIP_FACTOR = 0.25          # clipnorm = CLIP_FACTOR * norm64: every gradient is scaled by about a quarter
_STATES = {}


def known_for(table, st, grads, use):
    """the known-sums argument for the table's first tall matrix (None without one); use: gdot = sum_r g W in fp64 from the
    stored state, rounded to fp32 -- of the UNCLIPPED gradient, as the backward pass forms it"""
    tall = [i for i, d in enumerate(table) if R.is_tall(d)]
    if not tall:
        return None
    k = dict(tensor=tall[0], use=bool(use), gdot=None)
    if use:
        k['gdot'] = R.true_sums(st['params'], st['s'], grads, table[tall[0]])['gdot'].astype(F)
    return k


def prepared(case, route, gseed=900):
    """(table, n, n_cols, state, grads): optim_reference.make_state (two steps of history; computed once per case and route,
    handed out as copies) and fresh gradients; on the fast route vn2 of the tall matrix holds the true column sums of the
    stored parameters, rounded, as a whole Adam-WN step leaves them"""
    key = (case['name'], route)
    if key not in _STATES:
        _STATES[key] = R.make_state(case, route)
    table, n, n_cols, st = _STATES[key]
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    g, _ = R.make_grads(table, n, gseed)
    if route == 'fast':
        d = table[R.tall_index(table)]
        st['vn2'][d.col_offset:d.col_offset + d.cols] = R.true_sums(st['params'], st['s'], g, d)['A'].astype(F)
    return table, n, n_cols, st, g


def clip_args(variant, grads, table):
    """(clipnorm, clipvalue) of a variant: CLIP_FACTOR times the norm, the median |g|"""
    return (float(F(CLIP_FACTOR * norm64(grads, table))) if variant in ('clipnorm', 'both') else 0.0,
            median_abs(grads, table) if variant in ('clipvalue', 'both') else 0.0)


def clipped_ref(state, grads, descs, hyp, mode, known, scale32, clipvalue=0.0, decay=0.0, full_table=None):
    """optim_reference.ref_step of the clipped call: on g_eff (and gdot_eff, the known-sums form) from the given fp32 scale, with
    the decayed rate.  full_table: the table g_eff is formed over (default descs)."""
    ge = g_eff(grads, full_table or descs, scale32, clipvalue)
    if known is not None and known.get('use'):
        assert not clipvalue > 0, "refused by the contract"
        known = dict(known, gdot=gdot_eff(known['gdot'], scale32))
    t, _ = R.step_of(int(state['t']), mode)
    return R.ref_step(state, ge, descs, decayed_hyper(hyp, decay, t), mode, known), ge
