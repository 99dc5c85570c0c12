"""Latent paths in and out: encode a piece, decode a path, morph two pieces.

encode() reads a piece's latent path z_1..z_T off the encoder; decode() runs the decoder on a path of one's own (an edited
one, an averaged one, one read from a file); morph() is the standard demonstration of a VAE, and here also between two keys:
both pieces are encoded, their paths AND their labels mixed linearly on the device, and every mix decoded in one batch."""
import numpy as np
import torch

from .engine_generate import Constraints, lerp_rows, temper_args
from .vary import infer_labels


def _family(model):
    from .engine import VaeEngine
    if isinstance(model.engine, VaeEngine):
        from .cl_vae import model as M
    else:
        from .cl_vrnn import model as M
    return M, isinstance(model.engine, VaeEngine)


def _pieces(model, pieces, name='pieces'):
    x = np.asarray(pieces, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    D = model.engine.cfg['D']
    if x.ndim != 3 or x.shape[0] < 1 or x.shape[1] < 1 or x.shape[2] != D:
        raise ValueError("%s must be [N, T, %d] (or one piece [T, %d]) with N, T >= 1, got shape %s"
                         % (name, D, D, np.shape(pieces)))
    return x


def _labels(model, pieces, w, name='w'):
    cfg = model.engine.cfg
    N, C = pieces.shape[0], cfg['C']
    if w is None:
        _, is_vae = _family(model)
        if not is_vae and pieces.shape[1] < cfg['T']:
            raise ValueError("inferring the label needs at least seq_length = %d frames per piece, got %d"
                             % (cfg['T'], pieces.shape[1]))
        return infer_labels(model, pieces)
    w = np.asarray(w, dtype=np.float64)
    if w.shape == (C,):
        w = np.tile(w, (N, 1))
    if w.shape != (N, C):
        raise ValueError("%s must be [N, C] = %s (or [C]), got shape %s" % (name, (N, C), w.shape))
    return w


def encode(model, pieces, w=None, seed=0, z_temperature=1.0):
    """The latent paths of pieces [N, T, 88] (binary frames; one piece [T, 88] counts as N = 1) of any length T.  w [N, C]:
    the pieces' labels, which the encoder conditions on (None: inferred with the model's w-encoder as vary.infer_labels
    does; cl_vrnn then needs at least seq_length frames per piece).  Returns (z, z_mean, z_log_var), each [N, T, L] float64
    (encode_latents_device); z_temperature=0 gives z = z_mean."""
    M, _ = _family(model)
    x = _pieces(model, pieces)
    return M.encode_latents_device(model, x, _labels(model, x, w), seed=seed, z_temperature=z_temperature)


def decode(model, z, w, x0=None, history='own', seed=0, clamp=None, temperature=1.0, noise_rows=None, return_xhat=False):
    """Decode the latent paths z [N, T, L] under the labels w [N, C] (or [C], used for every path): decode_latents_device of
    the model's family.  Returns [N, T, 88] float64 (with return_xhat also the probabilities).  ValueError for a z whose last
    dimension is not the model's latent_dim."""
    M, _ = _family(model)
    cfg = model.engine.cfg
    z = np.asarray(z, dtype=np.float64)
    if z.ndim == 2:
        z = z[None]
    if z.ndim != 3 or z.shape[2] != cfg['L']:
        raise ValueError("z must be [N, T, %d], got shape %s" % (cfg['L'], z.shape))
    w = np.asarray(w, dtype=np.float64)
    if w.shape == (cfg['C'],):
        w = np.tile(w, (z.shape[0], 1))
    return M.decode_latents_device(model, z, w, x0=x0, history=history, seed=seed, clamp=clamp, temperature=temperature,
                                   noise_rows=noise_rows, return_xhat=return_xhat)


def morph(model, a, b, steps=8, w_a=None, w_b=None, z_temperature=0.0, common_noise=True, seed=0, temperature=1.0,
          clamp=None):
    """Interpolate between the pieces a and b ([pairs, T, 88] each, or one piece [T, 88] each; equal lengths) in latent
    space: both are encoded under their labels w_a, w_b ([pairs, C] or [C]; None: inferred as in encode), and for alpha_k =
    k / steps, k = 0..steps, the path (1 - alpha_k) z_a + alpha_k z_b is decoded under the label (1 - alpha_k) w_a + alpha_k
    w_b (a convex mix of two label rows stays on the simplex), the decoder running on its own output.  Paths and labels are
    mixed on the device (clv_lerp_rows: exact at both ends) and all steps + 1 rows of every pair are decoded in one batch.
    Returns [pairs, steps + 1, T, 88] float64: row 0 is a re-decoding of a, row `steps` one of b.

    z_temperature (default 0.0) is the encoder's latent temperature: at 0 the posterior MEANS are mixed.  With
    z_temperature > 0 the two paths carry independent noise, and a mix of two independently noised paths has LESS variance
    in the middle than at the ends (a factor (1 - alpha)^2 + alpha^2 = 1/2 at alpha = 1/2), so the middle rows would be
    decoded from tamer latents than the end rows; mixing the means keeps every row on the same footing.
    common_noise=True: every row of a pair draws the note uniforms of the pair's first row (noise_rows), so the rows differ
    through the path and the label only, not through the sampling noise.  Global row pair * (steps + 1) + k holds step k: with
    common_noise=False row 0 of a pair is vary(a) and row `steps` is vary(b) at those rows, bit for bit.
    clamp: uint8 roll [pairs, T, 88] (or [T, 88]) applied to every row of its pair, or a Constraints over the pairs (roll
    [pairs, T, 88] and / or voice counts; the decoding then runs on the frame chain).  ValueError for pieces of unequal
    length or count, steps < 1, wrong shapes, a bool or out-of-range temperature."""
    if isinstance(steps, (bool, np.bool_)) or int(steps) != steps or steps < 1:
        raise ValueError("steps must be an integer >= 1, got %r" % (steps,))
    K = int(steps)
    temper_args(temperature, z_temperature)
    a, b = _pieces(model, a, 'a'), _pieces(model, b, 'b')
    if a.shape != b.shape:
        raise ValueError("a and b must be as many pieces of equal length, got shapes %s and %s" % (a.shape, b.shape))
    w_a, w_b = _labels(model, a, w_a, 'w_a'), _labels(model, b, w_b, 'w_b')
    eng = model.engine
    cfg, d = eng.cfg, eng.device
    pairs, T, D = a.shape
    L, C, R = cfg['L'], cfg['C'], pairs * (K + 1)
    if isinstance(clamp, Constraints):      # roll and voice counts per pair, repeated for the pair's rows
        clamp = clamp.repeat_rows(K + 1).resolve(R, T, D, d)
    elif clamp is not None:
        clamp = np.asarray(clamp)
        if clamp.ndim == 2:
            clamp = clamp[None]
        if clamp.dtype != np.uint8 or clamp.shape != (pairs, T, D):
            raise ValueError("clamp must be uint8 %s, got %s %s" % ((pairs, T, D), clamp.dtype, clamp.shape))
        clamp = np.repeat(clamp, K + 1, axis=0)
    # Row (j, k) of the batch holds step k of pair j.  The encoder's noise follows the row, so a is encoded at the rows
    # k < steps and b at row k = steps: the end rows then carry exactly the latents vary() gives them there.
    is_b = (np.arange(R) % (K + 1)) == K
    src = np.where(is_b[:, None, None], np.repeat(b, K + 1, axis=0), np.repeat(a, K + 1, axis=0))
    w = np.where(is_b[:, None], np.repeat(w_b, K + 1, axis=0), np.repeat(w_a, K + 1, axis=0))
    f = dict(dtype=torch.float32, device=d)
    src_d, w_d = torch.as_tensor(src, **f), torch.as_tensor(w, **f).contiguous()
    zout = torch.zeros(3, R, T, L, **f)
    eng.vary(src_d, w_d, seed=int(seed), z_temperature=z_temperature, zout=zout)
    first = (np.arange(R) // (K + 1)) * (K + 1)
    alpha = (np.arange(R) % (K + 1)).astype(np.float64) / K
    z_mix = lerp_rows(zout[2].reshape(R, T * L), first, zout[2].reshape(R, T * L), first + K, alpha).reshape(R, T, L)
    w_mix = lerp_rows(w_d, first, w_d, first + K, alpha)
    Xs = eng.decode_latents(z_mix, w_mix, seed=int(seed), clamp=clamp, temperature=temperature,
                    noise_rows=first if common_noise else None)
    return Xs.cpu().numpy().astype(np.float64).reshape(pairs, K + 1, T, D)
