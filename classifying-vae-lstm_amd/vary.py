"""Variations and key transfer: re-decode a piece's latent path.

The model is a CLASSIFYING VAE: the key w is a latent of its own, separate from the frame latents z_t.  vary() reads a
piece's latent path z_1..z_T off the encoder (teacher-forced on the piece, under the piece's own key) and decodes that path
again with the decoder running on its own output: under the same key it gives a variation of the piece, under another key
(transfer_key) the piece moved to that key.  The frame loop runs on the device (vary_samples_device of both families)."""
import numpy as np


def key_rows(to_key, N, C, key_map=None):
    """The decoder's label rows [N, C] float64 for vary(to_key=...): a class index (one-hot rows), a key name looked up in
    key_map (PianoData.key_map: name -> class index), or an array [N, C] (or [C], used for every piece).  ValueError for a
    bool, an index outside [0, C), an unknown name, a name without a key_map, a wrong shape."""
    if isinstance(to_key, (bool, np.bool_)):
        raise ValueError("to_key must be a class index, a key name or an [N, C] array, got %r" % (to_key,))
    if isinstance(to_key, str):
        if key_map is None:
            raise ValueError("to_key=%r is a key name: pass the key_map it is looked up in" % (to_key,))
        if to_key not in key_map:
            raise ValueError("unknown key %r (known: %s)" % (to_key, ", ".join(sorted(map(str, key_map)))))
        to_key = int(key_map[to_key])
    if isinstance(to_key, (int, np.integer)):
        if not 0 <= int(to_key) < C:
            raise ValueError("class index %d outside [0, %d)" % (int(to_key), C))
        return np.tile(np.eye(C)[int(to_key)], (N, 1))
    w = np.asarray(to_key, dtype=np.float64)
    if w.shape == (C,):
        w = np.tile(w, (N, 1))
    if w.shape != (N, C):
        raise ValueError("to_key as an array must be [N, C] = %s (or [C]), got shape %s" % ((N, C), w.shape))
    return w


def infer_labels(model, sources):
    """w [N, C] float64 of every piece from the model's own w-encoder, without label noise: cl_vrnn the mean over the
    piece's windows of seq_length frames (cl_vrnn.model.infer_label), cl_vae the mean over its frames"""
    from .engine import VaeEngine
    cfg = model.engine.cfg
    if isinstance(model.engine, VaeEngine):
        from .cl_vae import model as M
        w_enc = M.make_w_encoder(model, cfg['D'])
        return np.vstack([np.vstack([M.sample_w(w_enc.predict(f[None, :]), add_noise=False) for f in src]).mean(axis=0)
                          for src in sources])
    from .cl_vrnn import model as M
    w_enc = M.make_w_encoder(model, cfg['D'], cfg['C'], cfg['T'])
    return np.vstack([M.infer_label(w_enc, src, cfg['T']) for src in sources])


def vary(model, sources, w=None, to_key=None, key_map=None, x0=None, history='own', seed=0, clamp=None, temperature=1.0,
         z_temperature=1.0, return_xhat=False):
    """Re-decode sources [N, T, 88] (binary frames).  w [N, C]: the pieces' own labels, which the encoder conditions on
    (None: inferred with the model's w-encoder; cl_vrnn then needs at least seq_length frames per piece).  to_key: the label
    the decoder conditions on, see key_rows (None: w, a variation in the piece's own key).  The other arguments are
    vary_samples_device's.  Returns [N, T, 88] float64 (with return_xhat also the probabilities)."""
    from .engine import VaeEngine
    sources = np.asarray(sources, dtype=np.float64)
    if sources.ndim != 3:
        raise ValueError("sources must be [N, T, 88], got shape %s" % (sources.shape,))
    cfg = model.engine.cfg
    N, C = sources.shape[0], cfg['C']
    is_vae = isinstance(model.engine, VaeEngine)
    if w is None:
        if not is_vae and sources.shape[1] < cfg['T']:
            raise ValueError("inferring the label needs at least seq_length = %d frames per piece, got %d"
                             % (cfg['T'], sources.shape[1]))
        w = infer_labels(model, sources)
    w_dec = None if to_key is None else key_rows(to_key, N, C, key_map)
    if is_vae:
        from .cl_vae.model import vary_samples_device
    else:
        from .cl_vrnn.model import vary_samples_device
    return vary_samples_device(model, sources, w, w_dec, x0=x0, history=history, seed=seed, clamp=clamp,
                               temperature=temperature, z_temperature=z_temperature, return_xhat=return_xhat)


def transfer_key(model, sources, to_key, w=None, key_map=None, **kw):
    """vary() with the decoder's key given: the pieces re-decoded under `to_key` (an index, a name in key_map, or rows)"""
    if to_key is None:
        raise ValueError("transfer_key needs to_key")
    return vary(model, sources, w=w, to_key=to_key, key_map=key_map, **kw)
