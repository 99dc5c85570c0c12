"""Shared data of the likelihood GPU test and its data-parallel worker: a cl_vrnn model with oracle-initialised weights
and 45 windows of sparse binary frames (not a test module)."""
import numpy as np

from oracle import clvae_oracle as O


def vrnn_case(dev, B=32, T=16, L=2, C=4, H=88, n=45, use_x_prev=True, seed=7):
    """(model, x, y, (p, cfg, X, Xp, wt)) -- model.engine holds the float32 values of p."""
    from clvae_amd.cl_vrnn.model import get_model
    cfg = O.vrnn_config(intermediate_dim=H, latent_dim=L, seq_length=T, n_classes=C, use_x_prev=use_x_prev)
    p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in O.vrnn_init_params(cfg, seed=seed).items()}
    model, _ = get_model(B, 88, H, L, T, C, use_x_prev, 'adam', seed=seed, device=dev)
    model.engine.P.set_weights(p)
    rng = np.random.default_rng(seed)
    win = (rng.random((n, T + 1, 88)) < 0.05).astype(np.float64)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(C)[rng.integers(0, C, n)]
    x = [X, Xp] if use_x_prev else X
    return model, x, [X, wt, wt, X], (p, cfg, X, Xp, wt)
