"""Classifying VAE -- key tracking CLI (no counterpart in the reference): the label head of a trained model on every frame
of every SONG of one split, HMM-smoothed: key accuracy per song, the confusion matrix, where the songs change
key.  One process, one GPU."""
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import clvae_amd  # noqa: E402,F401
from clvae_amd.keytrack import build_keys_parser, score_keys  # noqa: E402


def keys(args):
    from clvae_amd.cl_vae.model import load_model
    model, _, _ = load_model(args.model_file, batch_size=None)
    return score_keys(model, args)


def build_parser():
    return build_keys_parser()


if __name__ == '__main__':
    keys(build_parser().parse_args())
