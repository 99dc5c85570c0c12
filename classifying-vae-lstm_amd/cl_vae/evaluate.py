"""Classifying variational autoencoders -- scoring CLI (no counterpart in the reference): the importance-weighted
log-likelihood per frame row and Keras evaluate() of a trained model on one split, with the rows built
exactly as train.py builds its inputs.  One process, one GPU."""
import argparse
import json
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import clvae_amd  # noqa: E402,F401
from clvae_amd.cl_vae.model import load_model  # noqa: E402
from clvae_amd.cl_vae.train import flatten_windows  # noqa: E402
from clvae_amd.cli import parser_for, score_split  # noqa: E402
from clvae_amd.utils.model_utils import to_categorical  # noqa: E402
from clvae_amd.utils.pianoroll import PianoData  # noqa: E402


def evaluate(args):
    margs = json.load(open(args.model_file.replace('.h5', '.json')))
    model, _, margs = load_model(args.model_file, batch_size=margs['batch_size'])
    P = PianoData(args.train_file, batch_size=margs['batch_size'], seq_length=margs['seq_length'], step_length=1,
                  return_y_next=margs['predict_next'] or margs['use_x_prev'], squeeze_x=True, squeeze_y=True)
    if margs['seq_length'] > 1:
        flatten_windows(P, argparse.Namespace(**margs))
    w = to_categorical(getattr(P, args.split + '_song_keys'), margs['n_classes'])
    cur, hist = getattr(P, 'y_' + args.split), getattr(P, 'x_' + args.split)
    x = [cur, hist] if margs['use_x_prev'] else hist
    return score_split(model, x, [cur, w, w, cur], args, margs)


def build_parser():
    return parser_for('cl_vae.evaluate')


if __name__ == '__main__':
    evaluate(build_parser().parse_args())
